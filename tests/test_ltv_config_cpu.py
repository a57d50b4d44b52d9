"""Conditions on the inputs of tests/test_ltv_config_gpu.py, from the float64 oracle and the NumPy prototype of the kernels' working-set
rules alone: if these hold, a deviation of the kernels on the same inputs is the kernels'.  Nothing here needs a GPU."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from oracle.ltv_mpc_oracle import solve_mpcv
from tests import ltv_config_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CERT = 1e-7            # the bound of tests/test_ltv_mpc.py on the oracle's KKT residuals
PROTO_SWEEPS = 32      # half the handle's max_sweeps: keeps the GPU tests away from the cap
PROTO_TOL = 1e-7
MOVE = 1e-4            # every mutation moves the exact output by at least this (the comparison bound is 1e-6)

# every (configuration, T, delay) whose generated cases a GPU test solves
USED = sorted(set(cc.one_solve_grid()) | {(n, T, d) for n in cc.NAMES for T, d in cc.WARM + cc.CONVERGE + cc.THREAD + cc.MUTATION_SHAPES}
              | {("default", 30, 1)})


@functools.lru_cache(maxsize=None)
def prototype():
    """tools/ltv_ws_prototype.py, loaded where it lies"""
    spec = importlib.util.spec_from_file_location("ltv_ws_prototype", os.path.join(ROOT, "tools", "ltv_ws_prototype.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def solved(name, T, delay):
    """the exact solve of every case of a shape, once: [(output (2, T), certificate, rollout)]"""
    p, cs = cc.cases(name, T, delay)
    res = []
    for now, out, buff, xref, dref in cs:
        ref, _, info, xbar = solve_mpcv(now, out, buff, xref, dref, p)
        res.append((ref, max(info.values()), xbar))
    return res


def test_the_two_configurations_reach_the_handle_as_the_oracle_has_them():
    for name in cc.NAMES:
        p, cfg = cc.config_pair(name, 18, 1)
        assert (cfg.dt, cfg.predict_steps, cfg.delay_num) == (p.dt, p.T, p.delay_num)
        assert tuple(cfg.matrix_q) == p.Q and tuple(cfg.matrix_r) == p.R and tuple(cfg.matrix_rd) == p.Rd
        assert (cfg.max_vel, cfg.max_omega, cfg.max_acc, cfg.max_domega) == (p.max_speed, p.max_omega, p.max_accel, p.max_domega)
        assert cfg.max_sweeps == 64
        # what the default configuration cannot see
        assert p.Q[2] > 0 and min(p.R) > 0 and p.Q[0] != p.Q[1] and p.R[0] != p.R[1] and p.Rd[0] != p.Rd[1]
        assert p.max_speed != p.max_omega and p.max_accel != p.max_domega
    assert cc.params("dt02", 18, 1).dt == 0.02 and cc.params("asym", 18, 1).dt == 0.01
    p, cfg = cc.config_pair("default", 30, 1)
    assert tuple(cfg.matrix_q) == p.Q and tuple(cfg.matrix_r) == p.R and (cfg.max_vel, cfg.max_omega) == (p.max_speed, p.max_omega)


@pytest.mark.parametrize("name,T,delay", USED)
def test_oracle_certifies_itself_and_the_prototype_settles_on_it(name, T, delay):
    p, cs = cc.cases(name, T, delay)
    assert len(cs) == cc.B
    worst_cert, worst_dev, most = 0.0, 0.0, 0
    for (ref, cert, xbar), case in zip(solved(name, T, delay), cs):
        u, sweeps, settled = prototype().ws_riccati(xbar, case[3], case[4], p)
        assert settled and sweeps <= PROTO_SWEEPS, (name, T, delay, sweeps)
        worst_cert = max(worst_cert, cert); most = max(most, sweeps)
        worst_dev = max(worst_dev, float(np.max(np.abs(u.T - ref[:, delay:]))))
    print(f"{name} T {T} delay {delay}: certificate {worst_cert:.1e}, prototype sweeps {most}, |prototype - exact| {worst_dev:.1e}")
    assert worst_cert < CERT and worst_dev < PROTO_TOL, (worst_cert, worst_dev)
    # the rollout's clamp acts: a previous yaw rate beyond max_omega in a column the rollout integrates
    assert sum(cc.clamped(c, p) for c in cs) >= 1


@pytest.mark.parametrize("name", cc.NAMES)
@pytest.mark.parametrize("T,delay", cc.MUTATION_SHAPES)
def test_every_mutation_moves_the_exact_output(name, T, delay):
    """four cases: a kernel that drops or exchanges one of these parameters is at least MOVE off the oracle in one of them"""
    _, cs = cc.cases(name, T, delay)
    base = solved(name, T, delay)
    for what, change in cc.MUTATIONS:
        moved = max(float(np.max(np.abs(cc.mutated_output(cs[i], name, T, delay, change) - base[i][0]))) for i in range(4))
        print(f"{name} T {T} delay {delay}: {what}: {moved:.2e}")
        assert moved >= MOVE, (what, moved)


@pytest.mark.parametrize("name", cc.NAMES)
def test_every_kind_of_bound_row_is_active_at_the_active_shape(name):
    T, delay = cc.ACTIVE_SHAPE
    p = cc.params(name, T, delay)
    total = {}
    for ref, _, _ in solved(name, T, delay):
        for kind, n in cc.active_rows(ref, p).items():
            total[kind] = total.get(kind, 0) + n
    print(name, total)
    assert all(n >= 1 for n in total.values()) and len(total) == 4, total
