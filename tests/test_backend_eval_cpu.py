"""The oracle side of tests/test_backend_eval_gpu.py, on the CPU: oracle/backend_oracle.c is a restatement that only its own checks
pin, and tests/test_backend_oracle.py runs those on the default config alone.  Here every case of tests/backend_eval_cases.py is
pinned -- the gradient against central differences of the cost -- and every claim of the case table is asserted on the oracle:
which penalty terms change the cost, which do not, and which branches the inputs reach.  These conditions keep the GPU comparison
from going vacuous: a case whose term never fires compares zeros."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import backend_eval_cases as cases  # noqa: E402


@pytest.fixture(scope="module")
def orc():
    from oracle.backend_driver import BackendOracle
    return BackendOracle()


@pytest.fixture(scope="module")
def table():
    return {c.name: c for c in cases.build_cases()}


NAMES = [c.name for c in cases.build_cases()]


def costs(orc, case, **more):
    with cases.oracle_config(orc, case.overrides, **more):
        return np.array([orc.eval(cases.grids()[case.grid], ft, case.stage, x, **case.kw)["cost"] for ft, x in zip(case.fts, case.xs)])


def test_the_table_covers_what_it_is_for(table):
    """exact piece counts, every M of both builds, every check-point count of the pair loop, launches of at most 64 problems"""
    assert all(len(c.fts) <= 64 and len(c.fts) == len(c.xs) for c in table.values())
    assert sorted(ft.pieces for ft in table["pieces16-s2-default"].fts) == list(range(1, 17))
    assert [ft.pieces for ft in table["pieces16-s2-default"].fts] != list(range(1, 17))        # submitted shuffled
    assert [ft.pieces for ft in table["pieces32-s2-default"].fts] == [1, 2, 16, 17, 24, 31, 32]
    assert {c.overrides["n_check"] for c in table.values() if c.axis == "obstacle"} == {0, 1, 2, 3, 7, 8}
    assert all(ft.pieces == cases.M_CONFIG for c in table.values() if c.axis in ("config", "obstacle") for ft in c.fts)
    pts = np.array(cases.CHECK_PTS)
    assert len({tuple(p) for p in pts}) == 8
    for sx, sy in ((-1, 1), (1, -1), (-1, -1)):                     # no check point is the mirror image of another
        assert not any(np.allclose(p * (sx, sy), q) for p in pts for q in pts)
    for stage in (1, 2):
        assert any(c.stage == stage and {"tau_pos", "tau_neg", "tau_zero"} <= c.branches for c in table.values())


@pytest.mark.parametrize("name", NAMES)
def test_oracle_gradient_matches_central_differences(orc, table, name):
    """exact_chain = 1 wherever the reference's chain is knowingly inexact (the ICR model, the obstacle term), and the cost must not
    depend on that switch.  Free maps: 1e-5 of the largest entry.  Obstacle cases: the 2e-4 of tests/test_backend_oracle.py (the
    smoothed-L1 of a bilinear field is C1 only).  Stage 1 charges two different time weights in cost and gradient (reference quirk):
    made equal for this check, as in tests/test_backend_oracle.py."""
    case = table[name]
    grid = cases.grids()[case.grid]
    kw = dict(case.kw, time_weight=orc.cfg.p_time) if case.stage == 1 else case.kw
    bound = 1e-5 if case.grid == "free" else 2e-4
    worst = 0.0
    for ft, x in zip(case.fts, case.xs):
        with cases.oracle_config(orc, case.overrides, exact_chain=0):
            plain = orc.eval(grid, ft, case.stage, x, **kw)
        with cases.oracle_config(orc, case.overrides, exact_chain=case.exact_chain_for_fd):
            r = orc.eval(grid, ft, case.stage, x, **kw)
            fd = cases.fd_grad(orc, grid, ft, case.stage, x, **kw)
        assert r["cost"] == plain["cost"]                            # bit-equal between exact_chain 0 and 1
        err = float(np.max(np.abs(fd - r["grad"])) / np.max(np.abs(fd)))
        worst = max(worst, err)
        assert err <= bound, (name, ft.pieces, err)
    print(f"{name}: worst |fd - grad| / max|fd| {worst:.1e} (bound {bound:.0e})")


@pytest.mark.parametrize("name", NAMES)
def test_terms_are_active_where_the_table_says_so(orc, table, name):
    """zeroing the weight of an active term changes the cost of at least one problem of the launch; zeroing the weight of any other
    term of the stage leaves the bits of every cost alone"""
    case = table[name]
    base = costs(orc, case)
    assert np.all(np.isfinite(base)) and np.all(base > 0)
    for term, weight in cases.WEIGHT_OF[case.stage].items():
        without = costs(orc, case, **{weight: 0.0})
        changed = without != base
        if term in case.active:
            assert changed.any(), (name, term, changed)
        else:
            assert not changed.any(), (name, term, changed)


@pytest.mark.parametrize("name", NAMES)
def test_inputs_reach_the_branches_the_table_names(orc, table, name):
    """a scan in NumPy of the violations at the oracle's spline nodes: the named faces / limits are in violation, the durations sit on
    the named sides of tau = 0, smooth_eps = 1e-6 leaves no violation in the quartic branch and 10.0 none in the linear one, and an
    obstacle case has a check point outside the map and one inside it in violation"""
    case = table[name]
    with cases.oracle_config(orc, case.overrides):
        got = cases.reached(orc, case)
    assert case.branches <= got, (name, sorted(case.branches - got), sorted(got))
    eps = case.overrides.get("smooth_eps")
    if eps is not None:
        assert ("only_linear" if eps == 1e-6 else "only_quartic") in case.branches


def test_direct_v_omega_is_ignored_at_stage_1(orc, table):
    a, b = table["s1-direct-is-ignored"], table["s1-polygon-slow"]
    assert a.overrides["direct_v_omega"] == 1 and "direct_v_omega" not in b.overrides
    assert np.array_equal(costs(orc, a), costs(orc, b))
    c2 = costs(orc, table["s2-direct-slow"])
    assert np.all(c2 != costs(orc, table["s2-polygon-slow"]))       # ... and not at stage 2
