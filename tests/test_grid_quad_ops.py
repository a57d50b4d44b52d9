"""The quad-native group operations (csrc/nmpc_group_ops.h) inside the N = 20 grid kernel: the (4, 5) mapping, one iteration per launch.

A problem's four lanes are one DPP quad; the prediction's scans and sums, the forward sweep's scan and the maxima permute inside it.
A wrong permutation or a missing mask shows as a result that depends on the neighbours of a problem, so next to the oracle the tests
move the problems around and ask for the same bits.  B = 37 is two full blocks of 16 problems and a ragged one of 5; the prediction
runs a fixed number of steps (warm_start_steps) in every engine.  Needs a real MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from alore_legged_manipulator_amd.scenarios import make_batch, make_wide_batch, problem  # noqa: E402
from oracle.drivers import Oracle  # noqa: E402

BLOCK = 0x100  # ALORE_NMPC_BLOCK_LANES(L) = 0x100 | L (include/alore_nmpc.h)
N, B37, PG = 20, 37, 4
OUT = ("x", "u", "dual", "status", "n_iter", "kkt", "obj")


def relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@pytest.fixture(scope="module")
def nmpc_mod():
    from alore_legged_manipulator_amd import nmpc
    return nmpc


def engine(nmpc_mod, B, **kw):
    return nmpc_mod.BatchedNmpc(B, N, lanes_per_problem=BLOCK | 4, warm_start_steps=PG, **kw)


def solve(nmpc_mod, batch, **kw):
    eng = engine(nmpc_mod, batch["x"].shape[0], **kw)
    eng.load(batch)
    eng.rti(1)
    out = eng.fetch()
    assert eng.launch_info()["lanes_per_problem"] == (BLOCK | 4)
    return out


@pytest.fixture(scope="module")
def bench37(nmpc_mod):
    """the bench distribution and its solution (never modified)"""
    batch = make_batch(B37, N, seed=909, fast_tail=0.3)
    out = solve(nmpc_mod, batch)
    for v in out.values():
        v.setflags(write=False)
    return batch, out


@pytest.fixture(scope="module")
def wide37(nmpc_mod):
    """the stress distribution and its solution (never modified)"""
    batch = make_wide_batch(B37, N, 20261004)
    out = solve(nmpc_mod, batch)
    for v in out.values():
        v.setflags(write=False)
    return batch, out


def test_bench_distribution_matches_the_oracle(bench37):
    """members and tolerances of test_gpu_parity.py::test_one_tick_matches_oracle"""
    batch, out = bench37
    orc = Oracle(N)
    for b in range(B37):
        orc.reset(); orc.initialize_solver(); orc.load(problem(batch, b)); orc.preparation_step()
        assert orc.feedback_step() == 0 and out["status"][b] == 0, b
        assert relerr(out["x"][b].reshape(-1), orc.v["x"]) < 1e-4, (b, "x")
        assert relerr(out["u"][b].reshape(-1), orc.v["u"]) < 1e-4, (b, "u")
        assert 1 <= out["n_iter"][b] <= 16


def test_stress_distribution_matches_the_oracle(wide37):
    """the rule of test_gpu_parity.py::test_stage_block_kernel_on_the_stress_distribution, on every problem of the batch"""
    from tests.test_gpu_parity import check_against_oracle_and_float64
    batch, out = wide37
    assert (out["status"] == 0).all()
    check_against_oracle_and_float64(batch, out, batch["u"], list(range(B37)), N, "quad ops, stress")


@pytest.mark.parametrize("dist", ["bench", "stress"])
def test_a_problem_does_not_see_its_neighbours(nmpc_mod, bench37, wide37, dist):
    """the 37 problems in another order: other quads beside each, another block, the ragged one for some: the same bits"""
    batch, want = bench37 if dist == "bench" else wide37
    perm = np.random.default_rng(37).permutation(B37)
    got = solve(nmpc_mod, {k: v[perm] for k, v in batch.items()})
    for k in OUT:
        assert np.array_equal(want[k][perm], got[k]), k


@pytest.mark.parametrize("dist", ["bench", "stress"])
def test_three_slots_in_flight_equal_a_launch_alone(nmpc_mod, bench37, wide37, dist):
    """rti_range over 3 slots (one grid) and rti(1) on each slot alone: the same bits for the same problems.  Both engines hold the
    three slots (the comparison of test_grid_wavefront_ends.py: a slot's place in memory is the same on both sides); the slots hold
    the batch in three orders, and slot 0, in the order of the fixture, also returns the fixture's bits."""
    import torch
    batch, want = bench37 if dist == "bench" else wide37
    slots = 3
    perms = [np.arange(B37), np.roll(np.arange(B37), 5), np.arange(B37)[::-1].copy()]
    eng = engine(nmpc_mod, B37, slots=slots)
    ref = engine(nmpc_mod, B37, slots=slots)
    for s in range(slots):
        eng.load({k: v[perms[s]] for k, v in batch.items()}, slot=s)
        ref.load({k: v[perms[s]] for k, v in batch.items()}, slot=s)
    eng.rti_range(0, slots)
    for s in range(slots):
        ref.rti(1, slot=s)
    torch.cuda.synchronize()
    for k in OUT:
        assert torch.equal(eng.ts[k], ref.ts[k]), k
        assert np.array_equal(eng.ts[k][0].cpu().numpy().reshape(want[k].shape), want[k]), k
