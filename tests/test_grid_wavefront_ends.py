"""The two ends of a wavefront of the N = 20 grid kernel (the (4, 5) mapping, one iteration per launch).

Head: a full block of 16 problems brings W and y into LDS by a straight line of DMA pieces, a ragged block by the guarded form.
Tail: the terminal weights / reference the objective needs wait in the padding behind the W image, and on the diagonal-weights
path the iterate waits in the dead off-diagonal entries of the lane's own W records, instead of being read from global memory a
second time.  All of it only moves data, so every comparison between two launches here is bit for bit.

B = 37 is two full blocks and a ragged block of 5.  The prediction runs a fixed number of steps (warm_start_steps) in every
engine, so that no two launches compared here differ in it.  Needs a real MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from alore_legged_manipulator_amd.scenarios import make_batch, problem  # noqa: E402
from oracle.drivers import Oracle  # noqa: E402

BLOCK = 0x100  # ALORE_NMPC_BLOCK_LANES(L) = 0x100 | L (include/alore_nmpc.h)
N, B37, PG = 20, 37, 4
OUT = ("x", "u", "dual", "status", "n_iter", "kkt", "obj")


def relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def head(batch, n):
    return {k: v[:n].copy() for k, v in batch.items()}


@pytest.fixture(scope="module")
def nmpc_mod():
    from alore_legged_manipulator_amd import nmpc
    return nmpc


def engine(nmpc_mod, B, **kw):
    return nmpc_mod.BatchedNmpc(B, N, lanes_per_problem=BLOCK | 4, warm_start_steps=PG, **kw)


def solve(nmpc_mod, batch, **kw):
    B = batch["x"].shape[0]
    eng = engine(nmpc_mod, B, **kw)
    eng.load(batch)
    eng.rti(1)
    out = eng.fetch()
    assert eng.launch_info()["lanes_per_problem"] == (BLOCK | 4)
    return out


@pytest.fixture(scope="module")
def base37(nmpc_mod):
    """the batch most tests start from and its solution (never modified)"""
    batch = make_batch(B37, N, seed=808, fast_tail=0.3)
    out = solve(nmpc_mod, batch)
    assert (out["status"] == 0).all()
    for v in out.values():
        v.setflags(write=False)
    return batch, out


@pytest.fixture(scope="module")
def oracle37(base37):
    """one tick of the oracle on every problem of the batch: status, members, KKT value, objective"""
    batch, _ = base37
    orc = Oracle(N)
    res = []
    for b in range(B37):
        orc.reset()
        orc.initialize_solver()
        orc.load(problem(batch, b))
        orc.preparation_step()
        st = orc.feedback_step()
        res.append((st, {k: orc.v[k].copy() for k in ("x", "u", "dual", "d", "evGx", "evGu")}, orc.get_kkt(), orc.get_objective()))
    return res


def test_one_tick_matches_the_oracle_with_diagnostics(nmpc_mod, base37, oracle37):
    """members and tolerances of test_gpu_parity.py::test_one_tick_matches_oracle, and the objective (the member that sees a wrong
    terminal weight or reference) within 1e-4 relative, the bound test_sqp_iterations_in_kernel holds it to"""
    batch, out = base37
    eng = engine(nmpc_mod, B37)
    eng.load(batch)
    lin = eng.linearize()
    for b in range(B37):
        st, ref, kkt, obj = oracle37[b]
        assert st == 0 and out["status"][b] == 0
        assert np.max(np.abs(lin["d"][b].reshape(-1) - ref["d"])) < 2e-6
        assert np.max(np.abs(lin["evGx"][b].reshape(-1) - ref["evGx"])) < 2e-6
        assert np.max(np.abs(lin["evGu"][b].reshape(-1) - ref["evGu"])) < 2e-6
        assert relerr(out["x"][b].reshape(-1), ref["x"]) < 1e-4, (b, "x")
        assert relerr(out["u"][b].reshape(-1), ref["u"]) < 1e-4, (b, "u")
        assert relerr(out["dual"][b].reshape(-1), ref["dual"]) < 1e-3, (b, "dual")
        assert abs(out["kkt"][b] - kkt) <= 2e-3 * max(1.0, kkt), (b, out["kkt"][b], kkt)
        assert abs(out["obj"][b] - obj) <= 1e-4 * max(1.0, abs(obj)), (b, out["obj"][b], obj)
        assert 1 <= out["n_iter"][b] <= 16


def test_one_tick_matches_the_oracle_without_diagnostics(nmpc_mod, base37, oracle37):
    batch, with_diag = base37
    eng = engine(nmpc_mod, B37, diagnostics=False)
    eng.load(batch)
    eng.t["kkt"].fill_(-7.0); eng.t["obj"].fill_(-7.0)
    eng.rti(1)
    out = eng.fetch()
    for b in range(B37):
        st, ref, _, _ = oracle37[b]
        assert st == 0 and out["status"][b] == 0
        assert relerr(out["x"][b].reshape(-1), ref["x"]) < 1e-4, (b, "x")
        assert relerr(out["u"][b].reshape(-1), ref["u"]) < 1e-4, (b, "u")
        assert relerr(out["dual"][b].reshape(-1), ref["dual"]) < 1e-3, (b, "dual")
        assert 1 <= out["n_iter"][b] <= 16
    assert (out["kkt"] == -7.0).all() and (out["obj"] == -7.0).all()  # untouched
    for k in ("x", "u", "dual", "status", "n_iter"):
        assert np.array_equal(out[k], with_diag[k]), k


def test_full_block_path_equals_guarded_path(nmpc_mod):
    """the same problems in a full block (straight-line DMA) and in a ragged one (guarded DMA): equal bits"""
    batch16 = make_batch(16, N, seed=809, fast_tail=0.3)
    full = solve(nmpc_mod, batch16)
    five = solve(nmpc_mod, head(batch16, 5))
    one = solve(nmpc_mod, head(batch16, 1))
    assert (full["status"] == 0).all()
    for k in OUT:
        assert np.array_equal(five[k], full[k][:5]), k
        assert np.array_equal(one[k], full[k][:1]), k


def test_shared_members_return_the_bits_of_the_replicated_batch(nmpc_mod, base37):
    batch = {k: v.copy() for k, v in base37[0].items()}
    for k in ("W", "WN", "lbValues", "ubValues", "od"):
        batch[k][:] = batch[k][0]
    want = solve(nmpc_mod, batch)
    poisoned = {k: v.copy() for k, v in batch.items()}
    for k in ("W", "WN", "lbValues", "ubValues", "od"):
        poisoned[k][1:] = np.nan  # rows > 0 of a shared member are never read
    eng = engine(nmpc_mod, B37)
    eng.load(poisoned)
    eng.set_shared_members(W=True, bounds=True, od=True)
    eng.rti(1)
    got = eng.fetch()
    assert (got["status"] == 0).all()
    for k in OUT:
        assert np.array_equal(got[k], want[k]), k


def test_masked_problems_untouched_and_the_others_unchanged(nmpc_mod, base37):
    batch, want = base37
    mask = np.ones(B37, np.uint8); mask[[3, 20, 35]] = 0  # one per block, 35 in the ragged one
    broken = {k: v.copy() for k, v in batch.items()}
    broken["y"][20] = np.nan; broken["yN"][35] = np.nan; broken["x0"][3] = np.inf  # stale / non-finite references of idle robots
    eng = engine(nmpc_mod, B37)
    eng.load(broken)
    for k in ("status", "n_iter"):
        eng.ts[k][0].fill_(-7)
    for k in ("kkt", "obj"):
        eng.ts[k][0].fill_(123.5)
    before = eng.fetch()
    eng.set_problem_mask(mask)
    eng.rti(1)
    got = eng.fetch()
    on, off = mask == 1, mask == 0
    for k in OUT:
        assert np.array_equal(got[k][off], before[k][off], equal_nan=True), k
        assert np.array_equal(got[k][on], want[k][on]), k


def test_one_general_weights_wavefront_between_diagonal_ones(nmpc_mod, base37):
    """a 1e-38 off-diagonal entry sends the middle block down the general-weights body (global re-read of the iterate, the stash for the
    terminal cost): it agrees to 2e-6 like test_diagonal_weight_path_agrees_with_the_general_path, the other blocks do not notice"""
    batch, a = base37
    tweaked = {k: v.copy() for k, v in batch.items()}
    tweaked["W"][20, 3, 0, 1] = 1e-38; tweaked["W"][20, 3, 1, 0] = 1e-38
    b = solve(nmpc_mod, tweaked)
    assert (b["status"] == 0).all()
    wave = np.arange(16, 32)
    rest = np.setdiff1d(np.arange(B37), wave)
    for k in ("x", "u", "dual", "kkt", "obj"):
        assert np.array_equal(a[k][rest], b[k][rest]), k
        d = np.max(np.abs(a[k][wave].astype(np.float64) - b[k][wave])) / max(1.0, float(np.max(np.abs(a[k][wave]))))
        assert d < 2e-6, (k, d)
    assert np.array_equal(a["n_iter"], b["n_iter"])


def test_three_slots_in_flight_equal_the_slots_one_by_one(nmpc_mod):
    import torch
    slots = 3
    batches = [make_batch(B37, N, seed=900 + s, fast_tail=0.3) for s in range(slots)]
    eng = engine(nmpc_mod, B37, slots=slots)
    ref = engine(nmpc_mod, B37, slots=slots)
    for s in range(slots):
        eng.load(batches[s], slot=s)
        ref.load(batches[s], slot=s)
    eng.rti_range(0, slots)
    for s in range(slots):
        ref.rti(1, slot=s)
    torch.cuda.synchronize()
    assert (eng.ts["status"] == 0).all()
    for k in OUT:
        assert torch.equal(eng.ts[k], ref.ts[k]), k
