"""The device FlatTrajData builder (alore_backend_set_paths), the device predicted state and the masked plan launch on the GPU.

Oracle of the builder: alore_legged_manipulator_amd.flat_traj (NumPy), 1e-10 absolute like the CPU test of the same arithmetic
(test_flat_traj_build_cpu.py; the paths come from the same generator, which rejects paths whose piece count a last-ulp difference
decides).  Everything else is compared bit for bit: the optimiser is deterministic and independent of batch mates, so a plan of
device-built problems equals the plan of the same numbers uploaded through set_problems, and a slot the mask leaves out keeps its
bytes.  max_pieces = 16, a 20 m map (free, or with boxes)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from alore_legged_manipulator_amd.flat_traj import FrontEndParams
from tests import flat_traj_cases as cases

pytestmark = pytest.mark.gpu

TOL = 1e-10
HALF, RES = 10.0, 0.1
PRM_CUT = FrontEndParams(traj_cut_length=4.0)
RESULT_KEYS = ("ok", "attempts", "alm_rounds", "evals", "lbfgs_ret", "path_ret", "collision", "n_pieces", "cost", "min_dist", "tail_s",
               "xy_err", "inner", "T", "coef")
PROBLEM_KEYS = ("n_pieces", "inner", "init_T", "positions", "head", "tail", "start_xytheta", "final_xy", "if_cut")


def box_map(boxes):
    """distance to the nearest of the axis-aligned boxes (x0, x1, y0, y1), negative inside; 100 without boxes"""
    n = int(round(2 * HALF / RES))
    c = (np.arange(n) + 0.5) * RES - HALF
    X, Y = np.meshgrid(c, c, indexing="ij")
    d = np.full((n, n), 100.0)
    for x0, x1, y0, y1 in boxes:
        dx = np.maximum(np.maximum(x0 - X, X - x1), 0.0)
        dy = np.maximum(np.maximum(y0 - Y, Y - y1), 0.0)
        inside = np.minimum(np.minimum(X - x0, x1 - X), np.minimum(Y - y0, y1 - Y))
        d = np.minimum(d, np.where(inside > 0, -inside, np.hypot(dx, dy)))
    return d


def planner(n, boxes=()):
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    pl = BatchedMSPlanner(n, 16)
    pl.set_map(box_map(boxes), -HALF, -HALF, RES)
    return pl


def same_bytes(a, b, keys, idx_a=None, idx_b=None):
    for k in keys:
        x = a[k] if idx_a is None else a[k][idx_a]
        y = b[k] if idx_b is None else b[k][idx_b]
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), k


def as_flat_trajs(pr, idx):
    """the problem slots `idx` of problems() as what set_problems takes"""
    out = []
    for b in idx:
        M = int(pr["n_pieces"][b])
        pts = np.zeros((M - 1, 3)); pts[:, :2] = pr["inner"][b, :M - 1]
        pos = np.zeros((M - 1, 3)); pos[:, :2] = pr["positions"][b, :M - 1]
        out.append(SimpleNamespace(traj_pts=pts, positions=pos, init_T=float(pr["init_T"][b]), start_state=pr["head"][b], final_state=pr["tail"][b],
                                   start_xytheta=pr["start_xytheta"][b], final_xytheta=np.array([*pr["positions"][b, M - 1], 0.0]),
                                   if_cut=bool(pr["if_cut"][b])))
    return out


def against_the_oracle(pr, b, ft):
    M = ft.pieces
    assert pr["n_pieces"][b] == M and pr["if_cut"][b] == int(ft.if_cut), (b, pr["n_pieces"][b], M)
    pairs = [(pr["init_T"][b], ft.init_T), (pr["inner"][b, :M - 1], ft.traj_pts[:, :2]), (pr["positions"][b, :M - 1], ft.positions[:, :2]),
             (pr["positions"][b, M - 1], ft.final_xytheta[:2]), (pr["head"][b], ft.start_state), (pr["tail"][b], ft.final_state),
             (pr["start_xytheta"][b], ft.start_xytheta), (pr["final_xy"][b], ft.final_xytheta[:2])]
    for k, (a, e) in enumerate(pairs):
        assert np.max(np.abs(np.asarray(a) - np.asarray(e)), initial=0.0) <= TOL, (b, k, a, e)
    assert not pr["inner"][b, M - 1:].any() and not pr["positions"][b, M:].any()  # the rest of the rows is zero, as set_problems leaves it


def device_inputs(paths, K):
    import torch
    npts, xy, sy, ey, vaj, oaj = cases.pack(paths, K)
    return [torch.from_numpy(a).cuda() for a in (npts, xy, sy, ey, vaj, oaj)]


@pytest.fixture(scope="module")
def paths64():
    out, rejected = cases.make_paths(64, PRM_CUT, max_pieces=16)
    assert rejected <= 4
    return out


@pytest.fixture(scope="module")
def built64(paths64):
    """64 paths through the host route on a map with two boxes"""
    pl = planner(64, boxes=[(-1.0, 1.0, -1.0, 1.0), (4.0, 5.0, -6.0, -3.0)])
    pl.set_paths([p[0] for p in paths64], [p[1] for p in paths64], [p[2] for p in paths64], np.array([p[3] for p in paths64]),
                 np.array([p[4] for p in paths64]), params=PRM_CUT)
    return pl


def test_builder_against_the_oracle(paths64, built64):
    import torch
    pr = built64.problems()
    assert (built64.build_status() == 0).all()
    for b, p in enumerate(paths64):
        against_the_oracle(pr, b, cases.oracle(p, PRM_CUT))
    assert len(set(pr["n_pieces"])) >= 4 and pr["if_cut"].any() and not pr["if_cut"].all()
    # the device-pointer route: the same bits
    dv = planner(64)
    n, xy, sy, ey, vaj, oaj = device_inputs(paths64, 6)
    dv.set_paths_device(64, 6, n, xy, sy, ey, vaj, oaj, params=PRM_CUT)
    torch.cuda.synchronize()
    assert (dv.build_status() == 0).all()
    same_bytes(dv.problems(), pr, PROBLEM_KEYS)


def test_same_slots_same_plans(built64):
    built64.plan()
    r = built64.results()
    pr = built64.problems()
    other = planner(64, boxes=[(-1.0, 1.0, -1.0, 1.0), (4.0, 5.0, -6.0, -3.0)])
    other.set_problems(as_flat_trajs(pr, range(64)))
    same_bytes(other.problems(), pr, PROBLEM_KEYS)
    other.plan()
    same_bytes(other.results(), r, RESULT_KEYS)
    assert r["ok"].sum() >= 32  # the batch is not a batch of failures


def test_overflow_and_bad_input(paths64):
    import torch
    from alore_legged_manipulator_amd.backend import BackendError
    prm = FrontEndParams()
    zeros = np.zeros(3)
    long_one = (np.array([[-9.0, 0.0], [9.0, 0.0]]), 0.0, 0.0, zeros, zeros)
    seventeen = None
    for x1 in np.arange(0.0, 9.0, 0.05):  # the two-point path along y = 0 from x = -9 that needs exactly 17 pieces
        cand = (np.array([[-9.0, 0.0], [float(x1), 0.0]]), 0.0, 0.0, zeros, zeros)
        if cases.oracle(cand, prm).pieces == 17 and not cases.on_a_knife_edge(cand, prm):
            seventeen = cand
            break
    assert seventeen is not None and cases.oracle(long_one, prm).pieces > 17
    one_point = (np.array([[1.0, 2.0]]), 0.0, 0.0, zeros, zeros)
    good = [(p[0], p[1], p[2], zeros, zeros) for p in paths64]  # from rest, without the cut
    good = [p for p in good if cases.oracle(p, prm).pieces <= 16 and not cases.on_a_knife_edge(p, prm)][:4]
    assert len(good) == 4
    pl = planner(4)

    def host(paths):
        pl.set_paths([p[0] for p in paths], [p[1] for p in paths], [p[2] for p in paths], params=prm)

    with pytest.raises(BackendError, match="-5"):
        host([good[0], seventeen, good[1]])
    assert list(pl.build_status(3)) == [0, -2, 0]
    with pytest.raises(BackendError, match="-1"):
        host([good[0], one_point, good[1]])
    assert list(pl.build_status(3)) == [0, -1, 0]
    # the device route: the slot of a path that does not build is unchanged, its neighbours are built
    host(good)
    before = pl.problems()
    new = [good[3], seventeen, one_point, good[0]]
    n, xy, sy, ey, _, _ = device_inputs(new, 6)
    pl.set_paths_device(4, 6, n, xy, sy, ey, params=prm)
    torch.cuda.synchronize()
    assert list(pl.build_status()) == [0, -2, -1, 0]
    after = pl.problems()
    same_bytes(after, before, PROBLEM_KEYS, [1, 2], [1, 2])
    against_the_oracle(after, 0, cases.oracle(good[3], prm))
    against_the_oracle(after, 3, cases.oracle(good[0], prm))


# ---- a fleet of 16 on the free map: slot b drives along y = YS[b] from x = -3 to the right
YS = -5.5 + 0.7 * np.arange(16)
BOX = (-0.4, 0.4, -1.0, 1.0)  # crosses the lanes with |y| < 1 (slots 7, 8, 9); the next lanes are 0.3 and 0.5 m away from it


def fleet_paths():
    return [np.array([[-3.0, y], [3.0 + 0.3 * (b % 4), y]]) for b, y in enumerate(YS)]


def detour_paths():
    """around the box over (0, 1.8); the first point is overwritten with the predicted position"""
    return [np.array([[-3.0, y], [0.0, 1.8], [3.0 + 0.3 * (b % 4), y]]) for b, y in enumerate(YS)]


@pytest.fixture()
def fleet():
    pl = planner(16)
    pl.set_paths(fleet_paths(), 0.0, 0.0)
    pl.plan()
    return pl


def test_predicted_state_device_gives_the_bits_of_the_host_call(fleet):
    import torch
    r = fleet.results()
    total = r["T"].sum(axis=1)
    times = np.ascontiguousarray(total * np.linspace(0.1, 0.9, 16))
    st = np.ascontiguousarray(times * 0.25)
    sx = np.ascontiguousarray(np.stack([np.full(16, -2.5), YS + 0.05, np.full(16, 0.02)], 1))
    for with_start in (False, True):
        want = fleet.predicted_state(times, 0.01, st if with_start else None, sx if with_start else None)
        xyt, vaj, oaj = (torch.zeros(16, 3, dtype=torch.float64, device="cuda") for _ in range(3))
        fwd = torch.zeros(16, dtype=torch.int32, device="cuda")
        fleet.predicted_state_device(16, torch.from_numpy(times).cuda(), xyt, vaj, oaj, fwd, 0.01,
                                     torch.from_numpy(st).cuda() if with_start else None, torch.from_numpy(sx).cuda() if with_start else None)
        torch.cuda.synchronize()
        got = {"xytheta": xyt.cpu().numpy(), "vaj": vaj.cpu().numpy(), "oaj": oaj.cpu().numpy()}
        same_bytes(got, want, ("xytheta", "vaj", "oaj"))
        assert (fwd.cpu().numpy().astype(bool) == want["forward"]).all()
        assert np.abs(want["vaj"][:, 0]).max() > 0.1


def test_masked_replan(fleet):
    import torch
    r0, p0 = fleet.results(), fleet.problems()
    fleet.set_map(box_map([BOX]), -HALF, -HALF, RES)
    flags = fleet.check_plans()["collision"].astype(bool)
    assert flags.sum() >= 2 and (~flags).sum() >= 2, flags
    # everything the cycle reads is resident before it starts
    s = torch.cuda.Stream()
    n, xy, sy, ey, _, _ = device_inputs([(p, 0.0, 0.0, np.zeros(3), np.zeros(3)) for p in detour_paths()], 3)
    times = torch.full((16,), 0.5, dtype=torch.float64, device="cuda")
    xyt, vaj, oaj = (torch.zeros(16, 3, dtype=torch.float64, device="cuda") for _ in range(3))
    fwd = torch.zeros(16, dtype=torch.int32, device="cuda")
    # a spin kernel holds the stream back while the host issues the whole cycle: had any call of the cycle waited for the stream
    # (or the device), the spin would be over when the last call returns.  Its length is measured first (about half a second).
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        torch.cuda._sleep(1000)  # loads the kernel
        e0.record(s); torch.cuda._sleep(20_000_000); e1.record(s)
    e1.synchronize()
    cycles = int(20_000_000 * 500.0 / max(e0.elapsed_time(e1), 1e-3))
    torch.cuda.synchronize()
    gate = torch.cuda.Event()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        gate.record(s)
        fleet.check_plans(stream=s, fetch=False)
        fleet.predicted_state_device(16, times, xyt, vaj, oaj, fwd, 0.01, stream=s)
        xy[:, 0, :] = xyt[:, :2]
        sy.copy_(xyt[:, 2])
        fleet.set_paths_device(16, 3, n, xy, sy, ey, vaj, oaj, mask=fleet.check_mask(), stream=s)
        fleet.plan(mask=fleet.check_mask(), stream=s)
        still_held_back = not gate.query()
    r1 = fleet.results(stream=s)
    assert still_held_back, "a call of the cycle waited for the stream"
    p1 = fleet.problems()
    status = fleet.build_status()
    assert (status[flags] == 0).all() and (status[~flags] == 1).all(), status
    keep, redo = np.flatnonzero(~flags), np.flatnonzero(flags)
    same_bytes(r1, r0, RESULT_KEYS, keep, keep)
    same_bytes(p1, p0, PROBLEM_KEYS, keep, keep)
    # the rebuilt slots start at the predicted state and were planned again
    got = {"xytheta": xyt.cpu().numpy(), "vaj": vaj.cpu().numpy(), "oaj": oaj.cpu().numpy()}
    assert np.array_equal(p1["start_xytheta"][redo], got["xytheta"][redo])
    assert np.array_equal(p1["head"][redo][:, 1, 1], got["vaj"][redo][:, 0]) and (got["vaj"][redo][:, 0] > 0.1).all()
    fresh = planner(len(redo), boxes=[BOX])
    fresh.set_problems(as_flat_trajs(p1, redo))
    fresh.plan()
    same_bytes(fresh.results(), r1, RESULT_KEYS, None, redo)


def test_unmasked_plan_is_unchanged_by_masked_calls(fleet):
    import torch
    r0 = fleet.results()
    mask = torch.zeros(16, dtype=torch.int32, device="cuda")
    mask[::3] = 1
    fleet.plan(mask=mask)
    same_bytes(fleet.results(), r0, RESULT_KEYS)  # deterministic: the planned slots get the same bits, the others keep theirs
    fleet.plan()
    same_bytes(fleet.results(), r0, RESULT_KEYS)
    fleet.plan(mask=torch.ones(16, dtype=torch.int32, device="cuda"))
    same_bytes(fleet.results(), r0, RESULT_KEYS)
