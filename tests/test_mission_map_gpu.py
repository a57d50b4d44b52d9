"""The edits of missions in the resident map on the GPU (alore_backend_map_paint, alore_backend_mission_*) against the sequential
oracle of tests/mission_cases.py.

Everything is compared for EQUALITY: the state grid after every call, the edit list as bytes, status, phase and goal indices,
n_changed, the box and n_skipped.  Every operation that decides a cell or a rule is a correctly rounded double operation, one
narrowing to float or an integer operation, and contraction is off in csrc/mission_map.h.

Shapes: the 64 x 48 map of the occupancy tests (an x / y stride swap shows) at 0.1 m from (-3.2, -2.4); lists of 300 edits (more
than one workgroup of the cell pass, many overlaps); 300 mission slots (more than one round of the compacting workgroup and more
than four wavefronts), up to 10 tasks each."""
import ctypes as C

import numpy as np
import pytest

from tests import mission_cases as cases
from tests import occupancy_cases as occ

pytestmark = pytest.mark.gpu
KEYS = ("status", "phase", "goal_item", "goal_target", "goal_status")


def planner(n=1):
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    pl = BatchedMSPlanner(n, 16)
    pl.map_create(occ.NX, occ.NY, occ.X_LO, occ.Y_LO, occ.RES, detection_range=occ.RANGE, perspective=0)
    return pl


def _hip_runtime():
    """the HIP runtime this process already runs on (the one torch loaded)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def counts(pl):
    import torch  # noqa: F401  (loads the HIP runtime)
    hip = _hip_runtime()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    v = pl.map_device()
    out = []
    for ptr in (v.count_hit, v.count_all):
        a = np.full((v.nx, v.ny), -1, np.int32)
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemcpy(a.ctypes.data, ptr, a.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        out.append(a)
    return out


def on_device(edits):
    import torch
    return torch.from_numpy(np.ascontiguousarray(edits).view(np.uint8).copy()).cuda()


def same_mission(pl, snap, what):
    st = pl.mission_state()
    for key in KEYS:
        assert np.array_equal(st[key], snap[key]), (what, key, np.argwhere(st[key] != snap[key])[:8])
    assert len(st["edits"]) == len(snap["edits"]) and st["edits"].tobytes() == snap["edits"].tobytes(), (what, len(st["edits"]), len(snap["edits"]))
    grid = pl.map_state()["grid"]
    assert np.array_equal(grid, snap["grid"]), (what, np.argwhere(grid != snap["grid"])[:8])
    assert (st["n_changed"], tuple(st["box"]), st["n_skipped"]) == (snap["n_changed"], tuple(snap["box"]), snap["n_skipped"]), what


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
def test_host_lists_equal_the_oracle():
    pl = planner()
    before = pl.map_state()
    for k, (edits, (grid, n, box, skipped)) in enumerate(zip(cases.paint_calls(), cases.paint_expected())):
        c = pl.map_paint(cases.as_array(edits))
        st = pl.map_state()
        assert np.array_equal(st["grid"], grid), (k, np.argwhere(st["grid"] != grid)[:8])
        assert (c["n_changed"], c["box"], c["n_skipped"]) == (n, box, skipped), k
        assert np.array_equal(st["log_odds"], before["log_odds"]), k          # only the state grid is written
        hit, total = counts(pl)
        assert not hit.any() and not total.any(), k
    first = cases.paint_expected()[0][0]
    assert sorted(set(np.argwhere(first[:, 24] == 2)[:, 0].tolist())) == [2, 4, 6] + list(range(35, 45))   # the two pinned edits
    c = pl.map_paint(np.zeros(0, cases.EDIT_DTYPE))                            # an empty list: the counters of "nothing"
    assert (c["n_changed"], c["box"], c["n_skipped"]) == (0, (occ.NX, occ.NY, -1, -1), 0)


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
def test_a_device_list_is_read_up_to_its_device_count():
    import torch
    edits = cases.as_array(cases.seeded_edits() + [(0.0, 0.0, 3.1, 2.3, 1)] * 100)     # 300 ... 399: locks all over the map
    m = cases.new_map()
    n, box, _ = cases.paint_list(m, cases.seeded_edits())
    pl = planner()
    d_edits, d_count = on_device(edits), torch.tensor([300], dtype=torch.int32, device="cuda")
    pl.map_paint_device(d_edits, d_count)
    assert d_edits.numel() == 400 * 40
    c = pl.paint_counters()
    grid = pl.map_state()["grid"]
    assert np.array_equal(grid, m.grid), np.argwhere(grid != m.grid)[:8]
    assert (c["n_changed"], c["box"], c["n_skipped"]) == (n, box, 0)
    whole = cases.new_map()
    assert cases.paint_list(whole, [tuple(edits[300])])[0] > 1000                      # a single one applied would show
    # a NaN edit and an oversized one are skipped and counted
    bad = cases.seeded_edits()
    bad.insert(17, (float("nan"), 0.0, 0.5, 0.5, 1))
    bad.insert(211, (0.0, 0.0, 3.2, 0.5, 1))
    pl2 = planner()
    pl2.map_paint_device(on_device(cases.as_array(bad)), torch.tensor([302], dtype=torch.int32, device="cuda"))
    c = pl2.paint_counters()
    assert np.array_equal(pl2.map_state()["grid"], m.grid)
    assert (c["n_changed"], c["box"], c["n_skipped"]) == (n, box, 2)
    from alore_legged_manipulator_amd.backend import BackendError
    with pytest.raises(BackendError, match="not finite"):                       # the same list from the host is refused
        pl2.map_paint(cases.as_array(bad))
    assert np.array_equal(pl2.map_state()["grid"], m.grid)


def test_a_device_list_longer_than_one_launch_is_cut_in_order():
    """8500 small edits in device memory on a fresh handle, which has 8192 descriptors: two launches.  The later edit still wins
    across the cut, so the grid is the oracle's; the counters add up per launch, so n_changed is at least the oracle's"""
    import torch
    rng = np.random.default_rng(21)
    edits = [(round(float(x), 2), round(float(y), 2), h, h, int(v)) for x, y, h, v in
             zip(rng.uniform(-3.3, 3.3, 8500), rng.uniform(-2.5, 2.5, 8500), rng.choice([0.0, 0.1, 0.2], 8500), rng.uniform(size=8500) < 0.5)]
    m = cases.new_map()
    n, box, _ = cases.paint_list(m, edits)
    tail = cases.new_map()
    cases.paint_list(tail, edits[8192:])
    assert (tail.grid != 0).sum() > 500                                        # the second launch has work to do
    pl = planner()
    pl.map_paint_device(on_device(cases.as_array(edits)), torch.tensor([8500], dtype=torch.int32, device="cuda"))
    c = pl.paint_counters()
    grid = pl.map_state()["grid"]
    assert np.array_equal(grid, m.grid), np.argwhere(grid != m.grid)[:8]
    assert c["n_changed"] >= n and c["box"] == box and c["n_skipped"] == 0


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
def test_paint_then_update_esdf_is_build_esdf_of_the_fetched_grid():
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    pl, ref = planner(), BatchedMSPlanner(1, 16)
    pl.map_paint(cases.as_array(cases.seeded_edits()[:40]))
    pl.map_update_esdf((0.03, 0.07), occ.RANGE)
    st = pl.map_state()
    d = ref.build_esdf(st["grid"], occ.X_LO, occ.Y_LO, occ.RES, (0.03, 0.07), occ.RANGE)
    assert np.array_equal(st["dist"], d)
    assert (d < 1e300).any() and (d <= 0).any() and (d > 0.3).any()


# ---- 4, 5 -------------------------------------------------------------------------------------------------------------------
def mission_planner():
    pl = planner(cases.SLOTS)
    pl.mission_create()
    return pl


def test_missions_equal_the_oracle_after_every_call():
    pl = mission_planner()
    for k, (name, args, snap) in enumerate(cases.mission_expected()):
        if name == "set":
            n, pts, kinds, mask = args
            pl.mission_set(n, pts, kinds, mask)
        elif name == "goals":
            pl.mission_set_goals(args[0], args[1])
        else:
            pl.mission_step(args[0], args[1])                                 # rows of x, y, yaw: the stride is 24
        same_mission(pl, snap, (k, name))


def test_three_steps_back_to_back_on_a_side_stream():
    """poses and masks are device memory, nothing is fetched in between: one fetch at the end gives the state after step 3"""
    import torch
    calls = cases.mission_expected()
    pl = mission_planner()
    n, pts, kinds, mask = calls[0][1]
    T = cases.T
    d = dict(n=torch.from_numpy(n).cuda(), pts=torch.from_numpy(pts).cuda(), kinds=torch.from_numpy(kinds).cuda(), mask=torch.from_numpy(mask).cuda(),
             goals=torch.from_numpy(calls[1][1][0]).cuda(), gmask=torch.from_numpy(calls[1][1][1]).cuda())
    steps = [(torch.from_numpy(p).cuda(), None if a is None else torch.from_numpy(a).cuda()) for _, (p, a), _ in calls[2:]]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    pl.mission_set_device(cases.SLOTS, T, d["n"], d["pts"], 16 * (1 + 2 * T), d["kinds"], d["mask"], stream=st)
    pl.mission_set_goals(d["goals"], d["gmask"], stride=16, stream=st, count=cases.SLOTS)
    for poses, after in steps:
        pl.mission_step(poses, after, stride=24, stream=st, count=cases.SLOTS)
    same_mission(pl, calls[4][2], "after step 3")


# ---- 6 ----------------------------------------------------------------------------------------------------------------------
def test_error_paths_and_a_masked_slot():
    from alore_legged_manipulator_amd.backend import BackendError, BatchedMSPlanner
    bare = BatchedMSPlanner(4, 16)
    row = np.zeros((4, 21, 2))
    row[:, 1, 0], row[:, 2, 0] = (0.5, 1.0, 1.5, 2.0), (-0.5, -1.0, -1.5, -2.0)
    for call in (lambda: bare.map_paint([(0.0, 0.0, 0.5, 0.5, 1)]), lambda: bare.mission_create(), lambda: bare.mission_set([1] * 4, row),
                 lambda: bare.mission_set_goals(row[:, 1]), lambda: bare.mission_step(row[:, 1])):
        with pytest.raises(BackendError, match="no resident map"):
            call()
    assert bare.L.alore_backend_map_paint(bare.h, None, 0, None, 0, None) == -1
    assert b"no resident map" in bare.L.alore_backend_last_error(bare.h)
    pl = planner(4)
    with pytest.raises(BackendError, match="mission_create"):
        pl.mission_set([1] * 4, row)
    n = np.ones(4, np.int32)
    assert pl.L.alore_backend_mission_set(pl.h, 4, 10, n.ctypes.data, row.ctypes.data, 21 * 16, None, 0, None, 0, None) == -1
    assert b"mission_create" in pl.L.alore_backend_last_error(pl.h)
    assert not pl.map_state()["grid"].any()                                   # nothing was painted
    pl.mission_create()
    with pytest.raises(BackendError, match="stride"):
        pl.mission_step(1 << 20, stride=12, count=4)                          # refused before anything is read
    # a slot the mask leaves out is untouched: its status, phase and goals stay, and its items are not painted again
    o = cases.Missions(cases.new_map(), 4)
    for who in (pl, o):
        (who.mission_set if who is pl else who.set)([1] * 4, row)
        (who.mission_set_goals if who is pl else who.set_goals)(row[:, 1])
    assert (o.phase == cases.PHASE_ITEM).all()
    moved = row.copy()
    moved[:, 1, 1] = 1.0
    pl.mission_set([1] * 4, moved, mask=[1, 0, 0, 1])
    o.set([1] * 4, moved, mask=[1, 0, 0, 1])
    assert list(o.phase) == [0, 1, 1, 0] and len(o.edits) == 2
    same_mission(pl, o.snapshot(), "masked")


# ---- 7 ----------------------------------------------------------------------------------------------------------------------
def test_check_plans_and_search_paths_see_the_items():
    """the point of it: a plan through an item's square is flagged once the items are painted, and no longer once the item is
    freed; a path to a goal beside a locked target goes round the target's cells"""
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    from alore_legged_manipulator_amd.flat_traj import straight_goal
    pl = BatchedMSPlanner(2, 16)
    pl.set_free_map(6.0)
    pl.minco_plan([straight_goal((-1.5, -1.0, 0.0), (1.5, -1.0, 0.0)), straight_goal((-1.5, 1.1, 0.0), (1.5, 1.1, 0.0))])
    pl.map_create(occ.NX, occ.NY, occ.X_LO, occ.Y_LO, occ.RES, detection_range=occ.RANGE, perspective=0)
    pl.mission_create()
    row = np.zeros((2, 21, 2))
    row[0, 1], row[0, 2] = (0.0, -1.0), (0.5, 0.3)      # the item lies on the first plan, the target between the plans
    row[1, 1], row[1, 2] = (9.0, 9.0), (9.0, -9.0)      # the second robot's mission is off the map
    pl.mission_set([1, 1], row)
    pl.map_update_esdf((0.0, 0.0))
    assert list(pl.check_plans(min_safe_dis=0.2)["collision"]) == [1, 0]
    pl.mission_set_goals(row[:, 1])                     # heading to the items
    pl.mission_step([(1.0, -1.0), (0.0, 0.0)], esdf_odom=(0.0, 0.0))          # the first robot is 1 m from its item: freed
    st = pl.mission_state()
    assert len(st["edits"]) == 1 and st["edits"]["make_obs"][0] == 0 and st["n_changed"] > 0
    assert list(pl.check_plans(min_safe_dis=0.2)["collision"]) == [0, 0]
    pl.mission_set_goals(row[:, 2])                     # heading to the targets
    pl.mission_step([(0.75, 0.3), (0.0, 0.0)], esdf_odom=(0.0, 0.0))          # delivered: the target's square is locked
    grid = pl.map_state()["grid"]
    m = cases.new_map()
    cases.paint_list(m, [(0.0, -1.0, 0.5, 0.5, 0), (0.5, 0.3, 0.3, 0.3, 1)])
    assert np.array_equal(grid, m.grid) and grid[37, 27] == 2 and 36 <= (grid == 2).sum() <= 49   # the square round (0.5, 0.3)
    pl.search_paths([(-0.8, 0.3), (-0.8, 0.3)], [(1.3, 0.3), (1.3, 0.3)])     # the goal is 0.8 m beside the target, the start across it
    assert list(pl.search_status()) == [0, 0]
    paths = pl.paths()
    xy = paths["xy"][0][:paths["n_points"][0]]
    assert len(xy) >= 3                                 # not the straight line
    for a, b in zip(xy[:-1], xy[1:]):
        for t in np.linspace(0.0, 1.0, 200):
            p = a + t * (b - a)
            assert grid[int((p[0] - occ.X_LO) / occ.RES), int((p[1] - occ.Y_LO) / occ.RES)] != 2, p
