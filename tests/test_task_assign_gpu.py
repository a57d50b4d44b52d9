"""The modes of alore_backend_task_plan that choose the item-to-target assignment (ALORE_BE_TASK_ASSIGNED, ALORE_BE_TASK_JOINT) on the
GPU against the sequential oracle of tests/task_assign_cases.py.

Every comparison with the oracle is ==, the two rows of the new slab included.  Both slabs are pre-filled before a launch, so
whatever must stay untouched shows.  Maps have at most 64 x 48 cells at 0.1 m."""
import ctypes as C

import numpy as np
import pytest

from tests import task_assign_cases as cases
from tests import task_plan_cases as tc
from tests.test_task_plan_gpu import _hip, _params, pair, planner
from tests.test_task_plan_gpu import prefill as prefill_task

pytestmark = pytest.mark.gpu

KEYS = ("matrix", "order", "total", "leg_start_xy", "leg_goal_xy", "assignment", "assign_total")
SLAB = ("status", "matrix", "order", "n_order", "total", "leg_start_xy", "leg_goal_xy", "fields", "sweeps", "assignment", "assign_total")
MODES = [cases.ASSIGNED, cases.JOINT]
IDS = ["assigned", "joint"]


def prefill(pl, n):
    """rows 0..n-1 of both slabs: every int -9, every coordinate -777"""
    prefill_task(pl, n)
    hip, v = _hip(), pl.device_task_assign()
    for ptr, shape in ((v.assignment, (n, cases.MAX_TASKS)), (v.assign_total, (n, 2))):
        a = np.full(shape, cases.FILL_I, np.int32)
        assert hip.hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1) == 0          # hipMemcpyHostToDevice


def result(pl, n):
    return {**pl.task_result(n), **pl.task_assignment(n)}


def same_as_oracle(got, b, want, where):
    w = cases.expected_arrays(want)
    for k in ("status", "n_order", "fields"):
        assert int(got[k][b]) == w[k], (where, k, int(got[k][b]), w[k])
    for k in KEYS:
        assert np.array_equal(got[k][b], w[k]), (where, k, got[k][b], w[k])
    assert (got["sweeps"][b] == cases.FILL_I) if want.fields is None else got["sweeps"][b] >= 1, (where, got["sweeps"][b])


def plan_scene(name, pl=None, assignment="scene", mode=None):
    """the scene through the host route on pre-filled slabs: (results, return code of the call, planner)"""
    s = cases.get_scene(name)
    n_tasks, pts, asg = cases.arrays(s)
    if assignment != "scene":
        asg = assignment
    n = len(n_tasks)
    if pl is None:
        pl = planner(n)
    pl.set_map(s["map"].dist, s["map"].x_lo, s["map"].y_lo, s["map"].res)
    prefill(pl, n)
    rc = pl.L.alore_backend_task_plan(pl.h, n, s["max_tasks"], n_tasks.ctypes.data, pts.ctypes.data, pts.strides[0],
                                      None if asg is None else asg.ctypes.data, C.byref(_params({**s, "mode": s["mode"] if mode is None else mode})),
                                      0, None, 4, None)
    return result(pl, n), rc, pl


def host_return_code(want):
    """the existing rule: the first failed mission decides; tasks, end point and no order are ALORE_BE_E_INVALID"""
    return -1 if any(w.status < 0 for w in want) else 0


@pytest.mark.parametrize("name", cases.SCENES)
def test_scenes_equal_the_oracle(name):
    got, rc, _ = plan_scene(name)
    want = cases.expected(name)
    for b, w in enumerate(want):
        same_as_oracle(got, b, w, (name, b))
    assert rc == host_return_code(want)


def test_the_scenes_show_what_they_are_named_for():
    a, _, pl = plan_scene("crossed:assigned")
    ident, _, _ = plan_scene("crossed:assigned", pl, mode=tc.OPTIMAL)
    assert a["assignment"][0, :2].tolist() == [1, 0] and cases.less(pair(a["total"][0]), pair(ident["total"][0]))
    t, _, pl = plan_scene("tie:assigned")
    assert t["assignment"][0, :3].tolist() == [1, 0, 2]
    a, _, pl = plan_scene("joint_beats_assigned:assigned")
    j, _, _ = plan_scene("joint_beats_assigned:joint", pl)
    assert a["status"][0] == j["status"][0] == 0 and cases.less(pair(j["total"][0]), pair(a["total"][0]))
    assert cases.less(pair(a["assign_total"][0]), pair(j["assign_total"][0]))
    u, rc, _ = plan_scene("unroutable:assigned")
    assert rc == -1 and u["status"][0] == cases.E_NO_ORDER and u["n_order"][0] == 0 and u["assignment"][0, :2].tolist() == [0, 1]
    assert u["assign_total"][0, 0] > 0 and (u["order"][0] == cases.FILL_I).all() and (u["total"][0] == cases.FILL_I).all()
    m, rc, _ = plan_scene("too_many:joint")
    assert rc == -1 and m["status"].tolist() == [cases.E_TASKS, cases.E_TASKS, 0] and m["n_order"].tolist() == [0, 0, 10]


@pytest.mark.parametrize("mode", IDS)
def test_a_given_assignment_is_not_read(mode):
    name = "ignored_assignment:" + mode
    with_garbage, rc, pl = plan_scene(name)
    assert rc == 0 and cases.arrays(cases.scene(name))[2].tolist() == [[0, 0], [7, -1]]
    without, rc, _ = plan_scene(name, pl, assignment=None)
    assert rc == 0
    for k in SLAB:
        assert with_garbage[k].tobytes() == without[k].tobytes(), k
    _, rc, _ = plan_scene(name, pl, mode=tc.OPTIMAL)                       # the optimal mode reads it and refuses it
    assert rc == -1


@pytest.mark.parametrize("mode", MODES, ids=IDS)
@pytest.mark.parametrize("route", ["host", "device"])
def test_random_missions_equal_the_oracle(route, mode):
    """64 missions of mixed n in one launch: from host arrays, and from device tensors whose rows are 24 points apart"""
    import torch
    name = ("random", mode)
    want = cases.expected(name)
    n = len(want)
    assert n == 64 and sum(w.status == cases.OK for w in want) >= 48 and sum(w.status == cases.E_NO_ORDER for w in want) >= 1
    if route == "host":
        got, rc, _ = plan_scene(name)
        assert rc == -1
    else:
        s = cases.get_scene(name)
        n_tasks, pts, _ = cases.arrays(s)
        pl = planner(n, s["map"])
        prefill(pl, n)
        T = s["max_tasks"]
        wide = torch.full((n, 1 + 2 * T + 3, 2), float("nan"), dtype=torch.float64, device="cuda")
        wide[:, :1 + 2 * T] = torch.from_numpy(pts)
        d_n = torch.from_numpy(n_tasks).cuda()
        torch.cuda.synchronize()
        pl.task_plan_device(n, T, d_n, wide, mode=mode, safe_dis=s["safe_dis"], window_margin=s["margin"])
        got = result(pl, n)
    for b, w in enumerate(want):
        same_as_oracle(got, b, w, (route, mode, b))


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_a_masked_out_mission_keeps_every_byte_of_both_slabs(mode):
    import torch
    s = cases.random_scene(mode)
    n_tasks, pts, _ = cases.arrays(s)
    want = cases.expected(("random", mode))
    n, T = 6, s["max_tasks"]
    pl = planner(n, s["map"])
    prefill(pl, n)
    pl.task_plan(n_tasks[:n], pts[:n], mode=mode, safe_dis=s["safe_dis"], window_margin=s["margin"], check=False)
    first = result(pl, n)
    flags = np.array([1, 0, 1, 0, 0, 1], np.int32)
    words = torch.zeros(n, 2, dtype=torch.int32, device="cuda")            # the words next to the mask words say the opposite
    words[:, 0] = torch.from_numpy(flags)
    words[:, 1] = torch.from_numpy(1 - flags)
    d_n, d_pts = torch.from_numpy(n_tasks[n:2 * n].copy()).cuda(), torch.from_numpy(pts[n:2 * n].copy()).cuda()
    torch.cuda.synchronize()
    pl.task_plan_device(n, T, d_n, d_pts, mode=mode, safe_dis=s["safe_dis"], window_margin=s["margin"], mask=words[:, 0])
    got = result(pl, n)
    for b in range(n):
        if flags[b]:
            w = want[n + b]
            assert got["status"][b] == w.status
            if w.assignment is not None:
                assert got["assignment"][b, :w.n].tolist() == w.assignment and pair(got["assign_total"][b]) == w.assign_total
            if w.status == 0:
                assert got["order"][b, :len(w.order)].tolist() == w.order and pair(got["total"][b]) == w.total
        else:
            assert got["status"][b] == cases.MASKED
            for k in SLAB[1:]:
                assert got[k][b].tobytes() == first[k][b].tobytes(), (b, k)


def test_the_optimal_mode_leaves_the_new_slab_alone_and_computes_what_it_did():
    """mode 1 after mode 2 on one handle: the new slab keeps the bytes mode 2 wrote, the results equal those of a fresh handle"""
    s2, s1 = cases.random_scene(cases.ASSIGNED), tc.random_scene(tc.OPTIMAL)
    n = 64
    after2, _, pl = plan_scene(("random", cases.ASSIGNED))
    n_tasks, pts, asg = tc.arrays(s1)
    pl.task_plan(n_tasks, pts, asg, mode=tc.OPTIMAL, safe_dis=s1["safe_dis"], window_margin=s1["margin"], check=False)
    after1 = result(pl, n)
    for k in ("assignment", "assign_total"):
        assert after1[k].tobytes() == after2[k].tobytes(), k
    fresh = planner(n, s1["map"])
    prefill(fresh, n)
    fresh.task_plan(n_tasks, pts, asg, mode=tc.OPTIMAL, safe_dis=s1["safe_dis"], window_margin=s1["margin"], check=False)
    alone = result(fresh, n)
    assert (alone["assignment"] == cases.FILL_I).all() and (alone["assign_total"] == cases.FILL_I).all()
    want = tc.expected(("random", tc.OPTIMAL))
    for b in range(n):
        assert after1["status"][b] == alone["status"][b] == want[b].status and after1["n_order"][b] == alone["n_order"][b]
        P, L = want[b].P, len(want[b].order)
        assert np.array_equal(after1["matrix"][b, :P, :P], alone["matrix"][b, :P, :P])
        if want[b].status == 0:
            for k in ("order", "leg_start_xy", "leg_goal_xy"):
                assert after1[k][b, :L].tobytes() == alone[k][b, :L].tobytes(), (b, k)
            assert after1["total"][b].tobytes() == alone["total"][b].tobytes() and after1["order"][b, :L].tolist() == want[b].order


def test_the_assigned_mode_equals_the_optimal_mode_given_its_assignment():
    s = cases.random_scene(cases.ASSIGNED)
    n_tasks, pts, _ = cases.arrays(s)
    n = len(n_tasks)
    a, _, pl = plan_scene(("random", cases.ASSIGNED))
    given = np.where(a["assignment"] == cases.FILL_I, 0, a["assignment"]).astype(np.int32)
    given[a["assignment"][:, 0] == cases.FILL_I] = np.arange(cases.MAX_TASKS)     # no matching: any permutation, the identity
    prefill(pl, n)
    pl.task_plan(n_tasks, pts, given, mode=tc.OPTIMAL, safe_dis=s["safe_dis"], window_margin=s["margin"], check=False)
    o = result(pl, n)
    assert (a["status"] == 0).sum() >= 48
    for b in range(n):
        if a["assignment"][b, 0] == cases.FILL_I:
            continue
        assert o["status"][b] == a["status"][b]
        for k in ("order", "total", "leg_start_xy", "leg_goal_xy", "n_order"):
            assert o[k][b].tobytes() == a[k][b].tobytes(), (b, k)


@pytest.mark.parametrize("mode", IDS)
def test_the_order_phase_alone_writes_what_the_call_wrote(mode):
    """task_reorder on the matrices in the slab: the rows of the new slab are wiped in between and come back"""
    name = "joint_beats_assigned:" + mode
    first, _, pl = plan_scene(name)
    hip, v = _hip(), pl.device_task_assign()
    wiped = np.full(cases.MAX_TASKS, cases.FILL_I, np.int32)
    assert hip.hipMemcpy(v.assignment, wiped.ctypes.data, wiped.nbytes, 1) == 0
    assert (pl.task_assignment(1)["assignment"] == cases.FILL_I).all()
    pl.task_reorder()
    again = result(pl, 1)
    for k in SLAB:
        assert again[k].tobytes() == first[k].tobytes(), k
    same_as_oracle(again, 0, cases.expected(name)[0], name)


def test_the_chain_from_the_assigned_mode_to_the_search_of_the_first_carry_leg():
    """task_plan_device(mode=ASSIGNED) -> search_paths_device on leg 1 as it lies in the slab: the first carry leg, from the first
    item of the order to the target the returned assignment names for it"""
    import torch
    s = cases.scene("crossed:assigned")
    n_tasks, pts, _ = cases.arrays(s)
    pl = planner(1, s["map"])
    prefill(pl, 1)
    d_n, d_pts = torch.from_numpy(n_tasks).cuda(), torch.from_numpy(pts).cuda()
    torch.cuda.synchronize()
    pl.task_plan_device(1, s["max_tasks"], d_n, d_pts, mode=cases.ASSIGNED, safe_dis=s["safe_dis"], window_margin=s["margin"])
    v = pl.device_task()
    pl.search_paths_device(1, v.leg_start_xy + 16, v.leg_goal_xy + 16, start_stride=16 * v.max_legs, goal_stride=16 * v.max_legs,
                           safe_dis=s["safe_dis"], window_margin=s["margin"])
    got, paths = result(pl, 1), pl.paths(1)
    assert pl.search_status(1)[0] == 0 and got["status"][0] == 0
    item = int(got["order"][0, 0])
    target = int(got["assignment"][0, item])
    assert target == int(got["order"][0, 1]) == [1, 0][item]
    assert paths["xy"][0, 0].tolist() == list(pts[0, 1 + item]) and paths["xy"][0, paths["n_points"][0] - 1].tolist() == list(pts[0, 3 + target])
    assert not cases.less(pair(paths["cost_ab"][0]), pair(got["matrix"][0, 1 + item, 3 + target]))
