"""alore_backend_manager_* on the GPU against the oracle of tests/fleet_manager_cases.py: 70 robots (two wavefronts, the second
partial) through 12 ticks of scripted requests, poses, statuses and durations, every array of alore_backend_get_manager compared BIT
FOR BIT after every tick.  The scripted statuses go in through the pointer arguments of manager_end; the signs of the ESDF come from
a small resident map painted with map_set_grid and built by map_update_esdf."""
import numpy as np
import pytest

from tests import fleet_manager_cases as cases

pytestmark = pytest.mark.gpu
same = cases.same


def make_planner(B, params=None, manager=True):
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    pl = BatchedMSPlanner(B, 16)
    assert pl.P == cases.P
    pl.map_create(cases.NX, cases.NY, cases.X_LO, cases.Y_LO, cases.RES, detection_range=8.0, perspective=0)
    pl.map_set_grid(cases.grid_of_map())
    pl.map_update_esdf((0.0, 0.0))
    if manager:
        pl.manager_create(**(params or {}))
    return pl


def dev(a, dtype):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def snapshot(pl, n):
    g = pl.get_manager(n)
    return g["ints"], g["doubles"], np.array([g["counters"][k] for k in cases.COUNTERS[:7]] + [0], np.int32)


def run_device(pl, sc, n, host_begin=False):
    """the scenario through the device calls: (snapshots after every T and L step, the predicted-state arrays after manager_starts
    of every T step with the arrays before it)"""
    import torch
    snaps, started = [], []
    for step in cases.steps_of(sc, n):
        if step[0] == "Q":
            _, starts, goals, mask = step
            pl.manager_request(None if starts is None else starts[:n], None if goals is None else goals[:n], mask[:n])
            continue
        if step[0] == "L":
            task = sc["task"]
            pl.manager_next_legs(n, dev(step[2][:n], torch.float64), dev(task["leg_yaw"][:n], torch.float64), reset_legs=step[1])
        else:
            t = step[1]
            if host_begin:
                pl.manager_begin(t["now"], t["poses"][:n], t["collision"][:n])
            else:
                pl.manager_begin(t["now"], dev(t["poses"][:n], torch.float64), dev(t["collision"][:n], torch.int32), stride=24, count=n)
            x, v, o = (dev(t[k][:n], torch.float64) for k in ("xytheta", "vaj", "oaj"))
            sy, ey = torch.full((n,), -7.0, dtype=torch.float64, device="cuda"), torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
            pl.manager_starts(n, x, v, o, sy, ey)
            started.append(tuple(a.cpu().numpy() for a in (x, v, o, sy, ey)))
            pl.manager_end(n, dev(t["search"][:n], torch.int32), dev(t["build"][:n], torch.int32), dev(t["ok"][:n], torch.int32),
                           dev(t["T"][:n], torch.float64), dev(t["n_pieces"][:n], torch.int32))
        snaps.append(snapshot(pl, n))
    return snaps, started


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


_runs = {}


def full_run(seed):
    """the B = 70 run of a seed, once for the tests that need it"""
    if seed not in _runs:
        sc = cases.scenario(seed)
        pl = make_planner(sc["B"], sc["params"])
        dist = pl.map_state()["dist"]
        assert np.array_equal(np.sign(dist), np.sign(cases.stand_in_dist()))         # negative exactly in the inner 3 x 3 cells of the block
        _runs[seed] = (sc, dist) + run_device(pl, sc, sc["B"], host_begin=seed == 2)
    return _runs[seed]


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_every_tick_equals_the_oracle(seed):
    sc, dist, snaps, started = full_run(seed)
    fleet, exp, exp_started = cases.run_oracle(sc, dist=dist)
    assert len(snaps) == len(exp) == 12
    for k, (g, e) in enumerate(zip(snaps, exp)):
        same(g, e, (seed, "tick", k))
    assert dict(zip(cases.COUNTERS[:6], snaps[-1][2])) == {k: fleet.counters[k] for k in cases.COUNTERS[:6]}
    # manager_starts: rows of NONE robots bit for bit, FRESH rows the start state and zeros, REPLAN robots' plan_start_xytheta the
    # predicted pose; start_yaw / end_yaw of every robot
    seen = set()
    for k, (t, got, want) in enumerate(zip(sc["ticks"], started, exp_started)):
        action = snaps[k][0][4]
        for name, g, w in zip(("xytheta", "vaj", "oaj", "start_yaw", "end_yaw"), got, want):
            assert np.array_equal(bits(g), bits(w)), (seed, k, name)
        none, fresh, replan = action == cases.NONE, action == cases.FRESH, action == cases.REPLAN_ACTION
        for name, g in zip(("xytheta", "vaj", "oaj"), got):
            assert np.array_equal(bits(g[none]), bits(t[name][none])), (seed, k, name)
        assert np.array_equal(bits(got[0][fresh]), bits(snaps[k][1][3:6].T[fresh])) and not got[1][fresh].any() and not got[2][fresh].any()
        assert np.array_equal(bits(snaps[k][1][6:9].T[replan]), bits(t["xytheta"][replan]))
        seen |= set(action.tolist())
    assert seen == {cases.NONE, cases.FRESH, cases.REPLAN_ACTION}


@pytest.mark.parametrize("n", [1, 64])
def test_no_dependence_on_the_fleet_size(n):
    """robots 0..n-1 alone, on a handle of n robots, do what they do among 70"""
    seed = 1
    sc, dist, snaps70, _ = full_run(seed)
    snaps, _ = run_device(make_planner(n, sc["params"]), sc, n)
    _, exp, _ = cases.run_oracle(sc, count=n, dist=dist)
    for k, (g, g70, e) in enumerate(zip(snaps, snaps70, exp)):
        assert np.array_equal(g[0], g70[0][:, :n]) and np.array_equal(bits(g[1]), bits(g70[1][:, :n])), (n, k)
        same(g, e, (n, "tick", k))


def test_bad_calls_change_nothing():
    from alore_legged_manipulator_amd.backend import BackendError
    sc = cases.scenario(0, B=6, K=2)
    bare = make_planner(6, manager=False)
    poses = sc["ticks"][0]["poses"]
    for call in (lambda: bare.manager_begin(100.0, poses), lambda: bare.manager_end(6), lambda: bare.get_manager(6),
                 lambda: bare.manager_request(poses, poses)):
        with pytest.raises(BackendError, match="error -1.*manager_create"):
            call()
    pl = make_planner(6, sc["params"])
    run_device(pl, sc, 6)
    before = snapshot(pl, 6)
    with pytest.raises(BackendError, match="error -1.*manager_begin"):
        pl.manager_end(6)                                                           # the end of tick 1 has used its begin
    with pytest.raises(BackendError, match="error -1"):
        pl.manager_begin(101.0, np.zeros((7, 3)))                                   # count > max_problems
    with pytest.raises(BackendError, match="error -1"):
        pl.manager_end(7)
    with pytest.raises(BackendError, match="error -1"):
        pl.manager_request(np.zeros((7, 3)), None)
    with pytest.raises(BackendError, match="error -1"):
        pl.manager_begin(float("nan"), poses)
    with pytest.raises(BackendError, match="error -1.*manager_begin"):
        pl.manager_end(6)                                                           # the refused begins were no begin
    same(snapshot(pl, 6), before, "after the bad calls")


def test_next_legs_walk_the_missions_of_the_task_slab():
    """6 missions of 1 .. 3 tasks, one failed, one robot busy: every free robot takes its legs one after the other, bit for bit the
    goals of the task slab, and nothing else moves"""
    B, T, rng = len(cases.LEG_TASKS), max(cases.LEG_TASKS), np.random.default_rng(5)
    pl = make_planner(B, cases.SEED_PARAMS[0])
    pts = np.zeros((B, 1 + 2 * T, 2))
    cells = rng.permutation(8 * 16)[:B * (1 + 2 * T)].reshape(B, 1 + 2 * T)           # distinct free cells with x < 0
    pts[..., 0], pts[..., 1] = cases.X_LO + (cells // 16 + 0.5) * cases.RES, cases.Y_LO + (cells % 16 + 0.5) * cases.RES
    pts[3, 1] = (100.0, 0.0)                                                          # outside the map: the mission fails
    pl.task_plan(cases.LEG_TASKS, pts, check=False)
    task = pl.task_result(B)
    assert task["status"].tolist() == [0, 0, 0, -1, 0, 0] and task["n_order"].tolist() == [2, 6, 4, 0, 6, 2]
    sc = cases.legs_scenario(dict(status=task["status"], n_order=task["n_order"], leg_goal_xy=task["leg_goal_xy"]))
    snaps, _ = run_device(pl, sc, B)
    fleet, exp, _ = cases.run_oracle(sc)
    assert len(snaps) == len(exp)
    for k, (g, e) in enumerate(zip(snaps, exp)):
        same(g, e, ("legs", k))
    assert snaps[-2][0][3].tolist() == [2, 6, 4, 0, 6, 0] and snaps[-1][0][3].tolist() == [1, 1, 1, 0, 1, 0]
    first = snaps[0]                                                                  # after the first next_legs
    assert np.array_equal(bits(first[1][0:2].T[[0, 1, 2, 4]]), bits(task["leg_goal_xy"][[0, 1, 2, 4], 0]))
    assert first[0][1].tolist() == [1, 1, 1, 0, 1, 1] and first[0][2].tolist() == [1, 1, 1, 0, 1, 1]
