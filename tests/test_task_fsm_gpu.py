"""The whole task FSM on the device (csrc/task_fsm.hip through include/alore_fsm.h and task_fsm.py) against the oracle of
tests/task_fsm_cases.py, on the recorded mission scene the CPU test replays to the header.

B = 70 robots: one full wavefront and one of 6 lanes.  Lane b is mission robot b % 5 started b % 14 ticks late (it is reset by mask on
that tick), so the lanes of a wavefront sit in different states on every tick.  EQUAL after every tick: every integer (state,
task_num, indices, dwell, finished, request_mask, object_type, the grasp integers) and robot_vel_cmd, object_vel_cmd's zeros
included.  WITHIN DEVICE_VS_ORACLE: the other doubles.

THE TOLERANCE is measured, not chosen: HEADER_VS_ORACLE is the largest absolute difference between the g++ build of the header and
the oracle over every tick of every scene (tests/test_task_fsm_cpu.py prints it and asserts it), and the device gets ten times that
with a floor of 1e-12 -- the margin of tests/test_arm_ik_gpu.py, for the device's atan2 / sincos / hypot differing from glibc's by an
ulp (the commands are 2 e with |e| < pi and the IK is the one measured there)."""
import functools
import os
import sys

import numpy as np
import pytest

from tests import arm_ik_cases as arm_cases
from tests import task_fsm_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# measured by tests/test_task_fsm_cpu.py (it prints each figure and asserts this bound): default 4.441e-16, mission 3.331e-16,
# tracking 2.776e-16; the largest, rounded up
HEADER_VS_ORACLE = 4.5e-16
DEVICE_VS_ORACLE = max(10.0 * HEADER_VS_ORACLE, 1e-12)      # = 1e-12: the floor decides
# the device's own largest difference from the oracle on an MI355X (printed by test_every_tick_equals_the_oracle;
# profiles/task_fsm.txt): 3.553e-15 over 70 lanes x 1500 ticks

gpu = pytest.mark.gpu

B, ROBOTS, SPREAD = 70, 5, 14
MAX_PATH_POINTS = 24
INTS = cases.INT_NAMES
GRASP_INTS = ("grasp_time", "flag", "stable", "done", "ik_iterations", "ik_status")
GRASP_DBLS = ("k", "d_gripper", "gripper_ang", "err_norm")


def make(n, ticks=None, max_tasks=cases.MISSION_MAX_TASKS, max_objects=cases.MISSION_OBJECTS, classes=None, fsm=True):
    from alore_legged_manipulator_amd import arm, task_fsm
    h = arm.BatchedArm(n, **cases.IK)
    h.set_classes([arm.PRESETS[k] for k in arm.PRESET_NAMES])
    if classes is not None:
        h.set_robot_classes(np.asarray(classes, np.int32))
    if not fsm:
        return h, None
    f = task_fsm.BatchedTaskFsm(h, max_tasks, max_objects, MAX_PATH_POINTS, **(ticks if ticks is not None else cases.MISSION_TICKS))
    f.set_class_offsets([task_fsm.PRESET_COM_OFFSETS[k] for k in arm.PRESET_NAMES])
    return h, f


@functools.lru_cache(maxsize=None)
def oracle_arrays():
    """the mission scene's inputs and snapshots stacked: [T][R][...]"""
    sc = cases.mission_scene()
    ins = [np.array([[np.asarray(inp[i], float) for inp in row] for row in sc["inputs"]]) for i in range(4)]
    snaps = [np.array([[s[i] for s in row] for row in sc["snaps"]]) for i in range(7)]
    return ins, snaps


@functools.lru_cache(maxsize=None)
def schedule():
    """the mission scene tiled over the lanes: per global tick the inputs [B], the masks and rows of the events, the lanes to reset
    and `local`, the tick of its record each lane is at (-1 outside the record)"""
    sc = cases.mission_scene()
    ins, _ = oracle_arrays()
    T = len(sc["inputs"])
    mt = sc["max_tasks"]
    lane, robot, delay = np.arange(B), np.arange(B) % ROBOTS, np.arange(B) % SPREAD
    out = []
    for G in range(T + SPREAD - 1):
        t = G - delay
        at = np.clip(t, 0, T - 1)
        order, n_order, seq_mask = np.zeros((B, 2 * mt), np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
        xy, n_points, path_mask = np.zeros((B, MAX_PATH_POINTS, 2)), np.zeros(B, np.int32), np.zeros(B, np.int32)
        for b in lane[(t >= 0) & (t < T)]:
            for kind, data in sc["events"][t[b]][robot[b]]:
                if kind == "S":
                    order[b, :len(data)], n_order[b], seq_mask[b] = data, len(data), 1
                else:
                    xy[b, :len(data)], n_points[b], path_mask[b] = data, len(data), 1
        out.append(dict(pose=ins[0][at, robot], objs=ins[1][at, robot], base=ins[2][at, robot], jp=ins[3][at, robot], order=order, n_order=n_order,
                        seq_mask=seq_mask, xy=xy, n_points=n_points, path_mask=path_mask, reset=(t == 0).astype(np.int32),
                        local=np.where((t >= 0) & (t < T), t, -1)))
    return out


def lanes_of(robot):
    return [b for b in range(B) if b % ROBOTS == robot]


def snapshot(f, h, n):
    s = f.get(n)
    s.pop("counters")
    s.update(h.get_grasp(n))
    return s


GRASP_WINDOW = range(340, 440)          # global ticks on which the grasp step is repeated on a second handle: robots 2 and 3 run the IK, 0, 1 and 4 wait or approach


@pytest.fixture(scope="module")
def host_run():
    """the whole schedule through HOST pointers, a wait after every call; the state after every tick.  On the ticks of GRASP_WINDOW
    the grasp state is copied to a second arm handle first and alore_arm_grasp_step runs there on the same rows"""
    import torch
    sched = schedule()
    classes = [arm_cases.CLASS_NAMES.index(cases.MISSION_CLASSES[b % ROBOTS]) for b in range(B)]
    h, f = make(B, classes=classes)
    h2, _ = make(B, classes=classes, fsm=False)
    f.set_targets(np.array([cases.mission_scene()["robots"][b % ROBOTS]["targets"] for b in range(B)]))
    view, gv, gv2 = f.view(), h.grasp_view(), h2.grasp_view()
    snaps, grasp_checked, grasp_bad = [], 0, []
    for G, s in enumerate(sched):
        if s["reset"].any():
            f.reset(B, s["reset"])
            lanes = [b for b in lanes_of(2) if s["reset"][b]]
            if lanes:
                view["stop_after_back_off"][torch.tensor(lanes, device="cuda")] = 1      # the robot's own word
        if s["seq_mask"].any():
            f.set_sequences(s["order"], s["n_order"], s["seq_mask"])
        if s["path_mask"].any():
            f.set_paths(s["xy"], s["n_points"], s["path_mask"])
        second = G in GRASP_WINDOW
        if second:
            before = f.get(B)
            for k in gv:
                gv2[k].copy_(gv[k])
        f.tick(s["pose"], s["objs"], s["base"], s["jp"])
        snaps.append(snapshot(f, h, B))
        if second:
            h2.grasp_step(s["pose"][:, 0:2], snaps[-1]["object_pose_used"], s["base"], s["jp"])
            g2 = h2.get_grasp(B)
            stepped = np.nonzero((before["task_state"] == 3) & (before["dwell"] == 0))[0]
            grasp_checked += len(stepped)
            grasp_bad += [(G, int(b), k) for k in g2 for b in stepped if g2[k][b].tobytes() != snaps[-1][k][b].tobytes()]
    counters = f.get(B)["counters"]
    f.close(); h.close(); h2.close()
    return dict(snaps=snaps, grasp_checked=grasp_checked, grasp_bad=grasp_bad, counters=counters)


@gpu
def test_every_tick_equals_the_oracle(host_run):
    sched = schedule()
    _, (e_ints, e_gi, e_dbl, e_gd, e_cmd, e_vel, e_ctl) = oracle_arrays()
    robot = np.arange(B) % ROBOTS
    worst, compared = 0.0, 0
    for G, (s, got) in enumerate(zip(sched, host_run["snaps"])):
        on = s["local"] >= 0
        t, r = s["local"][on], robot[on]
        gints, ints = np.stack([got[k] for k in INTS], axis=1)[on], e_ints[t, r]
        assert np.array_equal(gints, ints), (G, np.argwhere(gints != ints)[:5], INTS)
        ggi = np.stack([got[k] for k in GRASP_INTS], axis=1)[on]
        assert np.array_equal(ggi, e_gi[t, r]), (G, np.argwhere(ggi != e_gi[t, r])[:5])
        assert np.array_equal(got["robot_vel_cmd"][on] == 0.0, e_vel[t, r] == 0.0), G
        assert np.array_equal(got["object_vel_cmd"][on] == 0.0, e_dbl[t, r][:, 1:4] == 0.0), G
        assert np.array_equal(got["control"][on][:, 13:15], ints[:, [0, 3]].astype(float)), G
        gdbl = np.column_stack([got["reach_threshold"], got["object_vel_cmd"], got["start_xytheta"], got["goal_xytheta"], got["object_pose_used"]])[on]
        worst = max(worst, np.abs(gdbl - e_dbl[t, r]).max(), np.abs(np.stack([got[k] for k in GRASP_DBLS], axis=1)[on] - e_gd[t, r]).max(),
                    np.abs(got["joint_cmd"][on] - e_cmd[t, r]).max(), np.abs(got["robot_vel_cmd"][on] - e_vel[t, r]).max(),
                    np.abs(got["control"][on] - e_ctl[t, r]).max())
        compared += int(on.sum())
    print("device vs oracle, mission scene on %d lanes, %d robot ticks: %.3e" % (B, compared, worst))
    assert compared == B * cases.MISSION_LENGTH
    assert worst <= DEVICE_VS_ORACLE, worst
    assert host_run["counters"] == dict(refused_sequences=0, refused_paths=0)
    states = np.array([s["task_state"] for s in host_run["snaps"]])
    assert max(len(set(row[:64].tolist())) for row in states) >= 4     # the lanes of the full wavefront sit in different states


@gpu
def test_grasping_robots_get_the_bits_of_the_arms_grasp_step(host_run):
    """a second arm handle, given the grasp state before the tick and the same rows (the object pose the FSM used), leaves for every robot
    that ran the grasp step the bits the FSM's tick left"""
    assert host_run["grasp_checked"] > 500, host_run["grasp_checked"]
    assert host_run["grasp_bad"] == [], host_run["grasp_bad"][:5]
    ran_ik = sum(int((s["ik_status"] != 3).sum()) for G, s in enumerate(host_run["snaps"]) if G in GRASP_WINDOW)
    assert ran_ik > 200                                        # and the window has ticks with the IK inside


@gpu
def test_device_pointers_without_a_wait_leave_the_same_bits(host_run):
    """the same schedule with every array on the device, on a side stream, no wait between the calls (the state after every tick is
    copied aside on the same stream): bit for bit what the host-pointer ticks with a wait after each left"""
    import torch
    sched = schedule()
    classes = [arm_cases.CLASS_NAMES.index(cases.MISSION_CLASSES[b % ROBOTS]) for b in range(B)]
    h, f = make(B, classes=classes)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda")
    f.set_targets(dev(np.array([cases.mission_scene()["robots"][b % ROBOTS]["targets"] for b in range(B)])))
    view = dict(f.view(), **h.grasp_view())
    for k in ("robot_path", "object_path", "target_poses", "counters", "object_sequence", "target_sequence"):
        view.pop(k)
    T = len(sched)
    first = SPREAD                                             # the resets by mask are host calls: the ticks behind them run without a wait
    for s in sched[:first]:
        if s["reset"].any():
            f.reset(B, s["reset"])
            for b in lanes_of(2):
                if s["reset"][b]:
                    view["stop_after_back_off"][b] = 1
        if s["seq_mask"].any():
            f.set_sequences(s["order"], s["n_order"], s["seq_mask"])
        if s["path_mask"].any():
            f.set_paths(s["xy"], s["n_points"], s["path_mask"])
        f.tick(s["pose"], s["objs"], s["base"], s["jp"])
    inputs = {k: dev(np.array([s[k] for s in sched[first:]])) for k in ("pose", "objs", "base", "jp", "order", "n_order", "seq_mask", "xy", "n_points",
                                                                         "path_mask")}
    hist = {k: torch.zeros((T - first,) + tuple(v.shape), dtype=v.dtype, device="cuda") for k, v in view.items()}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for i, s in enumerate(sched[first:]):
            if s["seq_mask"].any():
                f.set_sequences(inputs["order"][i], inputs["n_order"][i], inputs["seq_mask"][i], stream=stream)
            if s["path_mask"].any():
                f.set_paths(inputs["xy"][i], inputs["n_points"][i], inputs["path_mask"][i], stream=stream)
            f.tick(inputs["pose"][i], inputs["objs"][i], inputs["base"][i], inputs["jp"][i], stream=stream)
            for k, v in view.items():
                hist[k][i].copy_(v, non_blocking=True)
    stream.synchronize()
    for k in hist:
        got, exp = hist[k].cpu().numpy(), np.stack([s[k] for s in host_run["snaps"][first:]])
        assert got.tobytes() == exp.tobytes(), k
    f.close(); h.close()


# ---- the callbacks ---------------------------------------------------------------------------------------------------------------------
def put(view, name, values):
    import torch
    view[name][:len(values)] = torch.tensor(values, dtype=view[name].dtype, device="cuda")


def everything(f, h, n):
    s = f.get(n)
    s.pop("counters")
    s.update(h.get_grasp(n))
    return s


@gpu
@pytest.mark.parametrize("pointers", ["host", "device"])
def test_set_paths_honours_masks_states_and_sizes(pointers):
    import torch
    n = 8
    h, f = make(n)
    view = f.view()
    #             0 robot  1 object  2 tracking  3 robot, masked out  4 robot, no points  5 object, too many  6 planning  7 robot, dwelling
    put(view, "task_state", [1, 4, 2, 1, 1, 4, 0, 1])
    put(view, "dwell", [0, 0, 0, 0, 0, 0, 3, 5])
    put(view, "robot_path_index", [7] * n)
    put(view, "object_path_index", [7] * n)
    torch.cuda.synchronize()
    before = everything(f, h, n)
    rng = np.random.default_rng(2)
    xy = rng.uniform(-3, 3, (n, MAX_PATH_POINTS + 2, 2))
    n_points = np.array([8, 5, 8, 8, 0, MAX_PATH_POINTS + 1, 8, MAX_PATH_POINTS], np.int32)
    mask = np.array([1, 1, 1, 0, 1, 1, 1, 1], np.int32)
    if pointers == "host":
        f.set_paths(xy, n_points, mask)
    else:
        f.set_paths(torch.tensor(xy, device="cuda"), torch.tensor(n_points, device="cuda"), torch.tensor(mask, device="cuda"))
    after = everything(f, h, n)
    assert after["task_state"].tolist() == [2, 5, 2, 1, 1, 4, 0, 2]
    assert after["robot_path_index"].tolist() == [0, 7, 7, 7, 7, 7, 7, 0] and after["object_path_index"].tolist() == [7, 0, 7, 7, 7, 7, 7, 7]
    assert after["n_robot_path"].tolist() == [8, 0, 0, 0, 0, 0, 0, MAX_PATH_POINTS] and after["n_object_path"].tolist() == [0, 5, 0, 0, 0, 0, 0, 0]
    assert after["robot_path"][0, :8].tobytes() == xy[0, :8].tobytes() and after["object_path"][1, :5].tobytes() == xy[1, :5].tobytes()
    assert after["robot_path"][7].tobytes() == xy[7, :MAX_PATH_POINTS].tobytes()
    assert after["dwell"].tolist() == before["dwell"].tolist()                       # a delivery leaves the countdown alone
    for b in (2, 3, 4, 5, 6):                                                        # untouched, bit for bit
        for k in before:
            assert after[k][b].tobytes() == before[k][b].tobytes(), (b, k)
    assert f.get(n)["counters"] == dict(refused_sequences=0, refused_paths=1)
    # the dwelling robot: the state has changed, the countdown goes on, and it tracks only when it is over
    z = np.zeros((n, 4)), np.zeros((n, cases.MISSION_OBJECTS, 4)), np.tile([0, 0, 0, 0, 0, 0, 1.0], (n, 1)), np.tile(arm_cases.Q0, (n, 1))
    f.tick(*z)
    s = f.get(n)
    assert s["task_state"][7] == 2 and s["dwell"][7] == 4 and s["robot_path_index"][7] == 0 and s["control"][7, 13] == 2.0
    f.close(); h.close()


@gpu
def test_set_sequences_refuses_bad_rows():
    n = 8
    h, f = make(n)
    before = everything(f, h, n)
    order = np.array([[2, 1, 0, 0], [0, 0, 0, 0], [0, 0, 1, 1], [3, 0, 0, 0], [0, 2, 0, 0], [-1, 0, 0, 0], [1, 1, 0, 0], [1, 0, 2, 1]], np.int32)
    n_order = np.array([4, 0, 3, 2, 2, 2, 6, 4], np.int32)          # ok, < 2, odd, item out of range, target out of range, negative, > 2 max_tasks, masked
    f.set_sequences(order, n_order, [1, 1, 1, 1, 1, 1, 1, 0])
    after = everything(f, h, n)
    assert after["is_task_plan"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and after["n_tasks"][0] == 2
    assert after["object_sequence"][0, :2].tolist() == [2, 0] and after["target_sequence"][0, :2].tolist() == [1, 0]
    for b in range(1, n):
        for k in before:
            assert after[k][b].tobytes() == before[k][b].tobytes(), (b, k)
    assert f.get(n)["counters"] == dict(refused_sequences=6, refused_paths=0)
    f.close(); h.close()


@gpu
def test_refusals_come_before_anything_is_enqueued():
    from alore_legged_manipulator_amd import arm, task_fsm
    n = 4
    h, f = make(n)
    before = everything(f, h, n)
    with pytest.raises(arm.ArmError):
        task_fsm.BatchedTaskFsm(h)                                                   # a second FSM on the handle
    with pytest.raises(arm.ArmError):
        f.tick(np.zeros((9, 4)), np.zeros((9, cases.MISSION_OBJECTS, 4)), np.zeros((9, 7)), np.zeros((9, 7)))      # count > max_problems
    with pytest.raises(arm.ArmError):
        f.tick(np.zeros((n, 4)), np.zeros((n, 2, 4)), np.zeros((n, 7)), np.zeros((n, 7)))                          # object rows too short
    with pytest.raises(arm.ArmError):
        f.set_class_offsets([[np.nan, 0.0]])
    with pytest.raises(arm.ArmError):
        f.set_paths(np.zeros((n, 4, 2)), np.array([5, 0, 0, 0], np.int32))           # a row longer than its stride
    bare = arm.BatchedArm(2)
    assert bare.L.alore_fsm_reset(bare.h, 1, None) == -1 and b"no FSM" in bare.L.alore_arm_last_error(bare.h)      # a handle without an FSM
    for bad in (dict(max_tasks=0), dict(max_tasks=11), dict(max_objects=0), dict(max_path_points=0), dict(ticks_release=0)):
        with pytest.raises(arm.ArmError):
            task_fsm.BatchedTaskFsm(bare, **bad)
    after = everything(f, h, n)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k
    f.close(); h.close(); bare.close()


@gpu
def test_a_release_from_the_top_of_the_grasp():
    """a robot put into RELEASING with k = 0.25 and d_gripper = 0.01 (the reference's grasp leaves k = 0, so no mission gets there):
    40 calls of object_release, additions alone, bit for bit the oracle's; then the last task is over and the robot stands"""
    import torch
    n = 3
    h, f = make(n, classes=[1, 1, 1])
    view, gv = f.view(), h.grasp_view()
    put(view, "task_state", [6, 0, 6])
    gv["k"][0], gv["d_gripper"][0] = 0.25, 0.01
    m = cases.TaskFsm(arm_cases.class_row("table"), cases.COM_OFFSETS["table"], cases.MISSION_TICKS, n_objects=cases.MISSION_OBJECTS)
    m.task_state, m.g.k, m.g.d_gripper = "RELEASING", 0.25, 0.01
    z = np.zeros((n, 4)), np.zeros((n, cases.MISSION_OBJECTS, 4)), np.tile([0, 0, 0, 0, 0, 0, 1.0], (n, 1)), np.tile(arm_cases.Q0, (n, 1))
    for call in range(45):
        f.tick(*z)
        m.tick(z[0][0], z[1][0], z[2][0], z[3][0])
        s, g = f.get(n), h.get_grasp(n)
        assert g["k"][0] == m.g.k and g["d_gripper"][0] == m.g.d_gripper and g["joint_cmd"][0].tobytes() == m.g.joint_cmd.tobytes(), call
        assert (s["finished"][0], s["dwell"][0], s["task_num"][0], s["task_state"][0]) == (m.finished, m.dwell, m.task_num, 6), call
        assert g["robot_vel_cmd"][0].tobytes() == m.g.robot_vel_cmd.tobytes()
    assert m.finished == 1 and "release from k = 0.25" in m.branches and s["finished"].tolist() == [1, 0, 0]
    f.close(); h.close()


# ---- the chain with the back_end -------------------------------------------------------------------------------------------------------
@gpu
def test_the_order_slab_of_task_plan_is_read_as_it_lies():
    """3 missions on a small empty map: alore_backend_task_plan's `order` and `n_order` slabs go into set_sequences with stride 80, on
    the device; mission 2 has 3 tasks, more than the FSM's max_tasks of 2: its row is refused"""
    import torch
    from tests import fleet_manager_cases as fleet
    from tests.test_fleet_manager_gpu import make_planner
    n_tasks = [2, 1, 3]
    n, T = 3, 3
    pl = make_planner(n, manager=False)
    rng = np.random.default_rng(5)
    pts = np.zeros((n, 1 + 2 * T, 2))
    cells = rng.permutation(8 * 16)[:n * (1 + 2 * T)].reshape(n, 1 + 2 * T)             # distinct free cells with x < 0
    pts[..., 0], pts[..., 1] = fleet.X_LO + (cells // 16 + 0.5) * fleet.RES, fleet.Y_LO + (cells % 16 + 0.5) * fleet.RES
    pl.task_plan(n_tasks, pts, check=False)
    task = pl.task_result(n)
    assert task["status"].tolist() == [0, 0, 0] and task["n_order"].tolist() == [4, 2, 6]
    h, f = make(n, max_objects=3)
    v = pl.device_task()
    assert v.max_legs * 4 == 80
    f.set_sequences(v.order, v.n_order, order_stride=80, count=n)
    torch.cuda.synchronize()
    s = f.get(n)
    assert s["is_task_plan"].tolist() == [1, 1, 0] and s["n_tasks"].tolist() == [2, 1, 1] and s["counters"]["refused_sequences"] == 1
    for b in (0, 1):
        k = n_tasks[b]
        assert s["object_sequence"][b, :k].tolist() == task["order"][b, 0:2 * k:2].tolist()
        assert s["target_sequence"][b, :k].tolist() == task["order"][b, 1:2 * k:2].tolist()
    assert s["object_sequence"][2].tolist() == [0, 1, 2, 2, 2, 2, 2, 2, 2, 2]      # untouched: the identity of a reset, clamped into 3 objects
    f.close(); h.close()


@gpu
def test_path_points_device_feeds_set_paths():
    """3 plans, the second one rejected by the optimiser (its goal is inside an obstacle): path_points_device writes the bits of
    path_points on zeroed slabs; fed to set_paths, the robots of the good plans track and the rejected slot's robot keeps waiting"""
    import torch
    from alore_legged_manipulator_amd.flat_traj import straight_goal
    from tests.test_backend_gpu import circle_grid, planner_for
    fts = [straight_goal((0, 0, 0), (2.0, -1.0, 0.3)), straight_goal((0, 0, 0), (3.0, 1.3, 0.0)), straight_goal((0, 0, 0), (-2.0, 0.5, 2.8))]
    pl = planner_for(circle_grid(3.0, 1.3, 0.9), 3)
    res = pl.minco_plan(fts)
    assert res["ok"].tolist() == [1, 0, 1]
    panels = 3
    host = pl.path_points(panels)
    per = pl.P * (panels + 1)
    xy = torch.zeros((3, per, 2), dtype=torch.float64, device="cuda")
    yaw = torch.zeros((3, pl.P * panels), dtype=torch.float64, device="cuda")
    npts = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    pl.path_points_device(xy, npts, yaw, panels)
    torch.cuda.synchronize()
    got_n = npts.cpu().numpy()
    assert got_n.tolist() == [len(host[0][0]), 0, len(host[2][0])] and got_n[0] > 0
    for b in (0, 2):
        assert xy[b, :got_n[b]].cpu().numpy().tobytes() == host[b][0].tobytes()
        assert yaw[b, :len(host[b][1])].cpu().numpy().tobytes() == host[b][1].tobytes()
    assert (xy[1] == 0).all() and (xy[0, got_n[0]:] == 0).all()
    from alore_legged_manipulator_amd import arm, task_fsm
    h = arm.BatchedArm(3)
    f = task_fsm.BatchedTaskFsm(h, 2, 2, per)
    view = f.view()
    put(view, "task_state", [1, 1, 4])
    f.set_paths(xy, npts)
    torch.cuda.synchronize()
    s = f.get(3)
    assert s["task_state"].tolist() == [2, 1, 5] and s["n_robot_path"].tolist() == [int(got_n[0]), 0, 0] and s["n_object_path"][2] == got_n[2]
    assert s["robot_path"][0, :got_n[0]].tobytes() == host[0][0].tobytes() and s["object_path"][2, :got_n[2]].tobytes() == host[2][0].tobytes()
    assert s["counters"]["refused_paths"] == 0
    f.close(); h.close()


@gpu
def test_request_rows_go_into_the_manager_as_they_lie():
    """robots in WAIT_ROBOT_PATH and WAIT_OBJECT_PATH raise their flags; request_mask, start_xytheta and goal_xytheta go into
    alore_backend_manager_request on the device: nothing is refused and the manager holds the FSM's rows bit for bit; the goal of a
    WAIT_ROBOT_PATH robot is what alore_arm_grasp_poses(PLAN) writes for its object"""
    import torch
    from alore_legged_manipulator_amd import arm
    from tests import fleet_manager_cases as fleet
    from tests.test_fleet_manager_gpu import make_planner
    n = 6
    classes = [0, 1, 2, 0, 1, 2]
    h, f = make(n, classes=classes, ticks=dict(cases.MISSION_TICKS, ticks_no_plan=1))
    rng = np.random.default_rng(7)
    targets = np.zeros((n, 2, 4))
    targets[..., 0], targets[..., 1], targets[..., 3] = rng.uniform(-3, -1, (n, 2)), rng.uniform(-3, 3, (n, 2)), rng.uniform(-3, 3, (n, 2))
    f.set_targets(targets)
    f.set_sequences(np.tile(np.array([2, 1, 0, 0], np.int32), (n, 1)), np.full(n, 4, np.int32))
    view = f.view()
    put(view, "task_state", [1, 1, 1, 4, 4, 2])                   # three ask for a robot path, two for an object path, one tracks
    put(view, "object_type", [0, 0, 0, 1, 2, 0])
    put(view, "target_type", [0, 0, 0, 1, 0, 0])
    put(view, "n_robot_path", [0, 0, 0, 0, 0, 1])
    pose = np.column_stack([rng.uniform(-3, -1, n), rng.uniform(-3, 3, n), np.zeros(n), rng.uniform(-3, 3, n)])
    objs = np.zeros((n, cases.MISSION_OBJECTS, 4))
    objs[..., 0], objs[..., 1], objs[..., 3] = rng.uniform(-3, -1, (n, 3)), rng.uniform(-3, 3, (n, 3)), rng.uniform(-3, 3, (n, 3))
    f.tick(pose, objs, np.tile([0, 0, 0, 0, 0, 0, 1.0], (n, 1)), np.tile(arm_cases.Q0, (n, 1)))
    s = f.get(n)
    assert s["request_mask"].tolist() == [1, 1, 1, 1, 1, 0] and s["object_type"].tolist() == [2, 2, 2, 1, 2, 0]
    assert s["start_xytheta"][:3].tobytes() == pose[:3][:, [0, 1, 3]].tobytes()
    assert s["start_xytheta"][3:5].tobytes() == s["object_pose_used"][3:5][:, [0, 1, 3]].tobytes()
    assert s["goal_xytheta"][3].tobytes() == targets[3, 1, [0, 1, 3]].tobytes() and s["goal_xytheta"][4].tobytes() == targets[4, 0, [0, 1, 3]].tobytes()
    _, goal = h.grasp_poses(s["object_pose_used"], arm.POSE_PLAN)
    assert goal[:3].tobytes() == s["goal_xytheta"][:3].tobytes()
    exp_used = np.array([cases.com(objs[b, s["object_type"][b]], cases.COM_OFFSETS[arm_cases.CLASS_NAMES[classes[b]]]) for b in range(n)])
    assert np.abs(s["object_pose_used"] - exp_used).max() <= DEVICE_VS_ORACLE
    pl = make_planner(n, fleet.SEED_PARAMS[0])
    pl.manager_request(view["start_xytheta"], view["goal_xytheta"], view["request_mask"], stride=24, count=n)
    torch.cuda.synchronize()
    m = pl.get_manager(n)
    assert m["counters"]["refused"] == 0
    assert m["start"][:5].tobytes() == s["start_xytheta"][:5].tobytes() and m["goal"][:5].tobytes() == s["goal_xytheta"][:5].tobytes()
    assert not m["start"][5].any() and not m["goal"][5].any()       # the robot that did not ask
    f.close(); h.close()
