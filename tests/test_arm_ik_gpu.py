"""The batched Z1 grasp IK and the grasp step on the device (csrc/arm_ik.hip through include/alore_arm.h and arm.py) against the
oracle of tests/arm_ik_cases.py, on the scenes the CPU test runs the header on.

EQUAL: iterations, status, every integer of the grasp state, done, robot_vel_cmd and the at_target bits (the oracle's input guard
keeps every compared norm 1e-9 away from its threshold).  WITHIN DEVICE_TOL: q, err_norm, poses, joint_cmd.

THE TOLERANCE is not chosen, it is measured: HEADER_VS_ORACLE is the largest absolute difference between the g++ build of the
header and the NumPy oracle over all scenes, pieces and grasp sequences (two independent float64 evaluations of one contract:
BLAS-ordered sums there, index-ordered sums here), and the device gets ten times that with a floor of 1e-12, because the device's
sin / cos / atan2 differ from glibc's by a few ulp and the chain is well conditioned on these scenes (cond(J) <= 20)."""
import math
import os
import sys

import numpy as np
import pytest

from tests import arm_ik_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# measured by tests/test_arm_ik_cpu.py (it prints each figure and asserts this bound): the largest is 2.576e-14 (the grasp sequences,
# 900 ticks; the IK scenes 2.220e-15 at most, `far`; the pieces 2.220e-16), rounded up
HEADER_VS_ORACLE = 2.6e-14
DEVICE_TOL = max(10.0 * HEADER_VS_ORACLE, 1e-12)      # = 1e-12: the floor decides
# the device's own largest difference from the oracle on an MI355X (printed by these tests; profiles/arm_ik.txt): 3.109e-14 on the grasp
# sequences, 2.998e-15 on the IK scenes (`far`), 4.441e-16 on fk, the Jacobian and grasp_poses

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def arm():
    from alore_legged_manipulator_amd import arm as module
    return module


@pytest.fixture(scope="module")
def handles(arm):
    made = {}

    def get(**params):
        key = tuple(sorted(params.items()))
        if key not in made:
            made[key] = arm.BatchedArm(128, **params)
        return made[key]
    yield get
    for h in made.values():
        h.close()


def scene(name):
    return cases.nan_scene() if name == "nan" else cases.scenes()[name]


def compare(got, exp, n, label):
    assert np.array_equal(got["iterations"][:n], exp["iterations"][:n]), (label, got["iterations"][:n], exp["iterations"][:n])
    assert np.array_equal(got["status"][:n], exp["status"][:n]), label
    assert np.array_equal(np.isnan(got["err_norm"][:n]), np.isnan(exp["err_norm"][:n])), label
    with np.errstate(invalid="ignore"):                      # the poisoned rows: their NaN and inf are compared above and by the caller
        worst = max(np.nanmax(np.abs(got["q"][:n] - exp["q"][:n])), np.nanmax(np.nan_to_num(np.abs(got["err_norm"][:n] - exp["err_norm"][:n]))))
    print("device vs oracle, %s: %.3e" % (label, worst))
    assert worst <= DEVICE_TOL, (label, worst)
    return worst


@gpu
@pytest.mark.parametrize("name", ["newton", "half", "servo", "at_target", "far", "tiny_rotation", "nan"])
@pytest.mark.parametrize("pointers", ["host", "device"])
def test_the_device_solves_the_scene_as_the_oracle_does(handles, name, pointers):
    import torch
    sc, exp = scene(name), cases.solve_scene(name)
    h, n = handles(**sc["params"]), len(sc["q_init"])
    if pointers == "host":
        h.ik(sc["q_init"], sc["target"])
    else:
        h.ik(torch.tensor(sc["q_init"], device="cuda"), torch.tensor(sc["target"], device="cuda"))
    got = h.get_ik(n)
    compare(got, exp, n, "%s/%s" % (name, pointers))
    if name == "at_target":
        assert got["q"].tobytes() == sc["q_init"].tobytes()
    if name == "far":
        assert np.isfinite(got["q"]).all() and np.isfinite(got["err_norm"]).all()
    if name == "nan":
        bad = sorted(cases.NAN_ROWS)
        assert np.array_equal(got["q"][bad], sc["q_init"][bad], equal_nan=True) and (got["status"][bad] == -1).all()
        clean = scene("newton")
        h.ik(clean["q_init"], clean["target"])
        ref = h.get_ik(n)
        ok = [b for b in range(n) if b not in bad]
        for k in ("q", "err_norm", "iterations", "status"):
            assert got[k][ok].tobytes() == ref[k][ok].tobytes(), k                   # the batch mates of a poisoned problem: bit for bit
    if name == "servo":
        ratio = got["err_norm"] / exp["first_norm"]
        assert np.abs(ratio / (1.0 - 3e-3) ** 200 - 1.0).max() < 0.05


@gpu
@pytest.mark.parametrize("count", cases.COUNTS)
@pytest.mark.parametrize("stride", [56, 64])
@pytest.mark.parametrize("pointers", ["host", "device"])
def test_counts_and_strides(handles, count, stride, pointers):
    """one problem, less than a wavefront, exactly one, one more, 70; rows at 56 and at 64 bytes; what lies behind `count` in the result
    slabs is not touched"""
    import torch
    sc, exp = scene("newton"), cases.solve_scene("newton")
    h = handles(**sc["params"])
    view = h.ik_view()
    view["q"].fill_(-7.0)
    view["status"].fill_(-7)
    cols = stride // 8
    q = np.full((count, cols), np.nan)
    q[:, :7] = sc["q_init"][:count]
    t = np.full((count, 12 + cols - 7), np.nan)
    t[:, :12] = sc["target"][:count]
    if pointers == "host":
        h.ik(q[:, :7], t[:, :12])
    else:
        h.ik(torch.tensor(q, device="cuda")[:, :7], torch.tensor(t, device="cuda")[:, :12])
    compare(h.get_ik(count), exp, count, "count %d stride %d %s" % (count, stride, pointers))
    torch.cuda.synchronize()
    assert (view["q"][count:] == -7.0).all() and (view["status"][count:] == -7).all()


@gpu
def test_a_permuted_call_gives_permuted_results(handles):
    sc = scene("half")
    h = handles(**sc["params"])
    h.ik(sc["q_init"], sc["target"])
    ref = h.get_ik(cases.N)
    perm = np.random.default_rng(3).permutation(cases.N)
    h.ik(sc["q_init"][perm], sc["target"][perm])
    got = h.get_ik(cases.N)
    for k in ref:
        assert got[k].tobytes() == ref[k][perm].tobytes(), k                          # a problem does not depend on its lane or its mates


@gpu
def test_a_servo_sequence_runs_in_place_without_the_host(handles):
    """the q slab is the next call's q_init: three calls in stream order, then one read"""
    import torch
    sc, n = scene("servo"), 4
    h = handles(**sc["params"])
    target = torch.tensor(sc["target"][:n], device="cuda")
    view = h.ik_view()
    h.ik(torch.tensor(sc["q_init"][:n], device="cuda"), target)
    for _ in range(2):
        h.ik(view["q"][:n], target)
    got = h.get_ik(n)
    exp = dict(q=np.zeros((n, 7)), err_norm=np.zeros(n), iterations=np.zeros(n, np.int32), status=np.zeros(n, np.int32))
    for b in range(n):
        q = sc["q_init"][b]
        for _ in range(3):
            q, exp["err_norm"][b], exp["iterations"][b], exp["status"][b] = cases.ik_solve(q, sc["target"][b, :9].reshape(3, 3), sc["target"][b, 9:])
        exp["q"][b] = q
    compare(got, exp, n, "servo in place")
    assert (got["err_norm"] < 0.4 * cases.solve_scene("servo")["err_norm"][:n]).all()


@gpu
def test_fk_and_the_jacobian(handles):
    import torch
    h = handles()
    qs = np.tile(cases.Q0, (70, 1))
    qs[:, :6] += np.random.default_rng(8).uniform(-1.0, 1.0, (70, 6))
    qs[0] = 0.0
    exp_pose = np.array([cases.pose12(*cases.fk(q)) for q in qs])
    exp_jac = np.array([cases.jac_local(q) for q in qs])
    pose, jac = h.fk(qs)
    worst = max(np.abs(pose - exp_pose).max(), np.abs(jac - exp_jac).max())
    print("device vs oracle, fk and jacobian: %.3e" % worst)
    assert worst <= DEVICE_TOL
    dp, dj = torch.zeros((70, 12), dtype=torch.float64, device="cuda"), torch.zeros((70, 36), dtype=torch.float64, device="cuda")
    h.fk(torch.tensor(qs, device="cuda"), dp, dj)
    assert dp.cpu().numpy().tobytes() == pose.tobytes() and dj.cpu().numpy().tobytes() == jac.tobytes()
    h.fk(torch.tensor(qs, device="cuda"), dp.zero_(), None)
    assert dp.cpu().numpy().tobytes() == pose.tobytes()


@gpu
def test_grasp_poses_and_goal_rows(handles, arm):
    import torch
    h = handles()
    rng = np.random.default_rng(4)
    n = 70
    obj = np.column_stack([rng.uniform(-10, 10, n), rng.uniform(-10, 10, n), rng.uniform(0, 0.5, n), rng.uniform(-math.pi, math.pi, n)])
    class_of = rng.integers(0, 3, n).astype(np.int32)
    h.set_classes([arm.PRESETS[k] for k in arm.PRESET_NAMES])
    h.set_robot_classes(class_of)
    for which, cfg in ((arm.POSE_GRASP, "grasp_cfg"), (arm.POSE_PLAN, "plan_cfg")):
        exp = np.array([cases.grasp_pose(o, cases.class_row(cases.CLASS_NAMES[c])[cfg]) for o, c in zip(obj, class_of)])
        pose, goal = h.grasp_poses(obj, which)
        worst = max(np.abs(pose - exp).max(), np.abs(goal[:, :2] - exp[:, :2]).max())
        print("device vs oracle, grasp_poses %s: %.3e" % (cfg, worst))
        assert worst <= DEVICE_TOL and np.array_equal(goal[:, 2], obj[:, 3])
        dgoal = torch.zeros((n, 3), dtype=torch.float64, device="cuda")                 # stride 24: the layout manager_request reads
        h.grasp_poses(torch.tensor(obj, device="cuda"), which, None, dgoal)
        assert dgoal.cpu().numpy().tobytes() == goal.tobytes()
    h.set_robot_classes(torch.zeros(n, dtype=torch.int32, device="cuda"))
    pose, _ = h.grasp_poses(obj[:3], arm.POSE_GRASP)
    assert np.abs(pose - [cases.grasp_pose(o, cases.class_row("chair")["grasp_cfg"]) for o in obj[:3]]).max() <= DEVICE_TOL


@gpu
def test_refusals_come_before_anything_is_enqueued(handles, arm):
    import torch
    for bad in (dict(max_iter=0), dict(dt=0.0), dict(dt=math.nan), dict(eps=-1e-3), dict(eps=math.inf), dict(damp=0.0), dict(damp=math.nan)):
        with pytest.raises(arm.ArmError):
            arm.BatchedArm(4, **bad)
    h = handles()
    sc = scene("newton")
    h.ik(sc["q_init"][:4], sc["target"][:4])
    before = h.get_ik(8)
    q, t = np.tile(cases.Q0, (200, 1)), np.tile(sc["target"][0], (200, 1))
    with pytest.raises(arm.ArmError):
        h.ik(q, t)                                                                     # count > max_problems
    for qs, ts in ((48, 96), (56, 88), (60, 96), (56, 100)):
        with pytest.raises(arm.ArmError):
            h.ik_raw(4, q.ctypes.data, qs, t.ctypes.data, ts, 0)
    with pytest.raises(arm.ArmError):
        h.set_robot_classes(np.array([0, 1, 3], np.int32))                             # three classes: index 3 is outside
    with pytest.raises(arm.ArmError):
        h.set_robot_classes(np.array([0, -1], np.int32))
    with pytest.raises(arm.ArmError):
        h.set_classes([dict(arm.PRESETS["box"], category=7)])
    with pytest.raises(arm.ArmError):
        h.grasp_step(np.zeros((200, 2)), np.zeros((200, 4)), np.zeros((200, 7)), np.zeros((200, 7)))
    after = h.get_ik(8)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    torch.cuda.synchronize()


# ---- the grasp sequences --------------------------------------------------------------------------------------------------------------
def grasp_handle(arm):
    rows = cases.grasp_scene()
    h = arm.BatchedArm(8, **cases.GRASP_IK)
    h.set_classes([arm.PRESETS[k] for k in arm.PRESET_NAMES])
    h.set_robot_classes(np.array([r["class_index"] for r in rows], np.int32))
    return h, rows


INT_KEYS = ("grasp_time", "flag", "stable", "done", "ik_iterations", "ik_status")      # GraspFsm.INTS
DBL_KEYS = ("k", "d_gripper", "gripper_ang", "err_norm")


@pytest.fixture(scope="module")
def host_sequence(arm):
    """900 ticks issued from host arrays, the plant joint_positions <- joint_cmd on the host; the state after every tick"""
    h, rows = grasp_handle(arm)
    R = len(rows)
    obj, base = np.array([r["object_pose"] for r in rows]), np.array([r["arm_base_pose"] for r in rows])
    jp, out = np.tile(cases.Q0, (R, 1)), []
    for t in range(cases.GRASP_TICKS):
        h.grasp_step(np.array([r["robot_xy"][t] for r in rows]), obj, base, jp)
        s = h.get_grasp(R)
        jp = s["joint_cmd"].copy()
        out.append(s)
    h.close()
    return out


@gpu
def test_the_grasp_sequences_equal_the_oracle_tick_by_tick(host_sequence):
    ticks, _ = cases.run_grasp()
    worst = 0.0
    for t, (s, (ints, dbl, cmd, vel)) in enumerate(zip(host_sequence, ticks)):
        got = np.stack([s[k] for k in INT_KEYS], axis=1)
        assert np.array_equal(got, ints), (t, got, ints)
        assert np.array_equal(s["robot_vel_cmd"], vel), t
        worst = max(worst, np.abs(np.stack([s[k] for k in DBL_KEYS], axis=1) - dbl).max(), np.abs(s["joint_cmd"] - cmd).max())
    print("device vs oracle, grasp sequences: %.3e" % worst)
    assert worst <= DEVICE_TOL, worst
    assert sum(int(s["done"].sum()) for s in host_sequence) >= 10


@gpu
def test_the_grasp_sequences_run_on_device_pointers_without_the_host(arm, host_sequence):
    """the same 900 ticks with every array on the device, the joint_cmd slab as the next tick's joint_positions, no host wait in
    between (the state after every tick is copied aside on the same stream): bit for bit what the host-issued ticks gave"""
    import torch
    h, rows = grasp_handle(arm)
    R, T = len(rows), cases.GRASP_TICKS
    dev = lambda a: torch.tensor(np.asarray(a), device="cuda")
    xy = dev(np.array([[r["robot_xy"][t] for r in rows] for t in range(T)]))
    obj, base = dev(np.array([r["object_pose"] for r in rows])), dev(np.array([r["arm_base_pose"] for r in rows]))
    view = h.grasp_view()
    hist = {k: torch.zeros((T,) + tuple(v[:R].shape), dtype=v.dtype, device="cuda") for k, v in view.items()}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for t in range(T):
            h.grasp_step(xy[t], obj, base, view["joint_cmd"][:R], stream=stream)
            for k, v in view.items():
                hist[k][t].copy_(v[:R], non_blocking=True)
    stream.synchronize()
    for k in hist:
        got, exp = hist[k].cpu().numpy(), np.stack([s[k] for s in host_sequence])
        assert got.tobytes() == exp.tobytes(), k
    h.close()


@gpu
def test_reset_by_mask(arm):
    h, rows = grasp_handle(arm)
    R = len(rows)
    obj, base = np.array([r["object_pose"] for r in rows]), np.array([r["arm_base_pose"] for r in rows])
    for t in range(3):
        h.grasp_step(np.array([r["robot_xy"][t] for r in rows]), obj, base, np.tile(cases.Q0, (R, 1)))
    before = h.get_grasp(R)
    assert (before["grasp_time"] == 3).all() and before["robot_vel_cmd"][0, 0] == 0.15
    h.grasp_reset(R, [1, 0, 0, 1, 0])
    after = h.get_grasp(R)
    assert after["grasp_time"].tolist() == [0, 3, 3, 0, 3] and after["flag"].tolist() == [0, 1, 0, 0, 0]
    assert after["robot_vel_cmd"][0].tolist() == [0.0, 0.0, 0.0] and after["robot_vel_cmd"][2, 0] == -0.15
    assert after["gripper_ang"].tolist() == [-1.5] * 5 and after["err_norm"][0] == 1000.0 and after["ik_status"][0] == arm.IK_NOT_RUN
    h.close()
