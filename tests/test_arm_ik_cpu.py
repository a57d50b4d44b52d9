"""csrc/z1_kinematics.h (the Z1 grasp IK and the FSM's grasp step for one robot) on the CPU against its oracle,
tests/arm_ik_cases.py, and the build side of the feature: arm_ik.hip compiles for gfx950, the alore_arm_* calls are declared,
exported and bound.

Pinocchio is not installed, so the ORACLE is pinned by identities first (FK at 0, central differences of FK and of err(q),
exp(log6(T)) = T, the factorisation against np.linalg.solve, the quaternion of grasp_pose).  tests/harness/arm_ik_check.cpp
includes the header, is compiled with g++ -ffp-contract=off (once more with the address and undefined-behaviour sanitizers, as a
stand-alone program that is run directly) and is compared with the oracle on every scene: iterations, status, every integer of the
grasp state and the at_target bits EQUAL, the doubles within HEADER_VS_ORACLE (tests/test_arm_ik_gpu.py: the measured basis of
the device tolerance).

Status 2 (a pivot that is not positive and finite) is pinned on the oracle's factorisation only: no scene reaches it, because a
pivot at its threshold is exactly what the input guard keeps the scenes away from."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import arm_ik_cases as cases
from tests.test_arm_ik_gpu import HEADER_VS_ORACLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "harness", "arm_ik_check.cpp")
LIB = os.path.join(ROOT, "alore_legged_manipulator_amd", "libalore_nmpc.so")
FLAGS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
CALLS = ("alore_arm_default_params", "alore_arm_create", "alore_arm_destroy", "alore_arm_last_error", "alore_arm_fk", "alore_arm_ik",
         "alore_arm_device_ik", "alore_arm_get_ik", "alore_arm_set_classes", "alore_arm_set_robot_classes", "alore_arm_grasp_poses",
         "alore_arm_grasp_reset", "alore_arm_grasp_step", "alore_arm_device_grasp", "alore_arm_get_grasp")
SCENES = ("newton", "half", "servo", "at_target", "far", "tiny_rotation", "nan")


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("arm_ik_check")
    out = {}
    for name, flags in FLAGS.items():
        out[name] = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC, SRC, "-o", out[name]])
    return out


def nums(v):
    return " ".join(repr(float(x)) for x in np.asarray(v).reshape(-1))


def params_line(p):
    p = dict(cases.DEFAULTS, **p)
    return "P %r %r %r %d" % (p["eps"], p["damp"], p["dt"], p["max_iter"])


def run(exe, text, tmp_path):
    """the harness' output, one list of floats per line"""
    infile = tmp_path / "commands.txt"
    infile.write_text(text)
    r = subprocess.run([exe, str(infile)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-4000:])
    return [[float(v) for v in ln.split()] for ln in r.stdout.strip().split("\n")]


# ---- the oracle, pinned by identities -----------------------------------------------------------------------------------------------
def sample_q(seed, spread=0.6):
    q = cases.Q0.copy()
    q[0:6] += np.random.default_rng(seed).uniform(-spread, spread, 6)
    return q


def test_fk_at_zero_is_the_sum_of_the_origins():
    R, p = cases.fk(np.zeros(7))
    assert np.array_equal(R, np.eye(3))
    assert np.allclose(p, [0.0 + 0.0 - 0.35 + 0.218 + 0.07 + 0.0492 + 0.051, 0.0, 0.0585 + 0.045 + 0.057], rtol=0, atol=1e-15)
    R, p = cases.fk(np.array([0, 0, 0, 0, 0, 0, -0.7]))
    assert np.allclose(p, [0.0382, 0.0, 0.1605], rtol=0, atol=1e-15)       # the gripper joint does not move the tool frame


@pytest.mark.parametrize("seed", range(4))
def test_jac_local_is_the_derivative_of_fk(seed):
    q, h = sample_q(seed), 1e-6
    J, (R0, _) = cases.jac_local(q), cases.fk(q)
    for i in range(6):
        qa, qb = q.copy(), q.copy()
        qa[i] += h
        qb[i] -= h
        (Ra, pa), (Rb, pb) = cases.fk(qa), cases.fk(qb)
        S = R0.T @ (Ra - Rb) / (2 * h)
        fd = np.concatenate([R0.T @ (pa - pb) / (2 * h), [S[2, 1], S[0, 2], S[1, 0]]])
        assert np.abs(J[:, i] - fd).max() < 1e-8, (i, J[:, i], fd)


@pytest.mark.parametrize("seed", range(4))
def test_the_error_jacobian_is_the_derivative_of_err(seed):
    """-Jlog6(iMd^-1) J against central differences of err(q) = log6(oMf(q)^-1 oMdes); seed 3: a target 1e-3 rad away (the series)"""
    q, h = sample_q(seed), 1e-6
    Rd, pd = cases.fk(sample_q(seed + 100)) if seed < 3 else cases.fk(q + 1e-3)
    err, Ri, pi = cases.error(q, Rd, pd)
    Je = -(cases.jlog6(Ri.T, -(Ri.T @ pi)) @ cases.jac_local(q))
    for i in range(6):
        qa, qb = q.copy(), q.copy()
        qa[i] += h
        qb[i] -= h
        fd = (cases.error(qa, Rd, pd)[0] - cases.error(qb, Rd, pd)[0]) / (2 * h)
        assert np.abs(Je[:, i] - fd).max() < 1e-8, (i, Je[:, i], fd)


@pytest.mark.parametrize("angle", [0.0, 1e-9, 1e-4, 9.9e-3, 1.01e-2, 0.3, 1.5, 2.9])
def test_exp_of_log6_is_the_placement(angle):
    rng = np.random.default_rng(5)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    W = cases.skew(ax)
    R = np.eye(3) + math.sin(angle) * W + (1.0 - math.cos(angle)) * (W @ W)
    p = rng.uniform(-1, 1, 3)
    x = cases.log6(R, p)
    assert abs(math.sqrt(x[3:] @ x[3:]) - angle) < 1e-13
    R2, p2 = cases.exp6(x)
    assert np.abs(R2 - R).max() < 1e-13 and np.abs(p2 - p).max() < 1e-13


def test_the_series_meet_the_closed_forms():
    """both sides of SMALL agree as far as the closed forms can be evaluated there: alpha to an ulp; beta = (1 - alpha) / t^2 cancels,
    its error is 1e-16 / t^2 = 1e-12; beta' / t cancels twice, 2e-16 / t^4 = 2e-8.  (Both only multiply terms of the order t^2 |p|.)"""
    lo, hi = cases._alpha_beta(cases.SMALL * (1 - 1e-12)), cases._alpha_beta(cases.SMALL)
    assert abs(lo[0] - hi[0]) < 1e-15 and abs(lo[1] - hi[1]) < 2e-12 and abs(lo[2] - hi[2]) < 4e-8
    t = cases.SMALL
    assert abs((1.0 + t * t * (1 / 6 + t * t * (7 / 360 + t * t * 31 / 15120))) - t / math.sin(t)) < 1e-15


def test_the_factorisation_solves():
    rng = np.random.default_rng(9)
    for _ in range(20):
        Jm = rng.normal(size=(6, 6))
        A, b = Jm @ Jm.T + 1e-12 * np.eye(6), rng.normal(size=6)
        x, ok = cases.ldlt_solve(A, b)
        ref = np.linalg.solve(A, b)
        assert ok and np.abs(x - ref).max() <= 1e-9 * np.linalg.cond(A) * max(1.0, np.abs(ref).max()) * 1e-3
    assert cases.ldlt_solve(np.diag([1.0, 1.0, 0.0, 1.0, 1.0, 1.0]), np.ones(6))[1] is False
    assert cases.ldlt_solve(np.diag([1.0, -1.0, 1.0, 1.0, 1.0, 1.0]), np.ones(6))[1] is False
    assert cases.ldlt_solve(np.diag([1.0, math.inf, 1.0, 1.0, 1.0, 1.0]), np.ones(6))[1] is False


def test_grasp_pose_is_rz_ry():
    for name in cases.CLASS_NAMES:
        cfg = cases.CLASSES[name]["grasp_cfg"]
        obj = np.array([1.5, -2.0, 0.1, 2.2])
        g = cases.grasp_pose(obj, cfg)
        assert np.allclose(g[0:3], [1.5 - cfg[0] * math.cos(2.2), -2.0 - cfg[0] * math.sin(2.2), 0.1 + cfg[1]], rtol=0, atol=1e-15)
        assert np.abs(cases.quat_to_rot(g[3:7]) - cases.rot(2, 2.2) @ cases.rot(1, math.radians(cfg[2]))).max() < 1e-15
        assert abs(g[3:7] @ g[3:7] - 1.0) < 1e-15


def test_base_target_adjusts_by_category():
    base, tgt = np.array([1.0, 2.0, 0.5, 0.0, 0.0, math.sin(0.4), math.cos(0.4)]), np.array([1.3, 2.2, 0.9, 0.0, 0.3, 0.0, 2.0])
    R0, p0 = cases.base_target(base, tgt, cases.CATEGORY["other"], 0.0)
    assert np.abs(R0 - cases.rot(2, 0.8).T @ cases.quat_to_rot(tgt[3:7])).max() < 1e-15                # the quaternion is normalised
    assert np.allclose(p0 - [0.0, 0.0, 0.03], cases.rot(2, 0.8).T @ [0.3, 0.2, 0.4], rtol=0, atol=1e-15)
    for cat, shift in (("box", [0.0, 0.0, -0.2 / 2.2]), ("table", [0.2 / 1.5, 0.0, -0.01]), ("other", [0.2, 0.0, 0.03])):
        _, p = cases.base_target(base, tgt, cases.CATEGORY[cat], 0.2)
        assert np.allclose(p - (p0 - [0.0, 0.0, 0.03]), shift, rtol=0, atol=1e-15), cat


def test_the_class_numbers_are_the_presets():
    from alore_legged_manipulator_amd import arm
    for i, name in enumerate(cases.CLASS_NAMES):
        assert arm.PRESET_NAMES[i] == name and arm.PRESETS[name] == cases.class_row(name)


# ---- what the scenes are expected to do (on the oracle) --------------------------------------------------------------------------------
def test_the_scenes_do_what_they_are_for():
    s = {n: cases.solve_scene(n) for n in SCENES}
    for n in ("newton", "half", "tiny_rotation"):
        assert (s[n]["status"] == 0).all() and (s[n]["err_norm"] < 1e-3).all()
    assert set(s["newton"]["iterations"].tolist()) == {2, 3}                            # mixed across the problems of a wavefront
    assert len(s["half"]["iterations"]) == cases.N and len(set(s["half"]["iterations"].tolist())) >= 3
    assert (s["servo"]["status"] == 1).all() and (s["servo"]["iterations"] == 200).all()
    ratio = s["servo"]["err_norm"] / s["servo"]["first_norm"]
    assert np.abs(ratio / (1.0 - 3e-3) ** 200 - 1.0).max() < 0.05, ratio
    at = cases.scenes()["at_target"]
    assert (s["at_target"]["iterations"] == 0).all() and (s["at_target"]["status"] == 0).all()
    assert s["at_target"]["q"].tobytes() == at["q_init"].tobytes()
    assert (s["far"]["status"] == 1).all() and (s["far"]["iterations"] == 20).all()
    assert np.isfinite(s["far"]["q"]).all() and np.isfinite(s["far"]["err_norm"]).all()
    bad = sorted(cases.NAN_ROWS)
    ok = [b for b in range(cases.N) if b not in bad]
    assert (s["nan"]["status"][bad] == -1).all() and (s["nan"]["iterations"][bad] == 0).all()
    assert np.array_equal(s["nan"]["q"][bad], cases.nan_scene()["q_init"][bad], equal_nan=True)
    for k in ("q", "err_norm", "iterations", "status"):
        assert np.array_equal(s["nan"][k][ok], s["newton"][k][ok]), k
    first = s["tiny_rotation"]["first_norm"]
    assert (first > 0.01).all()                                                         # a real step from a rotation below SMALL


# ---- the header against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
@pytest.mark.parametrize("scene", SCENES)
def test_the_header_solves_the_scene_as_the_oracle_does(exes, build, scene, tmp_path):
    sc = cases.nan_scene() if scene == "nan" else cases.scenes()[scene]
    exp = cases.solve_scene(scene)
    text = [params_line(sc["params"])] + ["I %s %s" % (nums(q), nums(t)) for q, t in zip(sc["q_init"], sc["target"])]
    got = np.array(run(exes[build], "\n".join(text) + "\n", tmp_path))
    assert got.shape == (len(sc["q_init"]), 10)
    assert np.array_equal(got[:, 8].astype(int), exp["iterations"]) and np.array_equal(got[:, 9].astype(int), exp["status"])
    assert np.array_equal(np.isnan(got[:, 0:8]), np.isnan(np.column_stack([exp["q"], exp["err_norm"]])))
    with np.errstate(invalid="ignore"):                      # the poisoned rows of `nan`: inf - inf; their NaN pattern is compared above
        worst = max(np.nanmax(np.abs(got[:, 0:7] - exp["q"])), np.nanmax(np.abs(got[:, 7] - exp["err_norm"])))
    print("header vs oracle, %s: %.3e" % (scene, worst))
    assert worst <= HEADER_VS_ORACLE, worst
    if scene == "at_target":
        assert got[:, 0:7].tobytes() == sc["q_init"].tobytes()


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_the_header_has_the_oracles_pieces(exes, build, tmp_path):
    """fk, jac_local, log6, Jlog6, grasp_pose and base_target one by one, on poses of the scenes and on the small-angle branch"""
    sc, tiny = cases.scenes()["newton"], cases.scenes()["tiny_rotation"]
    qs = [cases.Q0, np.zeros(7)] + [sample_q(s) for s in range(6)]
    R0, p0 = cases.fk(cases.Q0)
    rel = [cases.pose12(R0.T @ t[0:9].reshape(3, 3), R0.T @ (t[9:12] - p0)) for t in list(sc["target"][:6]) + list(tiny["target"])]
    objs = [(np.array([0.3 * i, -0.2 * i, 0.05 * i, 0.9 * i - 2.0]), cases.CLASSES[n][cfg]) for i, n in enumerate(cases.CLASS_NAMES)
            for cfg in ("grasp_cfg", "plan_cfg")]
    rows = cases.grasp_scene()
    text = ["F " + nums(q) for q in qs] + ["L " + nums(t) for t in rel] + ["G %s %s" % (nums(o), nums(c)) for o, c in objs]
    text += ["B %s %s %d %r" % (nums(r["arm_base_pose"]), nums(cases.grasp_pose(r["object_pose"], r["cls"]["grasp_cfg"])), r["cls"]["category"], 0.1 * i)
             for i, r in enumerate(rows)]
    got = run(exes[build], "\n".join(text) + "\n", tmp_path)
    exp = [np.concatenate([cases.pose12(*cases.fk(q)), cases.jac_local(q).reshape(-1)]) for q in qs]
    exp += [np.concatenate([cases.log6(t[0:9].reshape(3, 3), t[9:12]), cases.jlog6(t[0:9].reshape(3, 3), t[9:12]).reshape(-1)]) for t in rel]
    exp += [cases.grasp_pose(o, c) for o, c in objs]
    exp += [cases.pose12(*cases.base_target(r["arm_base_pose"], cases.grasp_pose(r["object_pose"], r["cls"]["grasp_cfg"]), r["cls"]["category"], 0.1 * i))
            for i, r in enumerate(rows)]
    assert len(got) == len(exp)
    worst = max(np.abs(np.array(g) - e).max() for g, e in zip(got, exp))
    print("header vs oracle, pieces: %.3e" % worst)
    assert worst <= HEADER_VS_ORACLE, worst


def grasp_text():
    rows = cases.grasp_scene()
    text = [params_line(cases.GRASP_IK), "S %d %d" % (len(rows), cases.GRASP_TICKS)]
    for r in rows:
        c = r["cls"]
        text.append("%d %s %s %s %s %s" % (c["category"], nums(c["grasp_cfg"]), nums(c["plan_cfg"]), nums(c["arm_default_pose"]),
                                           nums(r["object_pose"]), nums(r["arm_base_pose"])))
    for t in range(cases.GRASP_TICKS):
        text += [nums(r["robot_xy"][t]) for r in rows]
    return "\n".join(text) + "\n"


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_the_header_steps_the_grasp_as_the_oracle_does(exes, build, tmp_path):
    ticks, _ = cases.run_grasp()
    R = len(cases.GRASP_ROBOTS)
    got = np.array(run(exes[build], grasp_text(), tmp_path)).reshape(cases.GRASP_TICKS, R, 20)
    worst = 0.0
    for t, (ints, dbl, cmd, vel) in enumerate(ticks):
        assert np.array_equal(got[t, :, 0:6].astype(np.int64), ints), (t, got[t, :, 0:6], ints)
        worst = max(worst, np.abs(got[t, :, 6:10] - dbl).max(), np.abs(got[t, :, 10:17] - cmd).max())
        assert np.array_equal(got[t, :, 17:20], vel), t
    print("header vs oracle, grasp sequences: %.3e" % worst)
    assert worst <= HEADER_VS_ORACLE, worst


def test_the_grasp_sequences_reach_every_branch():
    ticks, fsms = cases.run_grasp()
    ints = np.array([t[0] for t in ticks])                  # [tick][robot][grasp_time flag stable done ik_iterations ik_status]
    dbl = np.array([t[1] for t in ticks])                   # [tick][robot][k d_gripper gripper_ang err_norm]
    cmd, vel = np.array([t[2] for t in ticks]), np.array([t[3] for t in ticks])
    assert vel[0, :, 0].tolist() == [0.15, 0.0, -0.15, 0.0, 0.15]                      # too far, in range, too close
    assert (ints[:, :, 1].argmax(axis=0) == [29, 0, 20, 0, 12]).all()                  # the tick at which each robot enters the band
    done = [np.nonzero(ints[:, r, 3])[0].tolist() for r in range(5)]
    assert all(len(d) >= 2 for r, d in enumerate(done) if r != 3), done                # a second grasp follows the reset
    assert len(done[3]) == 1 and done[3][0] == 839 and min(fsms[3].err_seen) > 0.5     # out of reach: the grasp_time > 700 route
    assert dbl[699, 3, 1] == 0.0 and dbl[700, 3, 1] == 0.01 and ints[700, 3, 0] == 701
    for r in (0, 1, 2, 4):
        first, second = done[r][0], done[r][1]
        assert dbl[99, r, 1] == 0.0 and dbl[first - 1, r, 1] == 0.01 and ints[first, r, 0] == 0
        assert second - first == 99 + 140                                              # the quirk: d_gripper is 0.01 from the first tick after the wait
        assert dbl[first + 100, r, 1] == 0.01 and dbl[first + 100, r, 0] == 0.01
    table = cases.class_row("table")["arm_default_pose"]
    hit = np.nonzero((dbl[:, 1, 2] >= -0.4) & (ints[:, 1, 5] != cases.IK_NOT_RUN) & (ints[:, 1, 3] == 0))[0]
    assert len(hit) > 20 and all(cmd[t, 1, 0:6].tolist() == table[0:6] for t in hit)    # the default-pose switch of the table class
    assert not any(cmd[t, 2, 0:6].tolist() == cases.class_row("box")["arm_default_pose"][0:6] for t in range(cases.GRASP_TICKS))
    assert (ints[:, :, 5] != 2).all() and (ints[:, :, 5] != -1).all()
    assert {0, 1, cases.IK_NOT_RUN} <= set(ints[:, 0, 5].tolist())


# ---- the build side ---------------------------------------------------------------------------------------------------------------------
def test_calls_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alore_arm.h")).read(), flags=re.S)
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    from alore_legged_manipulator_amd import _lib, arm
    lib = _lib.load()
    arm._bind(lib)
    declared = sorted(set(re.findall(r"\b(alore_arm_[a-z_]+)\s*\(", hdr)))
    assert declared == sorted(CALLS)
    for name in CALLS:
        assert re.search(r"\b(int|void|const char \*)\s*" + name + r"\s*\(", hdr), name
        assert re.search(r"\sT\s+" + name + r"$", syms, re.M), name
        assert getattr(lib, name).argtypes is not None, name
    for method in ("fk", "ik", "ik_view", "get_ik", "set_classes", "set_robot_classes", "grasp_poses", "grasp_reset", "grasp_step", "grasp_view",
                   "get_grasp"):
        assert hasattr(arm.BatchedArm, method), method


def test_struct_mirrors_have_the_c_layout(tmp_path):
    from alore_legged_manipulator_amd import arm
    code = ('#include <stdio.h>\n#include "alore_arm.h"\nint main(){printf("%zu %zu %zu %zu %zu", sizeof(alore_arm_params), sizeof(alore_arm_class), '
            'sizeof(alore_arm_ik_view), sizeof(alore_arm_grasp_view), sizeof(alore_arm_grasp_host));}')
    (tmp_path / "s.c").write_text(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    sizes = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert sizes == [C.sizeof(arm.ArmParamsC), C.sizeof(arm.ArmClassC), C.sizeof(arm.IkViewC), C.sizeof(arm.GraspViewC), C.sizeof(arm.GraspHostC)]


def test_default_params_need_no_gpu():
    from alore_legged_manipulator_amd import arm
    p = arm.default_params()
    assert (p.eps, p.damp, p.dt, p.max_iter) == (1e-3, 1e-12, 3e-3, 200)
    assert list(p.joint1_xyz) == cases.JOINT1.tolist() and list(p.tool_xyz) == cases.TOOL.tolist() and list(p.joint_default) == cases.Q0.tolist()


def test_no_arm_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from alore_legged_manipulator_amd import arm
    with pytest.raises(arm.ArmError):
        arm.BatchedArm(4)


def test_the_kernels_are_in_the_gfx950_code_object():
    """arm_ik.hip is compiled for gfx950 and linked: its kernels are in the library's device code"""
    blob = open(LIB, "rb").read()
    for kernel in (b"ik_kernel", b"grasp_step_kernel", b"grasp_pose_kernel", b"fk_kernel"):
        assert re.search(rb"_ZN3arm\d+" + kernel, blob), kernel
    assert b"gfx950" in blob
