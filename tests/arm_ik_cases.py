"""The oracle of csrc/z1_kinematics.h and the scenes of its tests: a sequential NumPy float64 restatement, one problem and one robot
at a time, in the shape of the reference's FSM (b2z1_object_fsm.py: the IK setup :136-151, object_grasp :643-749, to_se3 and
get_grasp_pose :848-873).  Its own FK, frame Jacobian, log6, Jlog6 and LDL^T; nothing of the product is imported here.

Pinocchio is not available, so the oracle is pinned by identities (tests/test_arm_ik_cpu.py), not by parity.

THE INPUT GUARD.  Every norm the loop compares with eps is recorded; guard() asserts that none is within 1e-9 of eps, and the grasp
sequences assert the same distance of err_norm from 0.1 and of the distance gap from +-0.02: an evaluation that is a few ulp off
cannot change an iteration count or a transition on these scenes."""
import functools
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CLASSES = json.load(open(os.path.join(HERE, "golden", "grasp_classes.json")))
CATEGORY = {"other": 0, "table": 1, "box": 2}          # ALORE_ARM_CATEGORY_*
CLASS_NAMES = ("chair", "table", "box")                # the class index of the presets

Q0 = np.array([0.0, 1.48, -0.63, -0.84, 0.0, 1.57, 0.0])   # joint_default, b2z1_object_fsm.py:148
JOINT1 = np.array([0.0, 0.0, 0.0585])
ORIGINS = np.array([[0.0, 0.0, 0.045], [-0.35, 0.0, 0.0], [0.218, 0.0, 0.057], [0.07, 0.0, 0.0], [0.0492, 0.0, 0.0]])   # joint2..6
AXES = (2, 1, 1, 1, 2, 0)
TOOL = np.array([0.051, 0.0, 0.0])
DEFAULTS = dict(eps=1e-3, max_iter=200, damp=1e-12, dt=3e-3)
SMALL = 1e-2            # below this angle log3 / log6 / Jlog6 use their series
GUARD = 1e-9
# the constants of object_grasp
REACH_BAND, APPROACH_SPEED, WAIT_TICKS, ERR_STABLE, STABLE_TICKS, TIMEOUT_TICKS = 0.02, 0.15, 100, 0.1, 20, 700
D_GRIPPER, K_MAX, GRIPPER_OPEN, GRIPPER_CLOSED, GRIPPER_TABLE = 0.01, 0.25, -1.5, -0.1, -0.4
IK_NOT_RUN = 3


def rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    if axis == 0:
        return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    if axis == 1:
        return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def chain(q, joint1=JOINT1, tool=TOOL):
    """the tool placement and, per joint, its axis in link00 and its origin"""
    R, p = np.eye(3), np.zeros(3)
    axes, at = [], []
    for i in range(6):
        p = p + R @ (joint1 if i == 0 else ORIGINS[i - 1])
        R = R @ rot(AXES[i], q[i])
        axes.append(R[:, AXES[i]].copy())
        at.append(p.copy())
    p = p + R @ tool
    return R, p, axes, at


def fk(q, joint1=JOINT1, tool=TOOL):
    R, p, _, _ = chain(q, joint1, tool)
    return R, p


def _jac(R, p, axes, at):
    a, r = np.array(axes), p - np.array(at)              # [6][3] each: the axes in link00 and the arms to the tool point
    lin = np.stack([a[:, 1] * r[:, 2] - a[:, 2] * r[:, 1], a[:, 2] * r[:, 0] - a[:, 0] * r[:, 2], a[:, 0] * r[:, 1] - a[:, 1] * r[:, 0]])
    return np.concatenate([R.T @ lin, R.T @ a.T])


def jac_local(q, joint1=JOINT1, tool=TOOL):
    """pin.computeFrameJacobian(..., LOCAL) of gripperStator: linear rows first, one column per arm joint"""
    return _jac(*chain(q, joint1, tool))


def log3(R):
    s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn = math.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2])
    c = 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0)
    theta = math.atan2(sn, c)
    if theta < SMALL:
        t2 = theta * theta
        f = 1.0 + t2 * (1.0 / 6.0 + t2 * (7.0 / 360.0 + t2 * (31.0 / 15120.0)))
    else:
        f = theta / sn
    return f * s, theta


def _alpha_beta(t):
    """alpha = (t / 2) cot(t / 2), beta = (1 - alpha) / t^2, and beta' / t"""
    t2 = t * t
    if t < SMALL:
        alpha = 1.0 - t2 * (1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0)))
        beta = 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0))
        bdot = 1.0 / 360.0 + t2 * (1.0 / 7560.0)
    else:
        h = 0.5 * t
        sh, ch = math.sin(h), math.cos(h)
        alpha = h * ch / sh
        beta = (1.0 - alpha) / t2
        bdot = (-2.0 / t2 + (1.0 + 2.0 * sh * ch / t) / (4.0 * sh * sh)) / t2
    return alpha, beta, bdot


def log6(R, p):
    """pin.log6(SE3(R, p)).vector: (v, w)"""
    w, t = log3(R)
    alpha, beta, _ = _alpha_beta(t)
    v = alpha * p - 0.5 * np.cross(w, p) + (beta * (w @ p)) * w
    return np.concatenate([v, w])


def jlog6(R, p):
    """pin.Jlog6(SE3(R, p)): [[A, B], [0, A]]"""
    w, t = log3(R)
    alpha, beta, bdot = _alpha_beta(t)
    A = beta * np.outer(w, w) + alpha * np.eye(3) + 0.5 * skew(w)
    wp = w @ p
    v3 = (bdot * wp) * w - (t * t * bdot + 2.0 * beta) * p
    Cm = np.outer(v3, w) + beta * np.outer(w, p) + (wp * beta) * np.eye(3) + 0.5 * skew(p)
    out = np.zeros((6, 6))
    out[0:3, 0:3] = A
    out[3:6, 3:6] = A
    out[0:3, 3:6] = Cm @ A
    return out


def exp6(x):
    """the inverse of log6, for the identity exp(log6(T)) = T only (closed form; not part of the contract)"""
    v, w = x[:3], x[3:]
    t = math.sqrt(w @ w)
    W = skew(w)
    if t < 1e-3:          # (1 - cos t) / t^2 and (t - sin t) / t^3 cancel: their series, exact to 1e-14 here
        a, b, c = 1.0 - t * t / 6.0, 0.5 - t * t / 24.0, 1.0 / 6.0 - t * t / 120.0
    else:
        a, b, c = math.sin(t) / t, 2.0 * math.sin(0.5 * t) ** 2 / (t * t), (t - math.sin(t)) / (t ** 3)
    return np.eye(3) + a * W + b * (W @ W), (np.eye(3) + b * W + c * (W @ W)) @ v


def ldlt_solve(A, b):
    """A x = b by LDL^T without pivoting, column by column; (x, ok): ok False at the first pivot that is not positive and finite"""
    n = len(b)
    A, b = np.asarray(A).tolist(), np.asarray(b).tolist()      # plain floats: the same IEEE arithmetic, without array overhead
    L, d = [[0.0] * n for _ in range(n)], [0.0] * n
    for j in range(n):
        s = A[j][j]
        for k in range(j):
            s -= L[j][k] * L[j][k] * d[k]
        if not (s > 0.0 and s < math.inf):
            return None, False
        d[j] = s
        for i in range(j + 1, n):
            s = A[i][j]
            for k in range(j):
                s -= L[i][k] * L[j][k] * d[k]
            L[i][j] = s / d[j]
    x = [0.0] * n
    for i in range(n):
        s = b[i]
        for k in range(i):
            s -= L[i][k] * x[k]
        x[i] = s
    for i in range(n):
        x[i] = x[i] / d[i]
    for i in range(n - 1, -1, -1):
        s = x[i]
        for k in range(i + 1, n):
            s -= L[k][i] * x[k]
        x[i] = s
    return np.array(x), True


def norm6(e):
    return math.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3] + e[4] * e[4] + e[5] * e[5])


def error(q, Rd, pd, joint1=JOINT1, tool=TOOL):
    """err = log6(oMf^-1 oMdes) and iMd"""
    Rf, pf = fk(q, joint1, tool)
    Ri, pi = Rf.T @ Rd, Rf.T @ (pd - pf)
    return log6(Ri, pi), Ri, pi


def ik_solve(q_init, Rd, pd, eps=1e-3, max_iter=200, damp=1e-12, dt=3e-3, norms=None):
    """b2z1_object_fsm.py:710-726.  Returns q[7], err_norm, iterations, status; norms: a list that receives every evaluated norm"""
    q_init = np.asarray(q_init, float)
    if not (np.all(np.isfinite(q_init)) and np.all(np.isfinite(Rd)) and np.all(np.isfinite(pd))):
        return q_init.copy(), math.nan, 0, -1
    q = q_init.copy()
    err_norm, it = math.nan, 0
    while it < max_iter:
        Rf, pf, axes, at = chain(q)
        Ri, pi = Rf.T @ Rd, Rf.T @ (pd - pf)
        err = log6(Ri, pi)
        err_norm = norm6(err)
        if norms is not None:
            norms.append(err_norm)
        if err_norm < eps:
            return q, err_norm, it, 0
        Je = -(jlog6(Ri.T, -(Ri.T @ pi)) @ _jac(Rf, pf, axes, at))
        A = Je @ Je.T + damp * np.eye(6)
        x, ok = ldlt_solve(A, err)
        if not ok:
            return q, err_norm, it, 2
        v = -(Je.T @ x)
        q[0:6] = q[0:6] + v * dt
        it += 1
    return q, err_norm, it, 1


def guard(norms, level=1e-3):
    worst = min((abs(n - level) for n in norms), default=1.0)
    assert worst >= GUARD, ("an evaluated norm is within 1e-9 of its threshold", worst)
    return worst


def quat_to_rot(q):
    """scipy's Rotation.from_quat(x, y, z, w).as_matrix(): the quaternion is normalised first"""
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    x, y, z, w = q[0] / n, q[1] / n, q[2] / n, q[3] / n
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                     [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                     [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]])


def rot_to_quat(R):
    """test plumbing only (building arm-base poses): x, y, z, w of a rotation that is not near a half turn"""
    w = 0.5 * math.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2]))
    return np.array([(R[2, 1] - R[1, 2]) / (4.0 * w), (R[0, 2] - R[2, 0]) / (4.0 * w), (R[1, 0] - R[0, 1]) / (4.0 * w), w])


def grasp_pose(obj, cfg):
    """get_grasp_pose: tf's quaternion_from_euler(0, pitch, yaw, 'sxyz') is Rz(yaw) Ry(pitch) as x, y, z, w"""
    dx, dz, pitch = cfg
    x, y, z, yaw = obj
    hp, hy = 0.5 * (pitch * (math.pi / 180.0)), 0.5 * yaw
    sp, cp, sy, cy = math.sin(hp), math.cos(hp), math.sin(hy), math.cos(hy)
    return np.array([x - dx * math.cos(yaw), y - dx * math.sin(yaw), z + dz, -sy * sp, cy * sp, sy * cp, cy * cp])


def base_target(base_pose, target_pose, category, k):
    """:672-696: T_base^-1 T_target with the class's adjustment in the base frame"""
    Rb, Rt = quat_to_rot(base_pose[3:7]), quat_to_rot(target_pose[3:7])
    R = Rb.T @ Rt
    p = Rb.T @ (np.asarray(target_pose[0:3], float) - np.asarray(base_pose[0:3], float))
    if category == CATEGORY["box"]:
        p[2] -= k / 2.2
    elif category == CATEGORY["table"]:
        p[0] += k / 1.5
        p[2] -= 0.01
    else:
        p[0] += k
        p[2] += 0.03
    return R, p


def class_row(name):
    c = CLASSES[name]
    return dict(category=CATEGORY.get(c["category"], 0), grasp_cfg=list(c["grasp_cfg"]), plan_cfg=list(c["plan_cfg"]),
                arm_default_pose=list(c["arm_default_pose"]))


class GraspFsm:
    """the grasp part of the FSM for ONE robot: the attributes of :143-151 and object_grasp"""
    INTS = ("grasp_time", "flag", "stable", "done", "ik_iterations", "ik_status")
    DOUBLES = ("k", "d_gripper", "gripper_ang", "err_norm")

    def __init__(self, cls, ik=None):
        self.cls, self.ik = cls, dict(DEFAULTS, **(ik or {}))
        self.joint_cmd, self.robot_vel_cmd = Q0.copy(), np.zeros(3)
        self.done, self.ik_iterations, self.ik_status = 0, 0, IK_NOT_RUN
        self.norms, self.gaps, self.err_seen = [], [], []
        self.reset()

    def reset(self):
        self.k, self.d_gripper, self.gripper_ang, self.err_norm = 0.0, 0.0, GRIPPER_OPEN, 1000.0
        self.grasp_time, self.flag, self.stable = 0, 0, 0

    def step(self, robot_xy, object_pose, arm_base_pose, joint_positions):
        self.done = self._step(robot_xy, object_pose, arm_base_pose, joint_positions)
        return self.done

    def _step(self, robot_xy, object_pose, arm_base_pose, joint_positions):
        c = self.cls
        self.ik_iterations, self.ik_status = 0, IK_NOT_RUN
        self.grasp_time += 1
        dx, dy = robot_xy[0] - object_pose[0], robot_xy[1] - object_pose[1]
        gap = math.sqrt(dx * dx + dy * dy) - c["plan_cfg"][0]
        if not self.flag:
            self.gaps.append(gap)
            self.joint_cmd = Q0.copy()
            if gap > REACH_BAND:
                self.robot_vel_cmd = np.array([APPROACH_SPEED, 0.0, 0.0])
            elif gap < -REACH_BAND:
                self.robot_vel_cmd = np.array([-APPROACH_SPEED, 0.0, 0.0])
            else:
                self.robot_vel_cmd = np.zeros(3)
                self.flag = 1
            return 0
        if self.grasp_time < WAIT_TICKS:
            return 0
        self.err_seen.append(self.err_norm)
        self.stable = self.stable + 1 if self.err_norm < ERR_STABLE else 0
        if self.stable > STABLE_TICKS or self.grasp_time > TIMEOUT_TICKS:
            self.d_gripper = D_GRIPPER
        self.k = min(self.k + self.d_gripper, K_MAX)
        Rd, pd = base_target(arm_base_pose, grasp_pose(object_pose, c["grasp_cfg"]), c["category"], self.k)
        q, self.err_norm, self.ik_iterations, self.ik_status = ik_solve(joint_positions, Rd, pd, norms=self.norms, **self.ik)
        self.gripper_ang = max(min(self.gripper_ang + self.d_gripper, GRIPPER_CLOSED), GRIPPER_OPEN)
        q[6] = self.gripper_ang
        if c["category"] == CATEGORY["table"] and self.gripper_ang >= GRIPPER_TABLE:
            q[0:6] = c["arm_default_pose"][0:6]
        if self.gripper_ang >= GRIPPER_CLOSED:
            self.d_gripper = D_GRIPPER          # the quirk: it stays 0.01 for every later grasp
            self.k, self.gripper_ang, self.err_norm, self.stable, self.flag, self.grasp_time = 0.0, GRIPPER_OPEN, 1000.0, 0, 0, 0
            return 1
        self.joint_cmd = q
        return 0

    def snapshot(self):
        return (np.array([getattr(self, n) for n in self.INTS], np.int64), np.array([getattr(self, n) for n in self.DOUBLES]),
                self.joint_cmd.copy(), self.robot_vel_cmd.copy())


# ---- the IK scenes ---------------------------------------------------------------------------------------------------------------
N = 70
N_SERVO = 16          # 200 iterations each: the long scene is the small one
COUNTS = (1, 3, 64, 65, 70)


def pose12(R, p):
    return np.concatenate([np.asarray(R).reshape(9), p])


def _targets(rng, n, spread=0.3):
    qs = np.tile(Q0, (n, 1))
    qs[:, 0:6] += rng.uniform(-spread, spread, (n, 6))
    return np.array([pose12(*fk(q)) for q in qs])


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> dict(params, q_init [n][7], target [n][12]); every scene starts at Q0 unless it says otherwise"""
    rng = np.random.default_rng(20240613)
    base = _targets(rng, N)
    start = np.tile(Q0, (N, 1))
    out = {"newton": dict(params=dict(dt=1.0), q_init=start, target=base),
           "half": dict(params=dict(dt=0.5), q_init=start, target=base),
           "servo": dict(params={}, q_init=start[:N_SERVO], target=base[:N_SERVO])}
    q_at = np.tile(Q0, (N, 1))
    q_at[:, 0:6] += rng.uniform(-0.3, 0.3, (N, 6))
    q_at[:, 6] = rng.uniform(-1.5, -0.1, N)          # the gripper entry passes through
    out["at_target"] = dict(params={}, q_init=q_at, target=np.array([pose12(*fk(q)) for q in q_at]))
    far = _targets(rng, 8)
    for i in range(8):
        a = 2.0 * math.pi * i / 8
        far[i, 9:12] += 1.5 * np.array([math.cos(a) * 0.8, math.sin(a) * 0.8, 0.6])
    out["far"] = dict(params=dict(max_iter=20), q_init=np.tile(Q0, (8, 1)), target=far)
    tiny, R0, p0 = [], *fk(Q0)
    for i in range(8):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        ang = (0.0, 1e-9, 1e-6, 1e-4, 1e-3, 5e-3, 9.9e-3, 1.01e-2)[i]   # both sides of the branch, and the identity
        W = skew(ax)
        Rt = R0 @ (np.eye(3) + math.sin(ang) * W + (1.0 - math.cos(ang)) * (W @ W))
        tiny.append(pose12(Rt, p0 + R0 @ rng.uniform(-0.03, 0.03, 3)))
    out["tiny_rotation"] = dict(params=dict(dt=1.0), q_init=np.tile(Q0, (8, 1)), target=np.array(tiny))
    for sc in out.values():
        sc["q_init"].setflags(write=False)
        sc["target"].setflags(write=False)
    return out


NAN_ROWS = {5: ("target", 4), 9: ("q_init", 2), 33: ("target", 10)}   # problem -> (array, column) poisoned in the `nan` scene


def nan_scene():
    sc = scenes()["newton"]
    q, t = sc["q_init"].copy(), sc["target"].copy()
    for b, (which, col) in NAN_ROWS.items():
        (q if which == "q_init" else t)[b, col] = math.nan if b != 9 else math.inf
    return dict(params=sc["params"], q_init=q, target=t)


@functools.lru_cache(maxsize=None)
def solve_scene(name):
    """the oracle's q [n][7], err_norm [n], iterations [n], status [n] of a scene, with the input guard applied"""
    sc = nan_scene() if name == "nan" else scenes()[name]
    p = dict(DEFAULTS, **sc["params"])
    n = len(sc["q_init"])
    q, e, it, st, first = np.zeros((n, 7)), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n)
    for b in range(n):
        norms = []
        q[b], e[b], it[b], st[b] = ik_solve(sc["q_init"][b], sc["target"][b, 0:9].reshape(3, 3), sc["target"][b, 9:12], norms=norms, **p)
        guard(norms, p["eps"])
        first[b] = norms[0] if norms else math.nan
    for a in (q, e, it, st, first):
        a.setflags(write=False)
    return dict(q=q, err_norm=e, iterations=it, status=st, first_norm=first)


# ---- the grasp sequences ------------------------------------------------------------------------------------------------------------
GRASP_TICKS = 900
# damp: with the reference's 1e-12 the iteration towards a pose OUT OF REACH is a chaotic map once the arm is stretched (near the
# singularity the step along the lost direction is dt e / sigma: the elbow angle follows x -> x - a / x); a perturbation of 1e-13
# in one joint grows to 1e+2 rad within twenty ticks, so no two evaluations agree and no tolerance can hold.  With damp = 1e-3 the
# same perturbation stays below 1e-13 (measured on robot 3), and the reachable robots converge as before
GRASP_IK = dict(max_iter=50, damp=1e-3)
# robot: class, how the base stands at the start (gap to plan_cfg[0] in metres), whether the grasp pose can be reached
GRASP_ROBOTS = (("chair", 0.305, True), ("table", 0.004, True), ("box", -0.215, True), ("chair", -0.011, False), ("box", 0.135, True))


@functools.lru_cache(maxsize=None)
def grasp_scene():
    """per robot: the class, the object pose, the arm-base pose (constant: the base stands while it grasps, the approach is scripted
    through robot_xy alone) and robot_xy [ticks][2].  The arm base is placed so that the class's grasp pose, seen from it, is
    fk(Q0 + a small offset) moved back by the class's adjustment at k = K_MAX / 2: the adjustment sweeps through reachable poses."""
    rng = np.random.default_rng(777)
    rows = []
    for r, (name, gap0, reachable) in enumerate(GRASP_ROBOTS):
        cls = class_row(name)
        obj = np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), 0.0, rng.uniform(-3.0, 3.0)])
        g = grasp_pose(obj, cls["grasp_cfg"])
        qd = Q0.copy()
        qd[0:6] += rng.uniform(-0.2, 0.2, 6)
        Rd, pd = fk(qd)
        # undo the adjustment at half of its travel
        Rz, pz = base_target(np.array([0, 0, 0, 0, 0, 0, 1.0]), np.array([0, 0, 0, 0, 0, 0, 1.0]), cls["category"], 0.5 * K_MAX)
        pd = pd - pz
        if not reachable:
            pd = pd + np.array([0.9, 0.3, 0.5])
        Rg = quat_to_rot(g[3:7])
        Rb = Rg @ Rd.T                       # T_base = T_grasp T_d^-1
        pb = g[0:3] - Rb @ pd
        base = np.concatenate([pb, rot_to_quat(Rb)])
        head = rng.uniform(-math.pi, math.pi)
        xy = np.zeros((GRASP_TICKS, 2))
        gap = gap0
        for t in range(GRASP_TICKS):
            d = cls["plan_cfg"][0] + gap
            xy[t] = obj[0] + d * math.cos(head), obj[1] + d * math.sin(head)
            if abs(gap) > REACH_BAND:            # the base closes in by a centimetre per tick and then stands
                gap -= math.copysign(0.01, gap)
        rows.append(dict(name=name, cls=cls, class_index=CLASS_NAMES.index(name), object_pose=obj, arm_base_pose=base, robot_xy=xy))
    return rows


@functools.lru_cache(maxsize=None)
def run_grasp():
    """900 ticks of every robot with the plant joint_positions <- joint_cmd.  Returns per tick the stacked snapshots
    (ints [R][6], doubles [R][4], joint_cmd [R][7], robot_vel_cmd [R][3]) and the machines (for the guard and the coverage)"""
    rows = grasp_scene()
    fsms = [GraspFsm(r["cls"], GRASP_IK) for r in rows]
    jp = [Q0.copy() for _ in rows]
    ticks = []
    for t in range(GRASP_TICKS):
        snaps = []
        for r, (row, m) in enumerate(zip(rows, fsms)):
            m.step(row["robot_xy"][t], row["object_pose"], row["arm_base_pose"], jp[r])
            jp[r] = m.joint_cmd.copy()
            snaps.append(m.snapshot())
        ticks.append(tuple(np.stack([s[i] for s in snaps]) for i in range(4)))
    for m in fsms:
        guard(m.norms, m.ik["eps"])
        guard(m.err_seen, ERR_STABLE)
        guard(m.gaps, REACH_BAND)
        guard(m.gaps, -REACH_BAND)
    return ticks, fsms
