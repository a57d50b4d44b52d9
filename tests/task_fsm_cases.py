"""The oracle of csrc/task_fsm.h and the scenes of its tests: a sequential math / NumPy restatement of the reference's task FSM, one
robot at a time, in the shape of its methods (b2z1_object_fsm.py: FSM :511-572, path_callback :484-508, robot_tracking_controller
:575-640, object_tracking_controller :752-821, object_release :824-837, object_com_cal :876-897, the publishers :301-363, the control
row :366-375).  The grasp is tests/arm_ik_cases.py's GraspFsm, by import and unchanged; nothing of the product is imported here.

SLEEPS are skipped ticks: FSM() returns the number of ticks its call occupies and tick() counts them down (csrc/task_fsm.h).

THE INPUT GUARD.  Every comparison against a threshold is recorded: the distance against reach_threshold, |yaw error| against 5, 10
and 15 degrees, 2 e against the clamp, k against -0.15, and the remainder of wrap against 0; guard() asserts that none is within
1e-9 of its threshold on any scene, so a last-ulp difference in atan2, hypot or sincos cannot change an integer.  ONE EXCEPTION: k
is recorded against -0.15 but cannot keep a distance, because the release ends exactly when k, clamped to -0.15, equals it; that
comparison needs no distance: k is 0 minus 0.01 fifteen times, IEEE subtractions alone, the same bits in every evaluation (guard()).

THE SCENES.  Inputs are recorded by running the oracle against a kinematic follower: the robot is a unicycle that obeys
robot_vel_cmd; from the end of the grasp to the release the object is a unicycle that obeys object_vel_cmd and the robot rides behind
it at the class's grasp distance; the arm's joints follow joint_cmd; a stub planner answers every request a few ticks later with a
polyline of marker points, the last point of every piece twice.  The recorded inputs and deliveries are then replayed to the
header and to the device."""
import functools
import json
import math
import os

import numpy as np

from tests import arm_ik_cases as arm

HERE = os.path.dirname(os.path.abspath(__file__))
COM_OFFSETS = {k: v["com_offset"] for k, v in json.load(open(os.path.join(HERE, "golden", "fsm_classes.json"))).items()}
STATES = ("WAIT_TASK_PLANNING", "WAIT_ROBOT_PATH", "ROBOT_TRACKING", "GRASPING", "WAIT_OBJECT_PATH", "OBJECT_TRACKING", "RELEASING")
STATE = {n: i for i, n in enumerate(STATES)}                 # task_state_mapping
MAX_TASKS = 10
GUARD = 1e-9
TICK_NAMES = ("ticks_no_plan", "ticks_plan", "ticks_wait_path", "ticks_robot_reached", "ticks_grasp_done", "ticks_object_reached",
              "ticks_release", "ticks_release_done")
DEFAULT_TICKS = dict(zip(TICK_NAMES, (10, 310, 10, 100, 200, 100, 10, 410)))      # the reference's sleeps at 100 Hz
INT_NAMES = ("task_state", "task_num", "n_tasks", "object_type", "target_type", "robot_path_index", "object_path_index", "n_robot_path",
             "n_object_path", "dwell", "finished", "is_task_plan", "back_off", "stop_after_back_off", "request_mask")
DBL_NAMES = (("reach_threshold", 1), ("object_vel_cmd", 3), ("start_xytheta", 3), ("goal_xytheta", 3), ("object_pose_used", 4))


class Point:
    def __init__(self, x, y):
        self.x, self.y = x, y


class TaskFsm:
    """MovingBotController for ONE robot, without ROS"""

    def __init__(self, cls, com_offset, ticks=None, stop_after_back_off=0, n_objects=4, ik=None):
        self.cls, self.ticks, self.stop_after_back_off = cls, dict(DEFAULT_TICKS, **(ticks or {})), stop_after_back_off
        self.g = arm.GraspFsm(cls, ik)                       # k, d_gripper, joint_cmd, robot_vel_cmd ... and object_grasp
        self.task_state = "WAIT_TASK_PLANNING"
        self.obj_num = 1                                     # per robot: n_tasks
        self.n_objects = n_objects
        self.robot_path, self.object_path = [], []
        self.robot_pose = [0.0, 0.0, 0.0, 0.0]
        self.object_pose = [[0.0, 0.0, 0.0, 0.0] for _ in range(n_objects)]
        self.object_pose_rviz = [[0.0, 0.0, 0.0, 0.0] for _ in range(n_objects)]
        self.arm_base_pose, self.joint_positions = [0.0] * 7, [0.0] * 7
        self.object_vel_cmd = [0.0, 0.0, 0.0]
        self.object_type = self.target_type = 0
        self.object_sequence, self.target_sequence = list(range(MAX_TASKS)), list(range(MAX_TASKS))
        self.is_task_plan = False
        self.object_com_offset = list(com_offset)
        self.task_num = self.robot_path_index = self.object_path_index = 0
        self.target_poses = []
        self.reach_threshold = 0.25
        self.dwell, self.finished, self.back_off, self.request = 0, 0, 0, 0
        self.start_xytheta, self.goal_xytheta, self.object_pose_used = [0.0] * 3, [0.0] * 3, [0.0] * 4
        self.compared = []                                   # (value, threshold, what): the input guard
        self.branches = set()

    # ---- helpers -------------------------------------------------------------------------------------------------------------------
    def wrap(self, e):
        self.compared.append((math.fmod(e + math.pi, 2 * math.pi), 0.0, "wrap"))
        return (e + math.pi) % (2 * math.pi) - math.pi

    def clamp(self, omega, m):
        self.compared += [(omega, m, "clamp"), (omega, -m, "clamp")]
        return max(min(omega, m), -m)

    def task_state_callback(self, data, max_tasks=MAX_TASKS):
        """order: item and target alternately; a bad row is refused as a whole"""
        n = len(data)
        if n < 2 or n > 2 * max_tasks or n % 2 or any(not 0 <= v < self.n_objects for v in data[0::2]) or \
                any(not 0 <= v < max_tasks for v in data[1::2]):
            return False
        for i in range(n // 2):
            self.object_sequence[i], self.target_sequence[i] = data[2 * i], data[2 * i + 1]
        self.obj_num = n // 2
        self.is_task_plan = True
        return True

    def path_callback(self, points):
        if len(points) == 0:
            return
        if self.task_state == "WAIT_ROBOT_PATH":
            self.robot_path = [Point(*p) for p in points]
            self.robot_path_index = 0
            self.task_state = "ROBOT_TRACKING"
        elif self.task_state == "WAIT_OBJECT_PATH":
            self.object_path = [Point(*p) for p in points]
            self.object_path_index = 0
            self.task_state = "OBJECT_TRACKING"

    def get_grasp_pose(self, pose, cfg):
        return arm.grasp_pose(pose, cfg)

    def object_com_cal(self):
        dx, dy = self.object_com_offset
        for i in range(self.n_objects):
            x_c, y_c, z_c, yaw_c = self.object_pose_rviz[i]
            x_global = x_c + dx * math.cos(yaw_c) - dy * math.sin(yaw_c)
            y_global = y_c + dx * math.sin(yaw_c) + dy * math.cos(yaw_c)
            self.object_pose[i] = [x_global, y_global, z_c, yaw_c]

    # ---- one tick ------------------------------------------------------------------------------------------------------------------
    def tick(self, robot_pose, object_poses, arm_base_pose, joint_positions):
        self.robot_pose, self.object_pose_rviz = list(robot_pose), [list(p) for p in object_poses]
        self.arm_base_pose, self.joint_positions = list(arm_base_pose), list(joint_positions)
        self.object_com_cal()
        self.request = 0
        if self.dwell > 0:
            self.dwell -= 1
            self.branches.add("dwell")
            return
        if self.back_off:
            self.back_off = 0
            if self.stop_after_back_off:
                self.g.robot_vel_cmd = np.zeros(3)
                self.branches.add("stop_after_back_off")
        self.dwell = self.FSM() - 1
        if self._used:                                       # every call but WAIT_TASK_PLANNING's reads the object of object_type
            self.object_pose_used = list(self.object_pose[self.object_type])

    def FSM(self):
        """returns the ticks this call occupies"""
        t = self.ticks
        self._used = self.task_state != "WAIT_TASK_PLANNING"
        if self.task_state == "WAIT_TASK_PLANNING":
            if self.is_task_plan:
                self.task_state = "WAIT_ROBOT_PATH"
                self.task_num = 0
                self.branches.add("task plan")
                return t["ticks_plan"]
            self.branches.add("no task plan")
            return t["ticks_no_plan"]

        elif self.task_state == "WAIT_ROBOT_PATH":
            self.object_type = self.object_sequence[self.task_num]
            self.target_type = self.target_sequence[self.task_num]
            self.publish_planner_start_pose()
            self.publish_planner_goal_pose()
            return t["ticks_wait_path"]

        elif self.task_state == "ROBOT_TRACKING":
            if self.robot_tracking_controller():
                self.task_state = "GRASPING"
                return t["ticks_robot_reached"]

        elif self.task_state == "GRASPING":
            if self.g.step(self.robot_pose[0:2], self.object_pose[self.object_type], self.arm_base_pose, self.joint_positions):
                self.task_state = "WAIT_OBJECT_PATH"
                self.branches.add("grasp done")
                return t["ticks_grasp_done"]

        elif self.task_state == "WAIT_OBJECT_PATH":
            self.publish_planner_start_pose()
            self.publish_planner_goal_pose()
            return t["ticks_wait_path"]

        elif self.task_state == "OBJECT_TRACKING":
            if self.object_tracking_controller():
                self.task_state = "RELEASING"
                return t["ticks_object_reached"]

        elif self.task_state == "RELEASING":
            if self.object_release():
                self.task_num = self.task_num + 1
                self.g.robot_vel_cmd = np.array([-0.5, 0.0, 0.0])
                self.back_off = 1
                if self.task_num >= self.obj_num:
                    self.g.robot_vel_cmd = np.zeros(3)
                    self.finished, self.back_off = 1, 0
                    self.branches.add("all tasks completed")
                else:
                    self.task_state = "WAIT_ROBOT_PATH"
                    self.branches.add("next task")
                return t["ticks_release_done"]
            self.branches.add("release after the last task" if self.finished else "release call")
            return t["ticks_release"]
        return 1

    def publish_planner_start_pose(self):
        self.request = 1
        if self.task_state == "WAIT_ROBOT_PATH":
            self.start_xytheta = [self.robot_pose[0], self.robot_pose[1], self.robot_pose[3]]
        if self.task_state == "WAIT_OBJECT_PATH":
            o = self.object_pose[self.object_type]
            self.start_xytheta = [o[0], o[1], o[3]]

    def publish_planner_goal_pose(self):
        planner_goal_pose = self.get_grasp_pose(self.object_pose[self.object_type], self.cls["plan_cfg"])
        if self.task_state == "WAIT_ROBOT_PATH":
            self.goal_xytheta = [planner_goal_pose[0], planner_goal_pose[1], self.object_pose[self.object_type][3]]
            self.branches.add("robot request")
        if self.task_state == "WAIT_OBJECT_PATH":
            t = self.target_poses[self.target_type]
            self.goal_xytheta = [t[0], t[1], t[3]]
            self.branches.add("object request")

    def robot_tracking_controller(self):
        if self.robot_path_index >= len(self.robot_path):
            if len(self.robot_path) > 1:
                dx = self.object_pose[self.object_type][0] - self.robot_pose[0]
                dy = self.object_pose[self.object_type][1] - self.robot_pose[1]
                final_yaw = math.atan2(dy, dx)
                yaw_error = self.wrap(final_yaw - self.robot_pose[3])
                self.compared.append((abs(yaw_error), math.radians(5), "robot final yaw"))
                if abs(yaw_error) > math.radians(5):
                    omega = self.clamp(2.0 * yaw_error, 0.6)
                    self.g.robot_vel_cmd = np.array([0.0, 0.0, omega])
                    self.branches.add("robot final turn")
                    return False
            else:
                self.branches.add("robot path of one point")
            self.g.robot_vel_cmd = np.zeros(3)
            return True
        max_vx, max_wz, Kp_yaw = 0.5, 0.6, 2.0
        current_x, current_y, current_yaw = self.robot_pose[0], self.robot_pose[1], self.robot_pose[3]
        target = self.robot_path[self.robot_path_index]
        dx, dy = target.x - current_x, target.y - current_y
        dist = math.hypot(dx, dy)
        if self.robot_path_index == len(self.robot_path) - 1:
            self.branches.add("robot final point at threshold %g" % self.reach_threshold)
            self.reach_threshold = 0.15
        yaw_error = self.wrap(math.atan2(dy, dx) - current_yaw)
        self.compared.append((dist, self.reach_threshold, "robot reach"))
        if dist < self.reach_threshold:
            self.robot_path_index += 1
            self.branches.add("robot index at threshold %g" % self.reach_threshold)
            if dist == 0.0 or (self.robot_path_index >= 2 and (target.x, target.y) == (self.robot_path[self.robot_path_index - 2].x,
                                                                                        self.robot_path[self.robot_path_index - 2].y)):
                self.branches.add("robot doubled point")
            return False
        self.compared.append((abs(yaw_error), math.radians(15), "robot turn only"))
        if abs(yaw_error) > math.radians(15):
            vx = 0.0
            self.branches.add("robot turn only" + (" beyond 120 degrees" if abs(yaw_error) > math.radians(120) else ""))
        else:
            vx = max_vx
            self.branches.add("robot forward")
        omega = self.clamp(Kp_yaw * yaw_error, max_wz)
        self.g.robot_vel_cmd = np.array([vx, 0.0, omega])
        return False

    def object_tracking_controller(self):
        if self.object_path_index >= len(self.object_path):
            if len(self.object_path) > 1:
                last_point, second_last_point = self.object_path[-1], self.object_path[-2]
                dx, dy = last_point.x - second_last_point.x, last_point.y - second_last_point.y
                final_yaw = math.atan2(dy, dx)
                yaw_error = self.wrap(final_yaw - self.object_pose[self.object_type][3])
                self.compared.append((abs(yaw_error), math.radians(10), "object final yaw"))
                if abs(yaw_error) > math.radians(10):
                    omega = self.clamp(2.0 * yaw_error, 0.5)
                    self.object_vel_cmd = [0.0, 0.0, omega]
                    self.branches.add("object final turn")
                    return False
            else:
                self.branches.add("object path of one point")
            self.object_vel_cmd = [0.0, 0.0, 0.0]
            return True
        max_vx, max_wz, Kp_yaw = 0.5, 0.5, 2.0
        current_x, current_y = self.object_pose[self.object_type][0], self.object_pose[self.object_type][1]
        current_yaw = self.wrap(self.object_pose[self.object_type][3])
        target = self.object_path[self.object_path_index]
        dx, dy = target.x - current_x, target.y - current_y
        dist = math.hypot(dx, dy)
        if self.object_path_index == len(self.object_path) - 1:
            self.branches.add("object final point at threshold %g" % self.reach_threshold)
            self.reach_threshold = 0.2
        yaw_error = self.wrap(math.atan2(dy, dx) - current_yaw)
        self.compared.append((dist, self.reach_threshold, "object reach"))
        if dist < self.reach_threshold:
            self.object_path_index += 1
            self.branches.add("object index at threshold %g" % self.reach_threshold)
            return False
        self.compared.append((abs(yaw_error), math.radians(15), "object turn only"))
        if abs(yaw_error) > math.radians(15):
            vx = 0.0
            self.branches.add("object turn only")
        else:
            vx = max_vx
            self.branches.add("object forward")
        omega = self.clamp(Kp_yaw * yaw_error, max_wz)
        self.object_vel_cmd = [vx, 0.0, omega]
        return False

    def object_release(self):
        g = self.g
        if g.k != 0.0 or g.d_gripper != 0.0:
            self.branches.add("release from k = %g" % g.k)
        g.joint_cmd = np.array(self.cls["arm_default_pose"], float)
        g.joint_cmd[-1] = -1.5
        g.k = g.k - g.d_gripper
        self.compared.append((g.k, -0.15, "release"))
        g.k = max(g.k, -0.15)
        g.joint_cmd[1] = g.joint_cmd[1] + g.k
        g.robot_vel_cmd = np.zeros(3)
        if g.k <= -0.15:
            g.k = 0.0
            g.d_gripper = 0.0
            return True
        return False

    # ---- what is compared ----------------------------------------------------------------------------------------------------------
    def control_row(self):
        return np.concatenate([self.g.robot_vel_cmd, self.object_vel_cmd, self.g.joint_cmd, [STATE[self.task_state], self.object_type]])

    def snapshot(self):
        """ints [15] in the order of INT_NAMES, the grasp ints [6], doubles [14] in the order of DBL_NAMES, the grasp doubles [4],
        joint_cmd [7], robot_vel_cmd [3]"""
        ints = [STATE[self.task_state], self.task_num, self.obj_num, self.object_type, self.target_type, self.robot_path_index,
                self.object_path_index, len(self.robot_path), len(self.object_path), self.dwell, self.finished, int(self.is_task_plan),
                self.back_off, self.stop_after_back_off, self.request]
        dbl = [self.reach_threshold] + list(self.object_vel_cmd) + list(self.start_xytheta) + list(self.goal_xytheta) + list(self.object_pose_used)
        gi, gd, cmd, vel = self.g.snapshot()
        return np.array(ints, np.int64), gi, np.array(dbl, float), gd, cmd, vel


def guard(fsms):
    # `release`: k reaches -0.15 by design (it is clamped there, and that ends the release), so this one comparison cannot keep a
    # distance.  It needs none: k is 0 minus 0.01 fifteen times, IEEE subtractions alone, the same bits in every evaluation
    far = [(v, t, w) for m in fsms for v, t, w in m.compared if w != "release"]
    worst = min((abs(v - t) for v, t, _ in far), default=1.0)
    near = [(v, t, w) for v, t, w in far if abs(v - t) < GUARD]
    assert not near, ("a compared value is within 1e-9 of its threshold", near[:5])
    for m in fsms:
        arm.guard(m.g.norms, m.g.ik["eps"])
        arm.guard(m.g.err_seen, arm.ERR_STABLE)
        arm.guard(m.g.gaps, arm.REACH_BAND)
        arm.guard(m.g.gaps, -arm.REACH_BAND)
    return worst


# ---- the follower and the stub planner ---------------------------------------------------------------------------------------------
DT = 0.05                 # the follower's step: 2.5 cm per tick at 0.5 m/s
PANELS = 3                # marker points per piece: 3 panel ends, the last one twice
IK = dict(max_iter=20, damp=1e-3)      # arm_ik_cases.GRASP_IK's damping (its comment says why), fewer iterations per tick


def polyline(start, goal, kind):
    """the marker points of a plan from start to goal (x, y): `L` two pieces round a corner, `straight` two pieces in line, `one` the
    goal alone; per piece PANELS points, the last one twice"""
    if kind == "one":
        return [tuple(goal)]
    s, g = np.asarray(start, float), np.asarray(goal, float)
    corner = np.array([g[0], s[1]]) if kind == "L" else 0.5 * (s + g)
    pts = []
    for a, b in ((s, corner), (corner, g)):
        piece = [tuple(a + (b - a) * (i + 1) / PANELS) for i in range(PANELS)]
        pts += piece + [piece[-1]]
    return pts


def arm_base_for(cls, obj, rng_offset):
    """arm_ik_cases.grasp_scene's recipe: the base from which the class's grasp pose is fk(Q0 + offset), the adjustment undone at
    half of its travel: reachable"""
    g = arm.grasp_pose(obj, cls["grasp_cfg"])
    qd = arm.Q0.copy()
    qd[0:6] += rng_offset
    Rd, pd = arm.fk(qd)
    _, pz = arm.base_target(np.array([0, 0, 0, 0, 0, 0, 1.0]), np.array([0, 0, 0, 0, 0, 0, 1.0]), cls["category"], 0.5 * arm.K_MAX)
    pd = pd - pz
    Rb = arm.quat_to_rot(g[3:7]) @ Rd.T
    return np.concatenate([g[0:3] - Rb @ pd, arm.rot_to_quat(Rb)])


def com(raw, off):
    c, s = math.cos(raw[3]), math.sin(raw[3])
    return np.array([raw[0] + off[0] * c - off[1] * s, raw[1] + off[0] * s + off[1] * c, raw[2], raw[3]])


def run_scene(robots, ticks, tick_params, max_tasks, n_objects, plan_delay=3, seed=1):
    """robots: dicts with name (the class), pose (x, y, yaw), objects [n_objects][4] raw, targets [max_tasks][4], order, order_at (the
    tick before which the sequences arrive), robot_kind / object_kind (polyline kinds), stop_after_back_off.
    Returns dict(inputs [T][R] of (robot_pose, object_poses, base, joints), events [T][R] lists of ("S", order) / ("P", points),
    snaps [T][R], fsms)"""
    rng = np.random.default_rng(seed)
    R = len(robots)
    fsms, world = [], []
    for r in robots:
        cls = arm.class_row(r["name"])
        m = TaskFsm(cls, COM_OFFSETS[r["name"]], tick_params, r.get("stop_after_back_off", 0), n_objects, IK)
        m.target_poses = [list(t) for t in r["targets"]]
        fsms.append(m)
        world.append(dict(pose=np.array(r["pose"], float), objects=np.array(r["objects"], float), joints=arm.Q0.copy(), pending=None,
                          offset=rng.uniform(-0.2, 0.2, 6)))
    inputs, events, snaps = [], [], []
    for t in range(ticks):
        row_in, row_ev, row_sn = [], [], []
        for r, m, w in zip(robots, fsms, world):
            ev = []
            if t == r["order_at"]:
                assert m.task_state_callback(list(r["order"]), max_tasks)
                ev.append(("S", list(r["order"])))
            if w["pending"] is not None and w["pending"][0] == t:
                m.path_callback(w["pending"][1])
                ev.append(("P", w["pending"][1]))
                w["pending"] = None
            x, y, yaw = w["pose"]
            robot_pose = np.array([x, y, 0.0, yaw])
            obj_used = com(w["objects"][m.object_type], m.object_com_offset)
            base = arm_base_for(m.cls, obj_used, w["offset"])
            inp = (robot_pose, w["objects"].copy(), base, w["joints"].copy())
            m.tick(*inp)
            # the stub planner
            if m.request and w["pending"] is None:
                kind = r["robot_kind"] if m.task_state == "WAIT_ROBOT_PATH" else r["object_kind"]
                w["pending"] = (t + 1 + plan_delay, polyline(m.start_xytheta[0:2], m.goal_xytheta[0:2], kind))
            # the follower
            w["joints"] = m.g.joint_cmd.copy()
            if m.task_state in ("WAIT_OBJECT_PATH", "OBJECT_TRACKING"):
                o = w["objects"][m.object_type]
                vx, _, wz = m.object_vel_cmd
                o[0] += vx * math.cos(o[3]) * DT
                o[1] += vx * math.sin(o[3]) * DT
                o[3] += wz * DT
                c = com(o, m.object_com_offset)
                d = m.cls["plan_cfg"][0]
                w["pose"] = np.array([c[0] - d * math.cos(c[3]), c[1] - d * math.sin(c[3]), c[3]])
            else:
                vx, _, wz = m.g.robot_vel_cmd
                w["pose"] = w["pose"] + np.array([vx * math.cos(yaw) * DT, vx * math.sin(yaw) * DT, wz * DT])
            row_in.append(inp)
            row_ev.append(ev)
            row_sn.append(m.snapshot() + (m.control_row(),))
        inputs.append(row_in)
        events.append(row_ev)
        snaps.append(row_sn)
    guard(fsms)
    return dict(inputs=inputs, events=events, snaps=snaps, fsms=fsms, robots=robots, ticks=tick_params, max_tasks=max_tasks, n_objects=n_objects)


def ring(n, radius, cx=0.0, cy=0.0, phase=0.3):
    return [[cx + radius * math.cos(phase + 2 * math.pi * i / n), cy + radius * math.sin(phase + 2 * math.pi * i / n), 0.0,
             phase + 1.1 * i - 1.5] for i in range(n)]


MISSION_TICKS = dict(ticks_no_plan=2, ticks_plan=3, ticks_wait_path=2, ticks_robot_reached=3, ticks_grasp_done=4, ticks_object_reached=2,
                     ticks_release=1, ticks_release_done=4)
MISSION_CLASSES = ("chair", "table", "box", "chair", "table")
MISSION_MAX_TASKS, MISSION_OBJECTS = 2, 3
MISSION_LENGTH = 1500


@functools.lru_cache(maxsize=None)
def mission_scene():
    """5 robots of classes chair, table, box, chair, table with 2 tasks each, sequences that are not the identity, every dwell 1..4
    ticks; robot 2 runs stop_after_back_off = 1"""
    robots = []
    for r, name in enumerate(MISSION_CLASSES):
        robots.append(dict(name=name, pose=[0.3 * r, -0.2 * r, 0.4 * r - 0.9], objects=ring(MISSION_OBJECTS, 1.6 + 0.1 * r, 0.2, 0.1, 0.3 + 0.5 * r),
                           targets=[[2.6 - 0.3 * r, 1.2 + 0.2 * r, 0.0, 0.7], [-2.4, -1.5 + 0.3 * r, 0.0, -2.0]],
                           order=[(2, 1, 0, 0), (1, 0, 2, 1), (2, 0, 1, 1), (0, 1, 2, 0), (1, 1, 0, 0)][r], order_at=1 + r,
                           robot_kind="L" if r % 2 == 0 else "straight", object_kind="straight" if r % 2 == 0 else "L",
                           stop_after_back_off=1 if r == 2 else 0))
    return run_scene(robots, MISSION_LENGTH, MISSION_TICKS, MISSION_MAX_TASKS, MISSION_OBJECTS, seed=11)


TRACKING_LENGTH = 520


@functools.lru_cache(maxsize=None)
def tracking_scene():
    """robot 0: an L-shaped path, the start heading more than 120 degrees off; robot 1: a path of one point; robot 2: a straight path that
    ends across the object's axis, so that the final heading error exceeds the tolerance; robot 3: the object's path has one point"""
    ticks = dict(MISSION_TICKS)
    robots = [dict(name="chair", pose=[-2.0, -1.5, 2.9], objects=[[1.5, 1.0, 0.0, 1.2], [0.0, 3.0, 0.0, 0.0]], targets=[[3.0, 3.0, 0.0, 0.5]],
                   order=(0, 0), order_at=0, robot_kind="L", object_kind="L"),
              dict(name="box", pose=[0.2, 0.1, -0.4], objects=[[9.0, 9.0, 0.0, 0.0], [1.4, -0.3, 0.0, 0.3]], targets=[[2.0, -1.0, 0.0, 0.0]],
                   order=(1, 0), order_at=2, robot_kind="one", object_kind="straight"),
              dict(name="table", pose=[-1.0, 2.0, -1.2], objects=[[0.5, -1.0, 0.0, 2.4], [5.0, 5.0, 0.0, 0.0]], targets=[[-1.0, -2.5, 0.0, 1.0]],
                   order=(0, 0), order_at=1, robot_kind="straight", object_kind="straight"),
              dict(name="chair", pose=[1.0, 1.0, 0.5], objects=[[2.2, 1.8, 0.0, 0.6], [6.0, 0.0, 0.0, 0.0]], targets=[[2.4, 1.9, 0.0, 0.0]],
                   order=(0, 0), order_at=0, robot_kind="straight", object_kind="one")]
    return run_scene(robots, TRACKING_LENGTH, ticks, 1, 2, seed=5)


DEFAULT_LENGTH = 2100


@functools.lru_cache(maxsize=None)
def default_scene():
    """one robot with the reference's sleeps, its paths handed over on the tick after the request"""
    robots = [dict(name="chair", pose=[0.0, 0.0, 0.2], objects=[[1.8, 0.6, 0.0, 0.4]], targets=[[2.6, 1.4, 0.0, 0.0]], order=(0, 0), order_at=25,
                   robot_kind="straight", object_kind="straight")]
    return run_scene(robots, DEFAULT_LENGTH, None, 1, 1, plan_delay=0, seed=3)


def transitions(scene, r=0):
    """[(tick, state)] at which robot r's task_state changes"""
    out, last = [], None
    for t, row in enumerate(scene["snaps"]):
        s = int(row[r][0][0])
        if s != last:
            out.append((t, s))
            last = s
    return out
