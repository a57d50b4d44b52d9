"""ctypes binding of include/alore_fsm.h: the whole ALORE task FSM of B robots on the device, on top of a BatchedArm.

torch is used for device memory and streams only; every kernel is HIP in libalore_nmpc.so and there is no CPU path (a BatchedArm
cannot be made without a GPU).  Arrays may be NumPy arrays (HOST: uploaded, the call waits) or torch tensors on the device (read in
stream order, nothing waits); one call takes one kind."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .arm import ArmError, BatchedArm, _arg, _is_device, _stream
from .arm import _bind as _bind_arm

(WAIT_TASK_PLANNING, WAIT_ROBOT_PATH, ROBOT_TRACKING, GRASPING, WAIT_OBJECT_PATH, OBJECT_TRACKING, RELEASING) = range(7)
STATE_NAMES = ("WAIT_TASK_PLANNING", "WAIT_ROBOT_PATH", "ROBOT_TRACKING", "GRASPING", "WAIT_OBJECT_PATH", "OBJECT_TRACKING", "RELEASING")
MAX_TASKS, CONTROL_ROW = 10, 15

# com_offset of the reference's config.yaml (`objects`), parallel to arm.PRESET_NAMES
PRESET_COM_OFFSETS = {"chair": [0.0, 0.0], "table": [0.3, 0.5], "box": [0.2, 0.3]}

PARAM_FIELDS = ("ticks_no_plan", "ticks_plan", "ticks_wait_path", "ticks_robot_reached", "ticks_grasp_done", "ticks_object_reached",
                "ticks_release", "ticks_release_done", "stop_after_back_off", "reserved")


class FsmParamsC(C.Structure):
    """alore_fsm_params"""
    _fields_ = [(k, C.c_int) for k in PARAM_FIELDS]


WORDS = ("task_state", "task_num", "n_tasks", "object_type", "target_type", "robot_path_index", "object_path_index", "n_robot_path",
         "n_object_path", "dwell", "finished", "is_task_plan", "back_off", "stop_after_back_off", "request_mask")
# name, dtype, the shape behind [B] as a function of (max_tasks, max_objects, max_path_points)
VIEW_FIELDS = tuple((w, "i4", ()) for w in WORDS) + (
    ("object_sequence", "i4", (MAX_TASKS,)), ("target_sequence", "i4", (MAX_TASKS,)), ("reach_threshold", "f8", ()), ("object_vel_cmd", "f8", (3,)),
    ("start_xytheta", "f8", (3,)), ("goal_xytheta", "f8", (3,)), ("object_pose_used", "f8", (4,)), ("control", "f8", (CONTROL_ROW,)),
    ("robot_path", "f8", ("P", 2)), ("object_path", "f8", ("P", 2)), ("target_poses", "f8", ("T", 4)))
COUNTERS = ("refused_sequences", "refused_paths")


class FsmViewC(C.Structure):
    """alore_fsm_view"""
    _fields_ = [(k, C.c_void_p) for k, _, _ in VIEW_FIELDS] + [("counters", C.c_void_p)] + \
               [(k, C.c_int) for k in ("max_tasks", "max_objects", "max_path_points", "reserved")]


def _bind(L):
    if getattr(L, "_fsm_bound", False):
        return
    _bind_arm(L)
    V, I = C.c_void_p, C.c_int
    L.alore_fsm_default_params.restype = None
    L.alore_fsm_default_params.argtypes = [C.POINTER(FsmParamsC)]
    for name, args in (("alore_fsm_create", [V, C.POINTER(FsmParamsC), I, I, I]),
                       ("alore_fsm_destroy", [V]),
                       ("alore_fsm_set_class_offsets", [V, I, V]),
                       ("alore_fsm_reset", [V, I, V]),
                       ("alore_fsm_set_targets", [V, I, V, I, I, V]),
                       ("alore_fsm_set_sequences", [V, I, V, I, V, V, I, V]),
                       ("alore_fsm_set_paths", [V, I, V, I, V, V, I, V]),
                       ("alore_fsm_tick", [V, I, V, I, V, I, V, I, V, I, I, V]),
                       ("alore_fsm_device_view", [V, C.POINTER(FsmViewC)]),
                       ("alore_fsm_get", [V, I, C.POINTER(FsmViewC)])):
        fn = getattr(L, name)
        fn.restype = I
        fn.argtypes = args
    L._fsm_bound = True


def default_params() -> FsmParamsC:
    """the reference's sleeps at its 100 Hz loop as tick counts: 10, 310, 10, 100, 200, 100, 10, 410; stop_after_back_off 0"""
    L = _lib.load()
    _bind(L)
    p = FsmParamsC()
    L.alore_fsm_default_params(C.byref(p))
    return p


def _ints(a, name):
    """(address, on the device, keep-alive) of packed int32"""
    if a is None:
        return None, None, None
    if _is_device(a):
        if a.element_size() != 4 or not a.is_contiguous():
            raise ArmError(f"{name}: a contiguous int32 device tensor is needed")
        return int(a.data_ptr()), True, a
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a.ctypes.data, False, a


class BatchedTaskFsm:
    """The task FSM of the robots of ``arm`` (a BatchedArm): the grasp state, the class table and the class of every robot are the
    arm's.  ``params``: an FsmParamsC, or keywords of its fields."""

    def __init__(self, arm: BatchedArm, max_tasks: int = 4, max_objects: int = 4, max_path_points: int = 256, params: FsmParamsC | None = None,
                 **fields):
        self.arm, self.L = arm, arm.L
        _bind(self.L)
        self.params = params or default_params()
        for k, v in fields.items():
            setattr(self.params, k, v)
        self.B, self.max_tasks, self.max_objects, self.max_path_points = arm.B, int(max_tasks), int(max_objects), int(max_path_points)
        self.open = False
        self._check(self.L.alore_fsm_create(arm.h, C.byref(self.params), self.max_tasks, self.max_objects, self.max_path_points))
        self.open = True

    def close(self):
        if getattr(self, "open", False) and getattr(self.arm, "h", None):
            self.L.alore_fsm_destroy(self.arm.h)
        self.open = False

    __del__ = close

    def _check(self, rc):
        if rc != 0:
            raise ArmError(f"alore_fsm error {rc}: {self.L.alore_arm_last_error(self.arm.h).decode()}")

    def _kind(self, *arrays):
        dev = {_is_device(a) for a in arrays if a is not None}
        if len(dev) != 1:
            raise ArmError("the arrays of one call are all NumPy arrays or all device tensors")
        return dev.pop()

    def set_class_offsets(self, com_offset):
        """com_offset [n_classes][2], parallel to the arm's class table"""
        a = np.ascontiguousarray(com_offset, dtype=np.float64).reshape(-1, 2)
        self._check(self.L.alore_fsm_set_class_offsets(self.arm.h, len(a), a.ctypes.data))

    def reset(self, count=None, mask=None):
        n = self.B if count is None else int(count)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
        self._check(self.L.alore_fsm_reset(self.arm.h, n, None if m is None else m.ctypes.data))

    def set_targets(self, target_poses, stream=None):
        """target_poses [n][max_tasks][4] (x, y, z, yaw)"""
        if _is_device(target_poses):
            t = target_poses.reshape(target_poses.shape[0], -1)
            a, s, _, _ = _arg(t, self.max_tasks * 4, "target_poses")
            self._check(self.L.alore_fsm_set_targets(self.arm.h, t.shape[0], a, s, 1, _stream(stream)))
            return
        t = np.ascontiguousarray(target_poses, dtype=np.float64).reshape(-1, self.max_tasks * 4)
        self._check(self.L.alore_fsm_set_targets(self.arm.h, len(t), t.ctypes.data, t.strides[0], 0, _stream(stream)))

    def set_sequences(self, order, n_order, mask=None, order_stride=None, count=None, stream=None):
        """task_state_callback.  order: int32 [n][>= n_order], item and target alternately, or a raw device address with
        order_stride bytes between robots and count (the `order` slab of BatchedMSPlanner.device_task(), stride 80)"""
        na, dev, k1 = _ints(n_order, "n_order") if not isinstance(n_order, int) else (n_order, True, None)
        ma, _, k2 = _ints(mask, "mask") if not isinstance(mask, int) else (mask, True, None)
        if isinstance(order, int):
            oa, stride, n = order, int(order_stride), int(count)
        elif _is_device(order):
            if order.element_size() != 4 or order.dim() != 2 or order.stride(1) != 1:
                raise ArmError("order: an int32 device tensor [n][m] with unit column stride is needed")
            oa, stride, n = int(order.data_ptr()), int(order.stride(0)) * 4, order.shape[0]
        else:
            order = np.ascontiguousarray(order, dtype=np.int32)
            order = order.reshape(len(k1), -1)
            oa, stride, n = order.ctypes.data, order.strides[0], len(order)
        self._check(self.L.alore_fsm_set_sequences(self.arm.h, n, oa, stride, na, ma, int(bool(dev)), _stream(stream)))

    def set_paths(self, xy, n_points, mask=None, stream=None):
        """path_callback.  xy [n][m][2] and n_points [n]: what BatchedMSPlanner.path_points_device writes"""
        dev = self._kind(xy, n_points, mask)
        na, _, k1 = _ints(n_points, "n_points")
        ma, _, k2 = _ints(mask, "mask")
        if dev:
            x = xy.reshape(xy.shape[0], -1)
            a, s, _, _ = _arg(x, 2, "xy")
            n = x.shape[0]
        else:
            x = np.ascontiguousarray(xy, dtype=np.float64)
            x = x.reshape(len(k1), -1)
            a, s, n = x.ctypes.data, x.strides[0], len(x)
        self._check(self.L.alore_fsm_set_paths(self.arm.h, n, a, s, na, ma, int(dev), _stream(stream)))

    def tick(self, robot_pose, object_poses, arm_base_pose, joint_positions, stream=None):
        """one tick: robot_pose [n][4], object_poses [n][max_objects][4] raw, arm_base_pose [n][7], joint_positions [n][7]; the state
        stays on the device (view, get; the arm's grasp_view, get_grasp)"""
        dev = self._kind(robot_pose, object_poses, arm_base_pose, joint_positions)
        o = object_poses.reshape(object_poses.shape[0], -1) if dev else np.ascontiguousarray(object_poses, dtype=np.float64).reshape(len(robot_pose), -1)
        if o.shape[1] < self.max_objects * 4:
            raise ArmError(f"object_poses: rows of max_objects = {self.max_objects} poses are needed")
        pa, ps, _, k1 = _arg(robot_pose, 4, "robot_pose")
        oa, os_, _, k2 = _arg(o, self.max_objects * 4, "object_poses")
        ba, bs, _, k3 = _arg(arm_base_pose, 7, "arm_base_pose")
        ja, js, _, k4 = _arg(joint_positions, 7, "joint_positions")
        self._check(self.L.alore_fsm_tick(self.arm.h, k1.shape[0], pa, ps, oa, os_, ba, bs, ja, js, int(dev), _stream(stream)))

    def _shape(self, tail, n):
        return (n,) + tuple({"P": self.max_path_points, "T": self.max_tasks}.get(d, d) for d in tail)

    def view(self):
        """the resident state as torch tensors on the device, by the names of alore_fsm_view; counters [2]"""
        v = FsmViewC()
        self._check(self.L.alore_fsm_device_view(self.arm.h, C.byref(v)))
        out = {k: self.arm._tensor(getattr(v, k), self._shape(tail, self.B), "<" + t) for k, t, tail in VIEW_FIELDS}
        out["counters"] = self.arm._tensor(v.counters, (len(COUNTERS),), "<i4")
        return out

    def get(self, count=None):
        """the same copied to NumPy arrays (waits for the device); counters as a dict"""
        n = self.B if count is None else int(count)
        out = {k: np.zeros(self._shape(tail, n), np.float64 if t == "f8" else np.int32) for k, t, tail in VIEW_FIELDS}
        cnt = np.zeros(len(COUNTERS), np.int32)
        v = FsmViewC(**{k: a.ctypes.data for k, a in out.items()}, counters=cnt.ctypes.data)
        self._check(self.L.alore_fsm_get(self.arm.h, n, C.byref(v)))
        out["counters"] = dict(zip(COUNTERS, cnt.tolist()))
        return out
