"""ctypes binding of include/alore_arm.h: the batched Z1 grasp IK and the FSM's grasp step on the device.

torch is used for device memory and streams only; every kernel is HIP in libalore_nmpc.so and there is no CPU path
(``ArmError`` without a GPU).  Arrays may be NumPy arrays (HOST: uploaded, the call waits) or torch tensors on the device (read and
written in stream order, nothing waits); one call takes one kind."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)

CATEGORY_OTHER, CATEGORY_TABLE, CATEGORY_BOX = 0, 1, 2
POSE_GRASP, POSE_PLAN = 0, 1
IK_OK, IK_LIMIT, IK_PIVOT, IK_NOT_RUN, IK_NOT_FINITE = 0, 1, 2, 3, -1

# the three classes of the reference's config.yaml (`objects`), as numbers; the class index is the position in PRESET_NAMES
PRESET_NAMES = ("chair", "table", "box")
PRESETS = {
    "chair": dict(category=CATEGORY_OTHER, grasp_cfg=[0.45, 0.96, 60.0], plan_cfg=[0.8, 0.0, 0.0], arm_default_pose=[0.0, 1.9, -1.72, 0.72, 0.0, 0.0, -0.1]),
    "table": dict(category=CATEGORY_TABLE, grasp_cfg=[0.5, 0.62, 6.0], plan_cfg=[1.07, 0.0, 0.0], arm_default_pose=[0.0, 2.8, -1.15, -1.4, 0.0, 0.0, -0.1]),
    "box": dict(category=CATEGORY_BOX, grasp_cfg=[0.25, 0.45, 80.0], plan_cfg=[0.83, 0.0, 0.0], arm_default_pose=[0.0, 2.71, -0.82, -0.5, 0.0, 0.0, -0.1]),
}


class ArmParamsC(C.Structure):
    """alore_arm_params"""
    _fields_ = [("eps", C.c_double), ("damp", C.c_double), ("dt", C.c_double), ("max_iter", C.c_int), ("reserved", C.c_int),
                ("joint1_xyz", C.c_double * 3), ("tool_xyz", C.c_double * 3), ("joint_default", C.c_double * 7)]


class ArmClassC(C.Structure):
    """alore_arm_class"""
    _fields_ = [("category", C.c_int), ("reserved", C.c_int), ("grasp_cfg", C.c_double * 3), ("plan_cfg", C.c_double * 3),
                ("arm_default_pose", C.c_double * 7)]


class IkViewC(C.Structure):
    """alore_arm_ik_view"""
    _fields_ = [(k, C.c_void_p) for k in ("q", "err_norm", "iterations", "status")]


GRASP_FIELDS = (("joint_cmd", "f8", 7), ("robot_vel_cmd", "f8", 3), ("done", "i4", 0), ("k", "f8", 0), ("d_gripper", "f8", 0), ("gripper_ang", "f8", 0),
                ("err_norm", "f8", 0), ("grasp_time", "i4", 0), ("flag", "i4", 0), ("stable", "i4", 0), ("ik_iterations", "i4", 0), ("ik_status", "i4", 0))


class GraspViewC(C.Structure):
    """alore_arm_grasp_view"""
    _fields_ = [(k, C.c_void_p) for k, _, _ in GRASP_FIELDS]


class GraspHostC(C.Structure):
    """alore_arm_grasp_host"""
    _fields_ = [(k, C.c_void_p) for k, _, _ in GRASP_FIELDS]


class ArmError(RuntimeError):
    pass


def _bind(L):
    if getattr(L, "_arm_bound", False):
        return
    V, I = C.c_void_p, C.c_int
    L.alore_arm_default_params.restype = None
    L.alore_arm_default_params.argtypes = [C.POINTER(ArmParamsC)]
    L.alore_arm_last_error.restype = C.c_char_p
    L.alore_arm_last_error.argtypes = [V]
    for name, args in (("alore_arm_create", [C.POINTER(ArmParamsC), I, I, C.POINTER(V)]),
                       ("alore_arm_destroy", [V]),
                       ("alore_arm_fk", [V, I, V, I, V, I, V, I, I, V]),
                       ("alore_arm_ik", [V, I, V, I, V, I, I, V]),
                       ("alore_arm_device_ik", [V, C.POINTER(IkViewC)]),
                       ("alore_arm_get_ik", [V, I, V, V, V, V]),
                       ("alore_arm_set_classes", [V, I, C.POINTER(ArmClassC)]),
                       ("alore_arm_set_robot_classes", [V, I, V, I, V]),
                       ("alore_arm_grasp_poses", [V, I, V, I, I, V, I, V, I, I, V]),
                       ("alore_arm_grasp_reset", [V, I, V]),
                       ("alore_arm_grasp_step", [V, I, V, I, V, I, V, I, V, I, I, V]),
                       ("alore_arm_device_grasp", [V, C.POINTER(GraspViewC)]),
                       ("alore_arm_get_grasp", [V, I, C.POINTER(GraspHostC)])):
        fn = getattr(L, name)
        fn.restype = I
        fn.argtypes = args
    L._arm_bound = True


def default_params() -> ArmParamsC:
    """b2z1_object_fsm.py:705-708 and :148: eps 1e-3, 200 iterations, damp 1e-12, dt 3e-3; the Z1's joint1 and tool offsets"""
    L = _lib.load()
    _bind(L)
    p = ArmParamsC()
    L.alore_arm_default_params(C.byref(p))
    return p


class _DeviceArray:
    """a device allocation of the library as torch.as_tensor reads it"""

    def __init__(self, address, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(address), False), "version": 2}


def _stream(s):
    if s is None or isinstance(s, int):
        return s
    return int(s.cuda_stream)


def _is_device(a):
    return hasattr(a, "data_ptr")


def _arg(a, cols, name):
    """(address, stride in bytes, on the device, keep-alive) of rows of float64"""
    if _is_device(a):
        if a.dim() != 2 or a.shape[1] < cols or a.stride(1) != 1 or a.element_size() != 8:
            raise ArmError(f"{name}: a float64 device tensor [n][>={cols}] with unit column stride is needed")
        return int(a.data_ptr()), int(a.stride(0)) * 8, True, a
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] < cols or a.strides[1] != 8:
        a = np.ascontiguousarray(a.reshape(-1, cols))
    return a.ctypes.data, int(a.strides[0]), False, a


class BatchedArm:
    """B independent Z1 grasp problems / B robots of a fleet on one device.  ``params``: an ArmParamsC, or keywords of its fields."""

    def __init__(self, max_problems: int, params: ArmParamsC | None = None, device: int = 0, **fields):
        self.L = _lib.load()
        _bind(self.L)
        self.params = params or default_params()
        for k, v in fields.items():
            setattr(self.params, k, v)
        self.h = C.c_void_p()
        self.B = int(max_problems)
        self.device = device
        rc = self.L.alore_arm_create(C.byref(self.params), device, self.B, C.byref(self.h))
        if rc != 0:
            msg = self.L.alore_arm_last_error(None).decode()
            self.h = None
            raise ArmError(f"alore_arm_create failed ({rc}): {msg}")
        self.n_classes = len(PRESET_NAMES)

    def close(self):
        if getattr(self, "h", None):
            self.L.alore_arm_destroy(self.h)
            self.h = None

    __del__ = close

    def _check(self, rc):
        if rc != 0:
            raise ArmError(f"alore_arm error {rc}: {self.L.alore_arm_last_error(self.h).decode()}")

    def _tensor(self, address, shape, typestr):
        import torch
        return torch.as_tensor(_DeviceArray(address, shape, typestr), device=f"cuda:{self.device}")

    def _kinds(self, *arrays):
        dev = {_is_device(a) for a in arrays if a is not None}
        if len(dev) != 1:
            raise ArmError("the arrays of one call are all NumPy arrays or all device tensors")
        return dev.pop()

    # ---- kinematics ---------------------------------------------------------------------------------------------------------------
    def fk(self, q, pose=None, jac=None, stream=None):
        """q [n][7] -> (pose [n][12], jac [n][6][6]).  Device tensors: pose [n][12] and jac [n][36] are written in place (either may be
        None); NumPy: both are returned"""
        if self._kinds(q, pose, jac):
            qa, qs, _, _ = _arg(q, 7, "q")
            pa, ps = (_arg(pose, 12, "pose")[:2] if pose is not None else (None, 96))
            ja, js = (_arg(jac, 36, "jac")[:2] if jac is not None else (None, 288))
            self._check(self.L.alore_arm_fk(self.h, q.shape[0], qa, qs, pa, ps, ja, js, 1, _stream(stream)))
            return pose, jac
        qa, qs, _, keep = _arg(q, 7, "q")
        n = keep.shape[0]
        pose, jac = np.zeros((n, 12)), np.zeros((n, 6, 6))
        self._check(self.L.alore_arm_fk(self.h, n, qa, qs, pose.ctypes.data, 96, jac.ctypes.data, 288, 0, _stream(stream)))
        return pose, jac

    def ik(self, q_init, target, count=None, stream=None):
        """q_init [n][7], target [n][12]; the results stay on the device (ik_view, get_ik)"""
        dev = self._kinds(q_init, target)
        qa, qs, _, k1 = _arg(q_init, 7, "q_init")
        ta, ts, _, k2 = _arg(target, 12, "target")
        n = int(count if count is not None else k1.shape[0])
        self._check(self.L.alore_arm_ik(self.h, n, qa, qs, ta, ts, int(dev), _stream(stream)))

    def ik_raw(self, count, q_init, q_stride, target, target_stride, device_pointers, stream=None):
        """alore_arm_ik as it is: addresses and byte strides"""
        self._check(self.L.alore_arm_ik(self.h, count, q_init, q_stride, target, target_stride, device_pointers, _stream(stream)))

    def ik_view(self):
        """the device slabs as torch tensors: q [B][7], err_norm [B], iterations [B], status [B]"""
        v = IkViewC()
        self._check(self.L.alore_arm_device_ik(self.h, C.byref(v)))
        return dict(q=self._tensor(v.q, (self.B, 7), "<f8"), err_norm=self._tensor(v.err_norm, (self.B,), "<f8"),
                    iterations=self._tensor(v.iterations, (self.B,), "<i4"), status=self._tensor(v.status, (self.B,), "<i4"))

    def get_ik(self, count=None):
        n = self.B if count is None else int(count)
        out = dict(q=np.zeros((n, 7)), err_norm=np.zeros(n), iterations=np.zeros(n, np.int32), status=np.zeros(n, np.int32))
        self._check(self.L.alore_arm_get_ik(self.h, n, out["q"].ctypes.data, out["err_norm"].ctypes.data, out["iterations"].ctypes.data,
                                            out["status"].ctypes.data))
        return out

    # ---- classes ------------------------------------------------------------------------------------------------------------------
    def set_classes(self, classes):
        """a list of dicts with category, grasp_cfg, plan_cfg, arm_default_pose (PRESETS' values), or of ArmClassC"""
        rows = (ArmClassC * len(classes))()
        for r, c in zip(rows, classes):
            if isinstance(c, ArmClassC):
                C.memmove(C.byref(r), C.byref(c), C.sizeof(ArmClassC))
                continue
            r.category = int(c["category"])
            r.grasp_cfg[:], r.plan_cfg[:], r.arm_default_pose[:] = list(c["grasp_cfg"]), list(c["plan_cfg"]), list(c["arm_default_pose"])
        self._check(self.L.alore_arm_set_classes(self.h, len(classes), rows))
        self.n_classes = len(classes)

    def set_robot_classes(self, class_of, stream=None):
        if _is_device(class_of):
            if class_of.element_size() != 4 or not class_of.is_contiguous():
                raise ArmError("class_of: a contiguous int32 device tensor is needed")
            self._check(self.L.alore_arm_set_robot_classes(self.h, class_of.shape[0], int(class_of.data_ptr()), 1, _stream(stream)))
        else:
            a = np.ascontiguousarray(class_of, dtype=np.int32)
            self._check(self.L.alore_arm_set_robot_classes(self.h, len(a), a.ctypes.data, 0, _stream(stream)))

    def grasp_poses(self, object_pose, which=POSE_GRASP, out_pose=None, out_goal=None, stream=None):
        """object_pose [n][4] -> (pose [n][7], goal_xytheta [n][3]).  With POSE_PLAN the goal rows are what
        BatchedMSPlanner.manager_request takes as goals.  Device tensors are written in place; NumPy: both are returned"""
        if self._kinds(object_pose, out_pose, out_goal):
            oa, os_, _, _ = _arg(object_pose, 4, "object_pose")
            pa, ps = (_arg(out_pose, 7, "out_pose")[:2] if out_pose is not None else (None, 56))
            ga, gs = (_arg(out_goal, 3, "out_goal")[:2] if out_goal is not None else (None, 24))
            self._check(self.L.alore_arm_grasp_poses(self.h, object_pose.shape[0], oa, os_, int(which), pa, ps, ga, gs, 1, _stream(stream)))
            return out_pose, out_goal
        oa, os_, _, keep = _arg(object_pose, 4, "object_pose")
        n = keep.shape[0]
        pose, goal = np.zeros((n, 7)), np.zeros((n, 3))
        self._check(self.L.alore_arm_grasp_poses(self.h, n, oa, os_, int(which), pose.ctypes.data, 56, goal.ctypes.data, 24, 0, _stream(stream)))
        return pose, goal

    # ---- the grasp step -------------------------------------------------------------------------------------------------------------
    def grasp_reset(self, count=None, mask=None):
        n = self.B if count is None else int(count)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
        self._check(self.L.alore_arm_grasp_reset(self.h, n, None if m is None else m.ctypes.data))

    def grasp_step(self, robot_xy, object_pose, arm_base_pose, joint_positions, stream=None):
        """one tick of object_grasp for the robots of the rows; the state stays on the device (grasp_view, get_grasp)"""
        dev = self._kinds(robot_xy, object_pose, arm_base_pose, joint_positions)
        xa, xs, _, k1 = _arg(robot_xy, 2, "robot_xy")
        oa, os_, _, k2 = _arg(object_pose, 4, "object_pose")
        ba, bs, _, k3 = _arg(arm_base_pose, 7, "arm_base_pose")
        ja, js, _, k4 = _arg(joint_positions, 7, "joint_positions")
        self._check(self.L.alore_arm_grasp_step(self.h, k1.shape[0], xa, xs, oa, os_, ba, bs, ja, js, int(dev), _stream(stream)))

    def grasp_view(self):
        """the resident state as torch tensors on the device"""
        v = GraspViewC()
        self._check(self.L.alore_arm_device_grasp(self.h, C.byref(v)))
        return {k: self._tensor(getattr(v, k), (self.B, cols) if cols else (self.B,), "<" + t) for k, t, cols in GRASP_FIELDS}

    def get_grasp(self, count=None):
        n = self.B if count is None else int(count)
        out = {k: np.zeros((n, cols) if cols else n, np.float64 if t == "f8" else np.int32) for k, t, cols in GRASP_FIELDS}
        hostc = GraspHostC(**{k: out[k].ctypes.data for k in out})
        self._check(self.L.alore_arm_get_grasp(self.h, n, C.byref(hostc)))
        return out
