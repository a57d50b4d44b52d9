"""Host-side mirror of the reference's `mpc` node numerics for a batch of robots (include/alore_ltv_mpc.h):
``BatchedLtvMpc.get_cmd`` = MpcController::getCmd (mpc_controller/src/mpc.cpp:569-614) for B robots on the GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)


class LtvConfig(C.Structure):
    _fields_ = [("dt", C.c_double), ("predict_steps", C.c_int), ("delay_num", C.c_int), ("matrix_q", C.c_double * 4),
                ("matrix_r", C.c_double * 2), ("matrix_rd", C.c_double * 2), ("max_vel", C.c_double), ("min_vel", C.c_double),
                ("max_omega", C.c_double), ("max_acc", C.c_double), ("max_domega", C.c_double), ("max_sweeps", C.c_int)]


class LtvPlantParams(C.Structure):
    _fields_ = [("max_acc", C.c_double), ("max_domega", C.c_double), ("pose_pub_period", C.c_double), ("state_propa_period", C.c_double),
                ("substeps", C.c_int), ("follow", C.c_int)]


class LtvPlantView(C.Structure):
    """device pointers (alore_ltv_plant_view): pose [B][3] at a 24-byte stride, vw [B][2], cmd [B][2], at_goal [B], status [B]"""
    _fields_ = [("pose", C.c_void_p), ("vw", C.c_void_p), ("cmd", C.c_void_p), ("at_goal", C.c_void_p), ("status", C.c_void_p)]


def _bind(L):
    if getattr(L, "_ltv_bound", False):
        return
    L.alore_ltv_default_config.argtypes = [C.POINTER(LtvConfig)]
    L.alore_ltv_default_config.restype = None
    L.alore_ltv_create.argtypes = [C.POINTER(LtvConfig), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.alore_ltv_destroy.argtypes = [C.c_void_p]
    L.alore_ltv_last_error.argtypes = [C.c_void_p]
    L.alore_ltv_last_error.restype = C.c_char_p
    L.alore_ltv_set_refs.argtypes = [C.c_void_p, C.c_int, DP, DP, C.c_void_p]
    L.alore_ltv_refs_from_store.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, DP, IP, C.c_void_p]
    L.alore_ltv_get_cmd.argtypes = [C.c_void_p, C.c_int, DP, C.c_int, C.c_int, C.c_void_p]
    L.alore_ltv_results.argtypes = [C.c_void_p, C.c_int, DP, DP, IP, IP, C.c_void_p]
    L.alore_ltv_commands.argtypes = [C.c_void_p, C.c_int, DP, IP, C.c_void_p]
    L.alore_ltv_tick.argtypes = [C.c_void_p, C.c_int, DP, C.c_int, C.c_int, DP, IP, C.c_void_p]
    L.alore_ltv_set_state.argtypes = [C.c_void_p, C.c_int, DP, DP, C.c_void_p]
    # the closed loop on the device
    L.alore_ltv_plant_default_params.argtypes = [C.POINTER(LtvPlantParams)]
    L.alore_ltv_plant_default_params.restype = None
    L.alore_ltv_plant_init.argtypes = [C.c_void_p, C.POINTER(LtvPlantParams), C.c_int]
    L.alore_ltv_plant_set_state.argtypes = [C.c_void_p, C.c_int, DP, DP, DP, C.c_void_p]
    L.alore_ltv_plant_get_state.argtypes = [C.c_void_p, C.c_int, DP, DP, IP, C.c_void_p]
    L.alore_ltv_plant_stop.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.alore_ltv_plant_device.argtypes = [C.c_void_p, C.POINTER(LtvPlantView)]
    L.alore_ltv_refs_from_store_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
    L.alore_ltv_get_cmd_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p]
    L.alore_ltv_plant_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.alore_ltv_closed_loop_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p]
    L.alore_ltv_plant_get_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, DP, DP, IP, IP, IP, C.c_void_p]
    # the closed loop on the ICR EKF's estimate, with the simulator's noise
    L.alore_ltv_plant_set_icr.argtypes = [C.c_void_p, C.c_int, DP, C.c_void_p]
    L.alore_ltv_plant_set_noise.argtypes = [C.c_void_p, C.c_double, DP, C.c_ulonglong]
    L.alore_ltv_plant_noise_draws.argtypes = [C.c_void_p, C.c_int, C.c_ulonglong, C.c_int, C.c_int, DP, C.c_void_p]
    L.alore_ltv_refs_from_store_est.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
    L.alore_ltv_get_cmd_est.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p]
    L.alore_ltv_plant_ekf_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
    L.alore_ltv_ekf_closed_loop_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int,
                                                C.c_void_p]
    L.alore_ltv_plant_get_trace_est.argtypes = [C.c_void_p, C.c_int, C.c_int, DP, IP, IP, C.c_void_p]
    L._ltv_bound = True


def default_config(**kw) -> LtvConfig:
    L = _lib.load()
    _bind(L)
    c = LtvConfig()
    L.alore_ltv_default_config(C.byref(c))
    for k, v in kw.items():
        if k.startswith("matrix_"):
            for i, x in enumerate(v):
                getattr(c, k)[i] = x
        else:
            setattr(c, k, v)
    return c


def _dp(a):
    return a.ctypes.data_as(DP) if a is not None else None


class LtvError(RuntimeError):
    pass


class BatchedLtvMpc:
    def __init__(self, max_robots: int, config: LtvConfig | None = None, device: int = 0):
        self.L = _lib.load()
        _bind(self.L)
        self.cfg = config or default_config()
        self.h = C.c_void_p()
        rc = self.L.alore_ltv_create(C.byref(self.cfg), device, max_robots, C.byref(self.h))
        if rc != 0:
            raise LtvError(f"alore_ltv_create failed ({rc}): no GPU or bad configuration; there is no CPU path")
        self.B, self.T, self.d = max_robots, self.cfg.predict_steps, self.cfg.delay_num

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.alore_ltv_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise LtvError(f"alore_ltv error {rc}: {self.L.alore_ltv_last_error(self.h).decode()}")

    def set_refs(self, xref, dref):
        """xref (B, T, 3): x, y, theta;  dref (B, T, 2): v, omega"""
        xref = np.ascontiguousarray(xref, np.float64); dref = np.ascontiguousarray(dref, np.float64)
        self._n = xref.shape[0]
        self._check(self.L.alore_ltv_set_refs(self.h, self._n, _dp(xref), _dp(dref), None))

    def refs_from_store(self, nmpc_engine, now, est):
        est = np.ascontiguousarray(est, np.float64)
        self._n = est.shape[0]
        goal = np.zeros(self._n, np.int32)
        self._check(self.L.alore_ltv_refs_from_store(self.h, nmpc_engine.h, self._n, float(now), _dp(est), goal.ctypes.data_as(IP), None))
        return goal.astype(bool)

    def set_state(self, output=None, buff=None):
        o = None if output is None else np.ascontiguousarray(output, np.float64)
        b = None if buff is None else np.ascontiguousarray(buff, np.float64)
        n = (o if o is not None else b).shape[0]
        self._check(self.L.alore_ltv_set_state(self.h, n, _dp(o), _dp(b), None))

    def tick(self, now_state, n_relin=5, reset=False):
        """getCmd for all robots, returning only what a control tick publishes: cmd (n, 2) and the status"""
        now_state = np.ascontiguousarray(now_state, np.float64)
        n = now_state.shape[0]
        cmd = np.zeros((n, 2)); st = np.zeros(n, np.int32)
        self._check(self.L.alore_ltv_tick(self.h, n, _dp(now_state), int(n_relin), 1 if reset else 0, _dp(cmd), st.ctypes.data_as(IP), None))
        return cmd, st

    def get_cmd(self, now_state, n_relin=5, reset=False):
        now_state = np.ascontiguousarray(now_state, np.float64)
        n = now_state.shape[0]
        self._check(self.L.alore_ltv_get_cmd(self.h, n, _dp(now_state), int(n_relin), 1 if reset else 0, None))
        out = np.zeros((n, self.T, 2)); xopt = np.zeros((n, self.T + 1, 3))
        sw = np.zeros(n, np.int32); st = np.zeros(n, np.int32)
        self._check(self.L.alore_ltv_results(self.h, n, _dp(out), _dp(xopt), sw.ctypes.data_as(IP), st.ctypes.data_as(IP), None))
        return {"output": out, "cmd": out[:, self.d].copy(), "xopt": xopt, "sweeps": sw, "status": st}

    def _relin_info(self, n):
        self.relin_iters = np.zeros(n, np.int32); self.du = np.zeros(n)
        self._check(self.L.alore_ltv_relin_info(self.h, n, self.relin_iters.ctypes.data_as(IP), _dp(self.du), None))

    def get_cmd_converge(self, now_state, max_relin=150, du_th=0.01, reset=False):
        """get_cmd with the reference's stopping rule (mpc.cpp:581-584; defaults: max_iter, du_threshold of mpc3ms.yaml): every
        robot stops after the first pass whose du = sum |change of the output| <= du_th.  Fills self.relin_iters (passes taken,
        -max_relin: never met, 0: non-finite input) and self.du (du of the last pass); both are in the returned dict too."""
        now_state = np.ascontiguousarray(now_state, np.float64)
        n = now_state.shape[0]
        self._check(self.L.alore_ltv_get_cmd_converge(self.h, n, _dp(now_state), int(max_relin), float(du_th), 1 if reset else 0, None))
        out = np.zeros((n, self.T, 2)); xopt = np.zeros((n, self.T + 1, 3))
        sw = np.zeros(n, np.int32); st = np.zeros(n, np.int32)
        self._check(self.L.alore_ltv_results(self.h, n, _dp(out), _dp(xopt), sw.ctypes.data_as(IP), st.ctypes.data_as(IP), None))
        self._relin_info(n)
        return {"output": out, "cmd": out[:, self.d].copy(), "xopt": xopt, "sweeps": sw, "status": st,
                "relin_iters": self.relin_iters, "du": self.du}

    # ---- the closed loop on the device: sampling from the plant's pose, the solve, the simulator's plant (no host in the loop).
    # Successive calls are ordered on the default stream.  du_th None: n_relin fixed passes; else the converge rule, n_relin its cap.
    def plant_init(self, max_trace_ticks=0, **params):
        """the plant of planner_sim.launch behind the `mpc` node; params: fields of alore_ltv_plant_params (follow=1: the plant
        holds the commanded velocity over the tick); max_trace_ticks: size of the per-tick trace ring"""
        p = LtvPlantParams()
        self.L.alore_ltv_plant_default_params(C.byref(p))
        for k, v in params.items():
            setattr(p, k, v)
        self._check(self.L.alore_ltv_plant_init(self.h, C.byref(p), int(max_trace_ticks)))
        self.plant_params = p

    def plant_set_state(self, pose, vw=None, desired=None):
        pose = np.ascontiguousarray(pose, np.float64)
        vw = None if vw is None else np.ascontiguousarray(vw, np.float64)
        desired = None if desired is None else np.ascontiguousarray(desired, np.float64)
        self._n = pose.shape[0]
        self._check(self.L.alore_ltv_plant_set_state(self.h, self._n, _dp(pose), _dp(vw), _dp(desired), None))

    def plant_get_state(self, n=None):
        """-> pose (n, 3), vw (n, 2), at_goal (n,) bool.  Synchronises."""
        n = self._n if n is None else n
        pose = np.zeros((n, 3)); vw = np.zeros((n, 2)); goal = np.zeros(n, np.int32)
        self._check(self.L.alore_ltv_plant_get_state(self.h, n, _dp(pose), _dp(vw), goal.ctypes.data_as(IP), None))
        return pose, vw, goal.astype(bool)

    def plant_stop(self, mask=None, n=None):
        """the zero command of emergencyStop for the robots of a DEVICE mask (an int32 tensor or an (address, stride) pair; None:
        all): v = omega = 0 and desired = 0.  Asynchronous."""
        n = self._n if n is None else n
        if mask is None:
            a, st = None, 0
        elif isinstance(mask, tuple):
            a, st = int(mask[0]), int(mask[1])
        else:
            a, st = int(mask.data_ptr()), int(mask.stride(0) * 4)
        self._check(self.L.alore_ltv_plant_stop(self.h, n, a, st, None))

    def refs_stop(self, nmpc_engine, mask=None):
        """the trajectories of the masked robots become invalid in the store this controller samples (BatchedNmpc.refs_stop)"""
        nmpc_engine.refs_stop(mask)

    def plant_view(self) -> LtvPlantView:
        v = LtvPlantView()
        self._check(self.L.alore_ltv_plant_device(self.h, C.byref(v)))
        return v

    @staticmethod
    def _du(du_th):
        return -1.0 if du_th is None else float(du_th)

    def refs_from_store_device(self, nmpc_engine, now, n=None):
        n = self._n if n is None else n
        self._check(self.L.alore_ltv_refs_from_store_device(self.h, nmpc_engine.h, n, float(now), None))

    def get_cmd_device(self, n_relin=5, du_th=None, reset=False, n=None):
        n = self._n if n is None else n
        self._check(self.L.alore_ltv_get_cmd_device(self.h, n, int(n_relin), self._du(du_th), 1 if reset else 0, None))

    def plant_step(self, n=None):
        n = self._n if n is None else n
        self._check(self.L.alore_ltv_plant_step(self.h, n, None))

    def closed_loop_run(self, nmpc_engine, t0, dt_tick, n_ticks, n_relin=5, du_th=None, reset=False, n=None):
        """n_ticks control periods at now = t0 + k * dt_tick, enqueued back to back; returns without waiting"""
        n = self._n if n is None else n
        self._check(self.L.alore_ltv_closed_loop_run(self.h, nmpc_engine.h, n, float(t0), float(dt_tick), int(n_ticks), int(n_relin),
                                                     self._du(du_th), 1 if reset else 0, None))

    def plant_trace(self, max_ticks, n=None):
        """the most recent plant steps, oldest first -> dict pose (k, n, 3), cmd (k, n, 2), status (k, n), at_goal (k, n).  Synchronises."""
        n = self._n if n is None else n
        m = max(int(max_ticks), 0)
        pose = np.zeros((m, n, 3)); cmd = np.zeros((m, n, 2)); st = np.zeros((m, n), np.int32); goal = np.zeros((m, n), np.int32)
        k = C.c_int(0)
        self._check(self.L.alore_ltv_plant_get_trace(self.h, n, m, _dp(pose), _dp(cmd), st.ctypes.data_as(IP), goal.ctypes.data_as(IP),
                                                     C.byref(k), None))
        k = k.value
        return {"pose": pose[:k], "cmd": cmd[:k], "status": st[:k], "at_goal": goal[:k]}

    # ---- the loop planner_sim.launch runs: the plant with the simulator's noise, the ICR EKF of `nmpc_engine` (the BatchedNmpc
    # that holds the trajectory store: ekf_init / ekf_reset / ekf_get there), sampling and the solve on the filter's estimate
    def plant_set_icr(self, icr):
        """the true (xv, yr, yl) per robot, (n, 3): what the simulator's ControlPub message is formed with"""
        icr = np.ascontiguousarray(icr, np.float64)
        self._check(self.L.alore_ltv_plant_set_icr(self.h, icr.shape[0], _dp(icr), None))

    def plant_set_noise(self, noise_stddev=0.0, meas_stddev=None, seed=0):
        """noise_stddev: the simulator's multiplicative noise on (v, omega) of every PoseSub (the launch file: 0.01); meas_stddev
        (3,): noise on the pose that updates the filter; seed: draws are a pure function of (seed, robot, event, stream).
        Restarts the event count."""
        m = None if meas_stddev is None else np.ascontiguousarray(meas_stddev, np.float64).reshape(3)
        self._check(self.L.alore_ltv_plant_set_noise(self.h, float(noise_stddev), _dp(m), int(seed) & (2 ** 64 - 1)))

    def plant_noise_draws(self, event0, n_events, stream=0, n=None):
        """the standard normals (n_events, n, 2) of the handle's seed for events event0 ..., drawn on the device.  Synchronises."""
        n = self._n if n is None else n
        out = np.zeros((max(int(n_events), 0), max(n, 0), 2))
        self._check(self.L.alore_ltv_plant_noise_draws(self.h, n, int(event0), int(n_events), int(stream), _dp(out), None))
        return out

    def refs_from_store_est(self, nmpc_engine, now, n=None):
        n = self._n if n is None else n
        self._check(self.L.alore_ltv_refs_from_store_est(self.h, nmpc_engine.h, n, float(now), None))

    def get_cmd_est(self, nmpc_engine, n_relin=5, du_th=None, reset=False, n=None):
        n = self._n if n is None else n
        self._check(self.L.alore_ltv_get_cmd_est(self.h, nmpc_engine.h, n, int(n_relin), self._du(du_th), 1 if reset else 0, None))

    def plant_ekf_step(self, nmpc_engine, dt_tick=0.01, n=None):
        """plant on the true state (noisy PoseSub), ControlPub, the filter step, the trace record: one launch"""
        n = self._n if n is None else n
        self._check(self.L.alore_ltv_plant_ekf_step(self.h, nmpc_engine.h, n, float(dt_tick), None))

    def ekf_closed_loop_run(self, nmpc_engine, t0, dt_tick, n_ticks, n_relin=5, du_th=None, reset=False, n=None):
        """n_ticks control periods of the loop on the estimate, enqueued back to back; returns without waiting"""
        n = self._n if n is None else n
        self._check(self.L.alore_ltv_ekf_closed_loop_run(self.h, nmpc_engine.h, n, float(t0), float(dt_tick), int(n_ticks), int(n_relin),
                                                         self._du(du_th), 1 if reset else 0, None))

    def plant_trace_est(self, max_ticks, n=None):
        """per tick of plant_trace: est (k, n, 3), the estimate after the filter step; ekf_status (k, n).  Synchronises."""
        n = self._n if n is None else n
        m = max(int(max_ticks), 0)
        est = np.zeros((m, max(n, 0), 3)); st = np.zeros((m, max(n, 0)), np.int32)
        k = C.c_int(0)
        self._check(self.L.alore_ltv_plant_get_trace_est(self.h, n, m, _dp(est), st.ctypes.data_as(IP), C.byref(k), None))
        return {"est": est[:k.value], "ekf_status": st[:k.value]}

    def results(self, n=None):
        """alore_ltv_results: the stored output, xopt, sweeps and status as they lie on the device.  Synchronises."""
        n = self._n if n is None else n
        out = np.zeros((n, self.T, 2)); xopt = np.zeros((n, self.T + 1, 3))
        sw = np.zeros(n, np.int32); st = np.zeros(n, np.int32)
        self._check(self.L.alore_ltv_results(self.h, n, _dp(out), _dp(xopt), sw.ctypes.data_as(IP), st.ctypes.data_as(IP), None))
        return {"output": out, "cmd": out[:, self.d].copy(), "xopt": xopt, "sweeps": sw, "status": st}

    def tick_converge(self, now_state, max_relin=150, du_th=0.01, reset=False):
        """tick with the stopping rule of get_cmd_converge: cmd (n, 2), status, relin_iters; self.du is fetched as well"""
        now_state = np.ascontiguousarray(now_state, np.float64)
        n = now_state.shape[0]
        cmd = np.zeros((n, 2)); st = np.zeros(n, np.int32); it = np.zeros(n, np.int32)
        self._check(self.L.alore_ltv_tick_converge(self.h, n, _dp(now_state), int(max_relin), float(du_th), 1 if reset else 0, _dp(cmd),
                                                   st.ctypes.data_as(IP), it.ctypes.data_as(IP), None))
        self._relin_info(n)
        return cmd, st, it
