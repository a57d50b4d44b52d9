"""Host-side mirror of the reference's back_end entry point for a batch of problems.

``BatchedMSPlanner.minco_plan(flat_trajs)`` is ``MSPlanner::minco_plan(const FlatTrajData&)``
(planning_ddr_opt/back_end/src/optimizer.cpp:169-220) for many FlatTrajData at once, one wavefront per
problem on the GPU, through the C ABI of include/alore_backend.h.  Same parameter names as the reference's
yaml files (``config`` is alore_backend_config); results are what plan_manager reads back to build the
``Polynome`` message (plan_manager.hpp:784-831): ``polynomes()`` returns them in that wire format.
There is no CPU path: the constructor raises without the HIP library or without a GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

DP = C.POINTER(C.c_double)


class LbfgsParam(C.Structure):
    _fields_ = [("mem_size", C.c_int), ("past", C.c_int), ("max_iterations", C.c_int), ("max_linesearch", C.c_int),
                ("g_epsilon", C.c_double), ("delta", C.c_double), ("min_step", C.c_double), ("max_step", C.c_double),
                ("f_dec_coeff", C.c_double), ("s_curv_coeff", C.c_double), ("cautious_factor", C.c_double),
                ("machine_prec", C.c_double)]


class BackendConfig(C.Structure):
    """alore_backend_config (include/alore_backend.h)"""
    _fields_ = [("max_vel", C.c_double), ("min_vel", C.c_double), ("max_acc", C.c_double), ("max_omega", C.c_double),
                ("max_domega", C.c_double), ("max_cen_acc", C.c_double), ("direct_v_omega", C.c_int),
                ("w_time", C.c_double), ("w_acc", C.c_double), ("w_domega", C.c_double), ("w_collision", C.c_double),
                ("w_moment", C.c_double), ("w_mean_time", C.c_double), ("w_cen_acc", C.c_double),
                ("p_time", C.c_double), ("p_bigpath", C.c_double), ("p_moment", C.c_double), ("p_mean_time", C.c_double),
                ("p_acc", C.c_double), ("p_domega", C.c_double),
                ("energy_w", C.c_double * 2),
                ("smooth_eps", C.c_double), ("safe_dis", C.c_double), ("final_min_safe_dis", C.c_double),
                ("final_check_num", C.c_int), ("safe_replan_max", C.c_int),
                ("mean_lo", C.c_double), ("mean_hi", C.c_double),
                ("sparse_res", C.c_int), ("n_check", C.c_int), ("check_pts", (C.c_double * 2) * 8),
                ("icr_xv", C.c_double), ("standard_diff", C.c_int),
                ("lam0", C.c_double * 2), ("rho0", C.c_double * 2), ("rho_max", C.c_double * 2), ("gamma", C.c_double * 2),
                ("tol", C.c_double),
                ("cut_lam0", C.c_double * 2), ("cut_rho0", C.c_double * 2), ("cut_rho_max", C.c_double * 2),
                ("cut_gamma", C.c_double * 2), ("cut_tol", C.c_double),
                ("path_lbfgs", LbfgsParam), ("shot_path_past", C.c_int), ("shot_path_horizon", C.c_double),
                ("lbfgs", LbfgsParam), ("max_alm_rounds", C.c_int)]


class FlatTrajC(C.Structure):
    _fields_ = [("n_pieces", C.c_int), ("traj_pts", C.c_void_p), ("init_T", C.c_double), ("positions", C.c_void_p),
                ("start_state", (C.c_double * 3) * 2), ("final_state", (C.c_double * 3) * 2),
                ("start_xytheta", C.c_double * 3), ("final_xytheta", C.c_double * 3), ("if_cut", C.c_int)]


class StatusC(C.Structure):
    _fields_ = [("ok", C.c_int), ("attempts", C.c_int), ("alm_rounds", C.c_int), ("evals", C.c_int), ("lbfgs_ret", C.c_int),
                ("path_ret", C.c_int), ("collision", C.c_int), ("n_pieces", C.c_int), ("cost", C.c_double),
                ("xy_err", C.c_double * 2), ("min_dist", C.c_double), ("tail_s", C.c_double)]


class DeviceView(C.Structure):
    _fields_ = [("max_pieces", C.c_int), ("n_pieces", C.c_void_p), ("inner", C.c_void_p), ("T", C.c_void_p),
                ("coef", C.c_void_p), ("head", C.c_void_p), ("tail", C.c_void_p), ("start_xytheta", C.c_void_p),
                ("ok", C.c_void_p)]


class CheckC(C.Structure):
    """alore_backend_check (include/alore_backend.h)"""
    _fields_ = [("collision", C.c_int), ("first_panel", C.c_int), ("n_checked", C.c_int), ("pad", C.c_int),
                ("first_time", C.c_double), ("first_xy", C.c_double * 2), ("min_dist", C.c_double)]


class ClassStatC(C.Structure):
    """alore_backend_class_stat (include/alore_backend.h): the outcome of a plan launch per object class"""
    _fields_ = [("n", C.c_int), ("n_ok", C.c_int), ("n_collision", C.c_int), ("sum_attempts", C.c_int), ("sum_evals", C.c_longlong),
                ("max_evals", C.c_int), ("pad", C.c_int), ("min_dist", C.c_double), ("max_duration", C.c_double)]


class ClassViewC(C.Structure):
    """alore_backend_class_view: device addresses of the class table, the class and the effective xv per slot, the counter of
    clamped indices and the records of the last class_stats"""
    _fields_ = [("n_classes", C.c_int), ("pad", C.c_int), ("class_of", C.c_void_p), ("xv", C.c_void_p), ("clamped", C.c_void_p),
                ("classes", C.c_void_p), ("stats", C.c_void_p)]


class FrontEndParamsC(C.Structure):
    """alore_front_end_params (include/alore_backend.h); the fields of flat_traj.FrontEndParams"""
    _fields_ = [("distance_weight", C.c_double), ("yaw_weight", C.c_double), ("traj_cut_length", C.c_double),
                ("sample_time", C.c_double), ("min_traj_num", C.c_int), ("max_vel", C.c_double), ("max_acc", C.c_double)]


class PathsC(C.Structure):
    """alore_backend_paths: host or device addresses"""
    _fields_ = [("max_points", C.c_int), ("n_points", C.c_void_p), ("xy", C.c_void_p), ("start_yaw", C.c_void_p),
                ("end_yaw", C.c_void_p), ("start_vaj", C.c_void_p), ("start_oaj", C.c_void_p)]


class MapParamsC(C.Structure):
    """alore_backend_map_params (include/alore_backend.h)"""
    _fields_ = [("p_hit", C.c_double), ("p_miss", C.c_double), ("p_min", C.c_double), ("p_max", C.c_double), ("p_occ", C.c_double),
                ("detection_range", C.c_double), ("perspective", C.c_int)]


class ScanC(C.Structure):
    """alore_backend_scan: a cloud (host or device address) and the pose it was taken at"""
    _fields_ = [("points", C.c_void_p), ("n_points", C.c_int), ("point_stride_bytes", C.c_int), ("odom", C.c_double * 3)]


class MapViewC(C.Structure):
    _fields_ = [("grid", C.c_void_p), ("log_odds", C.c_void_p), ("dist", C.c_void_p), ("count_hit", C.c_void_p),
                ("count_all", C.c_void_p), ("nx", C.c_int), ("ny", C.c_int),
                ("x_lo", C.c_double), ("y_lo", C.c_double), ("res", C.c_double)]


class LaserParamsC(C.Structure):
    """alore_backend_laser_params (include/alore_backend.h): the parameters of the reference's laser simulator"""
    _fields_ = [("sensing_horizon", C.c_double), ("pc_resolution", C.c_double), ("hrz_laser_line_num", C.c_int),
                ("vtc_laser_line_num", C.c_int), ("vtc_laser_range_dgr", C.c_double), ("hrz_limited", C.c_int),
                ("hrz_laser_range_dgr", C.c_double), ("use_resolution_filter", C.c_int), ("if_perspective", C.c_int)]


class LaserViewC(C.Structure):
    """alore_backend_laser_view: device addresses of the slabs of the scans"""
    _fields_ = [("range_image", C.c_void_p), ("laser_points", C.c_void_p), ("world_points", C.c_void_p), ("index", C.c_void_p),
                ("compact_points", C.c_void_p), ("n_points", C.c_void_p), ("status", C.c_void_p), ("slots", C.c_int), ("bins", C.c_int),
                ("max_scans", C.c_int)]


class SearchParamsC(C.Structure):
    """alore_backend_search_params (include/alore_backend.h)"""
    _fields_ = [("safe_dis", C.c_double), ("window_margin", C.c_double)]


class TaskParamsC(C.Structure):
    """alore_backend_task_params (include/alore_backend.h)"""
    _fields_ = [("safe_dis", C.c_double), ("window_margin", C.c_double), ("mode", C.c_int)]


class TaskViewC(C.Structure):
    """alore_backend_task_view: device addresses of the slab of missions"""
    _fields_ = [("max_points", C.c_int), ("max_legs", C.c_int), ("status", C.c_void_p), ("matrix", C.c_void_p), ("order", C.c_void_p),
                ("n_order", C.c_void_p), ("total", C.c_void_p), ("leg_start_xy", C.c_void_p), ("leg_goal_xy", C.c_void_p),
                ("fields", C.c_void_p), ("sweeps", C.c_void_p)]


class TaskAssignViewC(C.Structure):
    """alore_backend_task_assign_view: device addresses of the assignment that TASK_ASSIGNED / TASK_JOINT chose"""
    _fields_ = [("assignment", C.c_void_p), ("assign_total", C.c_void_p)]


class MapEditC(C.Structure):
    """alore_backend_map_edit: a rectangle of the reference's paint* loops and the state it writes"""
    _fields_ = [("cx", C.c_double), ("cy", C.c_double), ("hx", C.c_double), ("hy", C.c_double), ("make_obs", C.c_int), ("reserved", C.c_int)]


class MissionParamsC(C.Structure):
    """alore_backend_mission_params (include/alore_backend.h)"""
    _fields_ = [("item_half", C.c_double), ("free_half", C.c_double), ("item_free_dist", C.c_double), ("target_lock_half", C.c_double),
                ("target_lock_dist", C.c_double), ("left_target_half", C.c_double), ("left_target_dist", C.c_double)]


class MissionViewC(C.Structure):
    """alore_backend_mission_view: device addresses of the slab of missions, their edit list and the paint counters"""
    _fields_ = [("max_tasks", C.c_int), ("edit_capacity", C.c_int), ("status", C.c_void_p), ("phase", C.c_void_p), ("goal_item", C.c_void_p),
                ("goal_target", C.c_void_p), ("goal_status", C.c_void_p), ("n_tasks", C.c_void_p), ("kinds", C.c_void_p), ("items", C.c_void_p),
                ("targets", C.c_void_p), ("edits", C.c_void_p), ("n_edits", C.c_void_p), ("counters", C.c_void_p)]


class ManagerParamsC(C.Structure):
    """alore_backend_manager_params (include/alore_backend.h)"""
    _fields_ = [("replan_time", C.c_double), ("max_replan_time", C.c_double), ("replan_on_collision_only", C.c_int),
                ("stop_inside_obstacle", C.c_int), ("stop_on_no_path", C.c_int), ("reserved", C.c_int)]


MANAGER_INT_ROWS = ("state", "have_goal", "have_start", "leg", "action", "returned", "plan_mask", "fresh_mask", "replan_mask", "stop_mask",
                    "after_plan_mask")
MANAGER_DOUBLE_ROWS = ("goal", "start", "plan_start_xytheta", "loop_start_time", "plan_start_time", "traj_start_time", "traj_total_time", "time")
MANAGER_COUNTERS = ("fresh", "replan", "going_to_goal", "stopped", "delivered", "arrived", "refused")
STATE_INIT, STATE_IDLE, STATE_PLANNING, STATE_REPLAN, STATE_GOINGTOGOAL, STATE_EMERGENCY_STOP = range(6)
ACTION_NONE, ACTION_FRESH, ACTION_REPLAN = 0, 1, 2


class ManagerViewC(C.Structure):
    """alore_backend_manager_view: device addresses of the slab of the robots' state machines"""
    _fields_ = [("max_problems", C.c_int), ("n_counters", C.c_int)] + [(k, C.c_void_p) for k in MANAGER_INT_ROWS + MANAGER_DOUBLE_ROWS] + \
        [("counters", C.c_void_p)]


# alore_backend_map_edit as a numpy dtype (what map_paint takes and mission_state returns)
EDIT_DTYPE = np.dtype([("cx", np.float64), ("cy", np.float64), ("hx", np.float64), ("hy", np.float64), ("make_obs", np.int32),
                       ("reserved", np.int32)])
MISSION_OK, MISSION_MASKED, MISSION_E_POINT, MISSION_E_TASKS = 0, 1, -1, -6
PHASE_NONE, PHASE_ITEM, PHASE_TARGET = 0, 1, 2
ITEM_SQUARE, ITEM_BOX, ITEM_TABLE, ITEM_CHAIR = 0, 1, 2, 3
MAX_PATH_POINTS = 31
TASK_MAX_TASKS, TASK_MAX_POINTS, TASK_MAX_LEGS = 10, 21, 20
TASK_GREEDY, TASK_OPTIMAL, TASK_ASSIGNED, TASK_JOINT = 0, 1, 2, 3
TASK_JOINT_MAX_TASKS = 5
TASK_OK, TASK_MASKED, TASK_E_ENDPOINT, TASK_E_WINDOW, TASK_E_TASKS, TASK_E_NO_ORDER = 0, 1, -1, -3, -6, -7
SEARCH_OK, SEARCH_MASKED, SEARCH_E_ENDPOINT, SEARCH_E_SAME_CELL, SEARCH_E_WINDOW, SEARCH_E_NO_PATH, SEARCH_E_POINTS = 0, 1, -1, -2, -3, -4, -5
TASK_E_RANGE = -8  # wide missions only (task_reserve): a cost field of the mission has a component of 32767 or more
SEARCH_E_RANGE = -6  # wide route only (search_reserve): a cost in the window has a component of 32767 or more
SEARCH_MAX_CELLS = 32768
LASER_OK, LASER_E_POSE, LASER_E_CAPACITY = 0, -1, -2
LASER_MAX_BINS = 8192
BUILD_OK, BUILD_MASKED, BUILD_E_POINTS, BUILD_E_PIECES = 0, 1, -1, -2


# the same record as a numpy dtype (what check_plans unpacks, and what a copy of the device slab holds)
CHECK_DTYPE = np.dtype([("collision", np.int32), ("first_panel", np.int32), ("n_checked", np.int32), ("pad", np.int32),
                        ("first_time", np.float64), ("first_xy", np.float64, 2), ("min_dist", np.float64)])


# alore_backend_class_stat as a numpy dtype (what class_stats returns)
CLASS_STAT_DTYPE = np.dtype([("n", np.int32), ("n_ok", np.int32), ("n_collision", np.int32), ("sum_attempts", np.int32),
                             ("sum_evals", np.int64), ("max_evals", np.int32), ("pad", np.int32), ("min_dist", np.float64),
                             ("max_duration", np.float64)])
MAX_CLASSES = 256


def _bind(L):
    if getattr(L, "_backend_bound", False):
        return
    L.alore_backend_set_classes.argtypes = [C.c_void_p, C.c_int, C.POINTER(BackendConfig), C.POINTER(FrontEndParamsC)]
    L.alore_backend_set_problem_classes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.alore_backend_device_classes.argtypes = [C.c_void_p, C.POINTER(ClassViewC)]
    L.alore_backend_class_stats.argtypes = [C.c_void_p, C.c_int, C.POINTER(ClassStatC), C.c_void_p]
    L.alore_backend_default_config.argtypes = [C.POINTER(BackendConfig)]
    L.alore_backend_default_config.restype = None
    L.alore_backend_create.argtypes = [C.POINTER(BackendConfig), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.alore_backend_destroy.argtypes = [C.c_void_p]
    L.alore_backend_last_error.argtypes = [C.c_void_p]
    L.alore_backend_last_error.restype = C.c_char_p
    L.alore_backend_set_map.argtypes = [C.c_void_p, DP, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]
    L.alore_backend_build_esdf.argtypes = [C.c_void_p, C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                           C.c_double, C.c_double, C.c_double, DP]
    L.alore_backend_predicted_state.argtypes = [C.c_void_p, C.c_int, C.c_double, DP, DP, DP, DP, DP, DP, C.POINTER(C.c_int)]
    L.alore_backend_path_points.argtypes = [C.c_void_p, C.c_int, C.c_int, DP, DP, C.POINTER(C.c_int)]
    L.alore_backend_path_points_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.alore_backend_set_problems.argtypes = [C.c_void_p, C.c_int, C.POINTER(FlatTrajC), C.c_void_p]
    L.alore_backend_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.alore_backend_results.argtypes = [C.c_void_p, C.c_int, C.POINTER(StatusC), DP, DP, DP, C.c_void_p]
    L.alore_backend_device_results.argtypes = [C.c_void_p, C.POINTER(DeviceView)]
    L.alore_backend_eval.argtypes = [C.c_void_p, C.c_int, C.c_int, DP, DP, DP, C.c_double, C.c_double, DP, DP, DP, C.c_void_p]
    L.alore_backend_lbfgs.argtypes = [C.c_void_p, C.c_int, C.c_int, DP, DP, DP, C.c_double, C.c_double, C.c_int, DP,
                                      C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), DP, C.c_void_p]
    L.alore_backend_last_plan_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.alore_backend_check_plans.argtypes = [C.c_void_p, C.c_int, DP, DP, C.c_double, C.c_int, C.POINTER(CheckC), C.c_void_p]
    L.alore_backend_device_check.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.alore_front_end_default_params.argtypes = [C.POINTER(FrontEndParamsC)]
    L.alore_front_end_default_params.restype = None
    L.alore_backend_set_paths.argtypes = [C.c_void_p, C.c_int, C.POINTER(PathsC), C.POINTER(FrontEndParamsC), C.c_int, C.c_void_p, C.c_int,
                                          C.c_void_p]
    L.alore_backend_device_build_status.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.alore_backend_build_status.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.alore_backend_launch_order.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.alore_backend_get_problems.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), DP, DP, DP, DP, DP, DP, DP, C.POINTER(C.c_int)]
    L.alore_backend_predicted_state_device.argtypes = [C.c_void_p, C.c_int, C.c_double] + [C.c_void_p] * 8
    L.alore_backend_plan_masked.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.alore_backend_replan_mask.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.alore_backend_map_default_params.argtypes = [C.POINTER(MapParamsC)]
    L.alore_backend_map_default_params.restype = None
    L.alore_backend_map_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.POINTER(MapParamsC)]
    L.alore_backend_map_logodds.argtypes = [C.c_void_p, DP]
    L.alore_backend_map_set_grid.argtypes = [C.c_void_p, C.POINTER(C.c_ubyte)]
    L.alore_backend_map_integrate.argtypes = [C.c_void_p, C.c_int, C.POINTER(ScanC), C.c_int, C.c_int, C.c_void_p]
    L.alore_backend_map_update_esdf.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p]
    L.alore_backend_map_get.argtypes = [C.c_void_p, C.POINTER(C.c_ubyte), DP, DP]
    L.alore_backend_map_device.argtypes = [C.c_void_p, C.POINTER(MapViewC)]
    L.alore_backend_laser_default_params.argtypes = [C.POINTER(LaserParamsC)]
    L.alore_backend_laser_default_params.restype = None
    L.alore_backend_laser_create.argtypes = [C.c_void_p, C.POINTER(LaserParamsC), C.c_int, C.c_int]
    L.alore_backend_laser_set_cloud.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.alore_backend_laser_scan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.alore_backend_device_laser.argtypes = [C.c_void_p, C.POINTER(LaserViewC)]
    L.alore_backend_get_laser.argtypes = [C.c_void_p, C.c_int, DP] + [C.POINTER(C.c_float)] * 2 + [C.POINTER(C.c_int), C.POINTER(C.c_float)] + \
        [C.POINTER(C.c_int)] * 2
    L.alore_backend_search_default_params.argtypes = [C.POINTER(SearchParamsC)]
    L.alore_backend_search_default_params.restype = None
    L.alore_backend_search_paths.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(SearchParamsC), C.c_int,
                                             C.c_void_p, C.c_int, C.c_void_p]
    L.alore_backend_device_paths.argtypes = [C.c_void_p, C.POINTER(PathsC)]
    L.alore_backend_device_search_status.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.alore_backend_search_status.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.alore_backend_search_sweeps.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.alore_backend_search_reserve.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.alore_backend_search_reserved.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.alore_backend_search_wide_ticks.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]
    L.alore_backend_get_paths.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), DP, C.POINTER(C.c_int)]
    L.alore_backend_task_default_params.argtypes = [C.POINTER(TaskParamsC)]
    L.alore_backend_task_default_params.restype = None
    L.alore_backend_task_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(TaskParamsC),
                                          C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.alore_backend_device_task.argtypes = [C.c_void_p, C.POINTER(TaskViewC)]
    L.alore_backend_get_task.argtypes = [C.c_void_p, C.c_int] + [C.POINTER(C.c_int)] * 5 + [DP, DP] + [C.POINTER(C.c_int)] * 2
    L.alore_backend_task_reorder.argtypes = [C.c_void_p, C.c_void_p]
    L.alore_backend_task_reserve.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.alore_backend_task_reserved.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.alore_backend_task_wide_ticks.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]
    L.alore_backend_device_task_assign.argtypes = [C.c_void_p, C.POINTER(TaskAssignViewC)]
    L.alore_backend_get_task_assign.argtypes = [C.c_void_p, C.c_int] + [C.POINTER(C.c_int)] * 2
    L.alore_backend_map_paint.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.alore_backend_device_paint_counters.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.alore_backend_map_paint_counters.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.alore_backend_mission_default_params.argtypes = [C.POINTER(MissionParamsC)]
    L.alore_backend_mission_default_params.restype = None
    L.alore_backend_mission_create.argtypes = [C.c_void_p, C.POINTER(MissionParamsC)]
    L.alore_backend_mission_set.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                            C.c_int, C.c_void_p]
    L.alore_backend_mission_set_goals.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.alore_backend_mission_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.alore_backend_device_mission.argtypes = [C.c_void_p, C.POINTER(MissionViewC)]
    L.alore_backend_get_mission.argtypes = [C.c_void_p, C.c_int] + [C.POINTER(C.c_int)] * 5 + [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.alore_backend_manager_default_params.argtypes = [C.POINTER(ManagerParamsC)]
    L.alore_backend_manager_default_params.restype = None
    L.alore_backend_manager_create.argtypes = [C.c_void_p, C.POINTER(ManagerParamsC)]
    L.alore_backend_manager_request.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.alore_backend_manager_begin.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.alore_backend_manager_starts.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
    L.alore_backend_manager_end.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
    L.alore_backend_manager_next_legs.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.alore_backend_device_manager.argtypes = [C.c_void_p, C.POINTER(ManagerViewC)]
    L.alore_backend_get_manager.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), DP, C.POINTER(C.c_int)]
    L._backend_bound = True


class BackendError(RuntimeError):
    pass


def default_config() -> BackendConfig:
    L = _lib.load()
    _bind(L)
    c = BackendConfig()
    L.alore_backend_default_config(C.byref(c))
    return c


def default_map_params() -> MapParamsC:
    """mapsim.yaml and planner_sim.launch: 0.99, 0.35, 0.12, 0.90, 0.80, range 27 m, perspective mode"""
    L = _lib.load()
    _bind(L)
    p = MapParamsC()
    L.alore_backend_map_default_params(C.byref(p))
    return p


def default_mission_params() -> MissionParamsC:
    """plan_manager.hpp: item squares of half 0.5, freed with half 0.5 within 2.0 m, targets locked with half 0.3 within 0.5 m, a
    target just left locked with half 0.2 within 0.3 m"""
    L = _lib.load()
    _bind(L)
    p = MissionParamsC()
    L.alore_backend_mission_default_params(C.byref(p))
    return p


def default_manager_params() -> ManagerParamsC:
    """planner_sim.launch: replan_time 5000, max_replan_time 0.05; periodic replans, no collision stop, no stop flag without a path"""
    L = _lib.load()
    _bind(L)
    p = ManagerParamsC()
    L.alore_backend_manager_default_params(C.byref(p))
    return p


def default_laser_params() -> LaserParamsC:
    """planner_sim.launch and perspective_laser.yaml: horizon 27 m, resolution 0.1 m, 360 x 16 lines over 30 degrees, no horizontal
    limit, no filter, perspective mode"""
    L = _lib.load()
    _bind(L)
    p = LaserParamsC()
    L.alore_backend_laser_default_params(C.byref(p))
    return p


class _DeviceArray:
    """a device allocation of the library as torch.as_tensor reads it"""

    def __init__(self, address, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(address), False), "version": 2}


def default_search_params() -> SearchParamsC:
    """jps_safe_dis of jps3ms.yaml (0.3) and a window margin of 3 m"""
    L = _lib.load()
    _bind(L)
    p = SearchParamsC()
    L.alore_backend_search_default_params(C.byref(p))
    return p


def _search_params(safe_dis, window_margin) -> SearchParamsC:
    p = default_search_params()
    if safe_dis is not None:
        p.safe_dis = float(safe_dis)
    if window_margin is not None:
        p.window_margin = float(window_margin)
    return p


def default_task_params() -> TaskParamsC:
    """jps_safe_dis 0.3, a window margin of 3 m and the greedy order, the reference's live call"""
    L = _lib.load()
    _bind(L)
    p = TaskParamsC()
    L.alore_backend_task_default_params(C.byref(p))
    return p


def _task_params(safe_dis, window_margin, mode) -> TaskParamsC:
    p = default_task_params()
    if safe_dis is not None:
        p.safe_dis = float(safe_dis)
    if window_margin is not None:
        p.window_margin = float(window_margin)
    if mode is not None:
        p.mode = int(mode)
    return p


def _dp(a):
    return a.ctypes.data_as(DP) if a is not None else None


def _front_end_params(params) -> FrontEndParamsC:
    """flat_traj.FrontEndParams (or anything with its fields; None: the defaults) as the C struct"""
    c = FrontEndParamsC()
    if params is None:
        L = _lib.load()
        _bind(L)
        L.alore_front_end_default_params(C.byref(c))
    else:
        for name, _ in FrontEndParamsC._fields_:
            setattr(c, name, getattr(params, name))
    return c


def _dev(a):
    """device address of a torch tensor, or the address itself (int / None)"""
    if a is None or isinstance(a, int):
        return a
    return int(a.data_ptr())


def _stream(s):
    """hipStream_t of a torch stream, or the handle itself (int / None = the default stream)"""
    if s is None or isinstance(s, int):
        return s
    return int(s.cuda_stream)


def _mask(mask, stride):
    """(address, stride in bytes) of a device mask: a torch int32 tensor (its own stride), an address with `stride`, or a pair"""
    if mask is None:
        return None, 0
    if isinstance(mask, tuple):
        return int(mask[0]), int(mask[1])
    if isinstance(mask, int):
        return mask, int(stride)
    return int(mask.data_ptr()), int(mask.stride(0) * mask.element_size()) if mask.dim() else 4


class BatchedMSPlanner:
    """MSPlanner for a batch.  ``max_pieces``: the longest trajectory (pieces) the handle accepts (<= 64: the handle
    takes the 16-, 32- or 64-piece build of the optimiser, ``self.P``; 64 pieces are a route of about 50 m at the default front end)."""

    def __init__(self, max_problems: int, max_pieces: int = 16, config: BackendConfig | None = None, device: int = 0):
        self.L = _lib.load()
        _bind(self.L)
        self.cfg = config or default_config()
        self.h = C.c_void_p()
        rc = self.L.alore_backend_create(C.byref(self.cfg), device, max_pieces, max_problems, C.byref(self.h))
        if rc != 0:
            raise BackendError(f"alore_backend_create failed ({rc}): no GPU, or unsupported configuration; there is no CPU path")
        self.P = 16 if max_pieces <= 16 else 32 if max_pieces <= 32 else 64
        self.B = max_problems
        self.count = 0
        self._keep = None
        self.n_classes = 0
        self._class_fe = False

    # ---- object classes: one robot model per problem slot (alore_backend_set_classes)
    def set_classes(self, configs, front_end=None):
        """The class table: a list of BackendConfig (whole configs), and optionally the front-end parameters per class
        (flat_traj.FrontEndParams or FrontEndParamsC) that set_paths(params=None) then builds every slot with.  An empty list
        removes the table.  Waits for the device."""
        configs = list(configs)
        n = len(configs)
        arr = (BackendConfig * max(n, 1))()
        for k, c in enumerate(configs):
            C.memmove(C.byref(arr[k]), C.byref(c), C.sizeof(BackendConfig))
        fe = None
        if front_end is not None and n:
            if len(front_end) != n:
                raise BackendError("set_classes: front_end needs an entry per class")
            fe = (FrontEndParamsC * n)()
            for k, p in enumerate(front_end):
                q = _front_end_params(p)
                C.memmove(C.byref(fe[k]), C.byref(q), C.sizeof(FrontEndParamsC))
        self._check(self.L.alore_backend_set_classes(self.h, n, arr if n else None, fe))
        self.n_classes = n
        self._class_fe = fe is not None

    def set_problem_classes(self, class_of, count: int | None = None, stream=None):
        """The class of slots 0..count-1: a NumPy array / list (checked on the host: an index outside the table raises and
        changes nothing; waits for the stream) or an int32 device tensor (read in stream order, clamped into the table by the
        kernel, nothing waits: class_view().clamped counts what it clamped)."""
        if hasattr(class_of, "data_ptr"):
            if not (class_of.is_cuda and str(class_of.dtype) == "torch.int32" and class_of.dim() == 1 and class_of.is_contiguous()):
                raise BackendError("set_problem_classes: a contiguous int32 device tensor with a word per slot")
            n = int(count or class_of.numel())
            self._check(self.L.alore_backend_set_problem_classes(self.h, n, int(class_of.data_ptr()), 1, _stream(stream)))
            return
        k = np.ascontiguousarray(class_of, np.int32).reshape(-1)
        self._check(self.L.alore_backend_set_problem_classes(self.h, int(count or k.size), k.ctypes.data, 0, _stream(stream)))

    def class_view(self) -> ClassViewC:
        v = ClassViewC()
        self._check(self.L.alore_backend_device_classes(self.h, C.byref(v)))
        return v

    def class_xv(self):
        """float64 device tensor [max_problems] over the view's xv: the effective ICR offset of every slot, what
        BatchedNmpc.refs_set_from_backend takes for `xv`"""
        import torch
        return torch.as_tensor(_DeviceArray(self.class_view().xv, (self.B,), "<f8"), device="cuda")

    def class_state(self, count: int | None = None) -> dict:
        """class_of, xv [count] and the clamped counter copied to the host (waits)"""
        import torch
        n, v = int(count or self.count or self.B), self.class_view()
        torch.cuda.synchronize()
        return {"n_classes": v.n_classes,
                "class_of": torch.as_tensor(_DeviceArray(v.class_of, (n,), "<i4"), device="cuda").cpu().numpy(),
                "xv": torch.as_tensor(_DeviceArray(v.xv, (n,), "<f8"), device="cuda").cpu().numpy(),
                "clamped": int(torch.as_tensor(_DeviceArray(v.clamped, (1,), "<i4"), device="cuda").cpu()[0])}

    def class_stats(self, fetch: bool = True, count: int | None = None, stream=None):
        """Per class, the outcome of slots 0..count-1 of the last plan launch, reduced on the device: a CLASS_STAT_DTYPE array
        [max(n_classes, 1)].  fetch=False: the records stay in the slab of class_view().stats and nothing waits."""
        n = int(count or self.count)
        if not fetch:
            self._check(self.L.alore_backend_class_stats(self.h, n, None, _stream(stream)))
            return None
        rec = np.zeros(max(self.n_classes, 1), CLASS_STAT_DTYPE)
        self._check(self.L.alore_backend_class_stats(self.h, n, rec.ctypes.data_as(C.POINTER(ClassStatC)), _stream(stream)))
        return rec

    def _fe_arg(self, params):
        """the fe argument of alore_backend_set_paths: NULL when the class table carries front-end parameters and none are given"""
        if params is None and self._class_fe:
            return None
        return C.byref(_front_end_params(params))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.alore_backend_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise BackendError(f"alore_backend error {rc}: {self.L.alore_backend_last_error(self.h).decode()}")

    # plan_env::SDFmap: dist[ix, iy] double grid, cell centres at (i + 0.5) res + lo
    def set_map(self, dist: np.ndarray, x_lo: float, y_lo: float, res: float):
        dist = np.ascontiguousarray(dist, dtype=np.float64)
        self._check(self.L.alore_backend_set_map(self.h, _dp(dist), dist.shape[0], dist.shape[1], x_lo, y_lo, res))
        self.map_res = float(res)

    def build_esdf(self, grid: np.ndarray, x_lo: float, y_lo: float, res: float, odom=(0.0, 0.0), detection_range: float = 1e3) -> np.ndarray:
        """SDFmap::updateESDF2d on the device from a uint8 state grid (0 unknown, 1 free, 2 occupied); the result becomes
        the planner's map and is returned."""
        g = np.ascontiguousarray(grid, dtype=np.uint8)
        dist = np.zeros(g.shape)
        self._check(self.L.alore_backend_build_esdf(self.h, g.ctypes.data_as(C.POINTER(C.c_ubyte)), g.shape[0], g.shape[1], x_lo, y_lo, res,
                                                    float(odom[0]), float(odom[1]), float(detection_range), _dp(dist)))
        self.map_res = float(res)
        return dist

    # ---- the resident occupancy map: point clouds in, log-odds, cell states and the ESDF updated in place on the device
    def map_create(self, nx: int, ny: int, x_lo: float, y_lo: float, res: float, params: MapParamsC | None = None, **fields):
        """plan_env::SDFmap on the device: all cells unknown, log-odds at clamp_min - 0.01, distances DBL_MAX.  params: a
        MapParamsC (None: the defaults), fields: single members to change (detection_range=2.0, perspective=0, ...).  The map
        becomes the planner's map; set_map / build_esdf end it."""
        p = MapParamsC()
        if params is None:
            self.L.alore_backend_map_default_params(C.byref(p))
        else:
            C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
        for k, v in fields.items():
            if k not in dict(MapParamsC._fields_):
                raise TypeError(f"alore_backend_map_params has no field {k}")
            setattr(p, k, v)
        self._check(self.L.alore_backend_map_create(self.h, int(nx), int(ny), float(x_lo), float(y_lo), float(res), C.byref(p)))
        self.map_shape = (int(nx), int(ny))
        self.map_res = float(res)
        self.map_params = p

    @property
    def map_logodds(self) -> np.ndarray:
        """logit of p_hit, p_miss, p_min, p_max, p_occ as the library computed them"""
        out = np.zeros(5)
        self._check(self.L.alore_backend_map_logodds(self.h, _dp(out)))
        return out

    def map_set_grid(self, grid: np.ndarray):
        """seeds the cell states from a prior map ([nx][ny] of 0 unknown, 1 unoccupied, 2 occupied); waits"""
        g = np.ascontiguousarray(grid, dtype=np.uint8)
        if g.shape != getattr(self, "map_shape", None):
            raise BackendError(f"map_set_grid: the grid must have the map's shape {getattr(self, 'map_shape', None)}")
        self._check(self.L.alore_backend_map_set_grid(self.h, g.ctypes.data_as(C.POINTER(C.c_ubyte))))

    def map_integrate(self, scans, update_esdf: bool = True, stream=None, point_stride_bytes: int | None = None):
        """One updateOccupancyCallback per scan, in order, each followed (update_esdf) by updateESDF2d in its window.  scans: a list
        of (points, odom) with odom = (x, y[, yaw]) in host values and points either NumPy [n][k >= 2] (x, y first; converted to
        float32; uploaded, the call waits) or, for all scans, torch float32 device tensors [n][k] / raw device addresses given as
        (address, n_points) (read in place in stream order, nothing waits).  point_stride_bytes: bytes between points for raw
        addresses (default: the row stride of the array or tensor)."""
        n = len(scans)
        arr = (ScanC * max(n, 1))()
        keep, device = [], None
        for k, (pts, odom) in enumerate(scans):
            a = arr[k]
            if isinstance(pts, tuple):
                dev, a.points, a.n_points, a.point_stride_bytes = True, int(pts[0]) or None, int(pts[1]), int(point_stride_bytes or 8)
            elif isinstance(pts, np.ndarray) or not hasattr(pts, "data_ptr"):
                q = np.asarray(pts, np.float32)
                q = np.ascontiguousarray(q.reshape(len(q), -1)) if q.size else np.zeros((0, 2), np.float32)
                keep.append(q)
                dev, a.points, a.n_points, a.point_stride_bytes = False, q.ctypes.data if q.size else None, q.shape[0], max(q.shape[1], 2) * 4
            else:
                if str(pts.dtype) != "torch.float32" or pts.dim() != 2 or pts.stride(1) != 1:
                    raise BackendError("map_integrate: device points must be a float32 tensor [n][k >= 2] with unit stride along k")
                keep.append(pts)
                dev, a.points, a.n_points = True, int(pts.data_ptr()) if pts.shape[0] else None, int(pts.shape[0])
                a.point_stride_bytes = int(point_stride_bytes or pts.stride(0) * 4)
            if device is not None and dev != device:
                raise BackendError("map_integrate: the scans of one call are all host arrays or all device tensors")
            device = dev
            a.odom[0], a.odom[1], a.odom[2] = float(odom[0]), float(odom[1]), float(odom[2]) if len(odom) > 2 else 0.0
        self._check(self.L.alore_backend_map_integrate(self.h, n, arr, int(bool(device)), int(bool(update_esdf)), _stream(stream)))

    def map_update_esdf(self, odom, detection_range: float | None = None, stream=None):
        """updateESDF2d alone in the window odom +- detection_range (None: the map's own); asynchronous"""
        r = self.map_params.detection_range if detection_range is None else float(detection_range)
        self._check(self.L.alore_backend_map_update_esdf(self.h, float(odom[0]), float(odom[1]), r, _stream(stream)))

    def map_state(self) -> dict:
        """the resident map copied to the host (waits): grid uint8 [nx][ny], log_odds and dist float64 [nx][ny]"""
        shape = getattr(self, "map_shape", (0, 0))
        grid, lo, dist = np.zeros(shape, np.uint8), np.zeros(shape), np.zeros(shape)
        self._check(self.L.alore_backend_map_get(self.h, grid.ctypes.data_as(C.POINTER(C.c_ubyte)), _dp(lo), _dp(dist)))
        return {"grid": grid, "log_odds": lo, "dist": dist}

    def map_device(self) -> MapViewC:
        v = MapViewC()
        self._check(self.L.alore_backend_map_device(self.h, C.byref(v)))
        return v

    # ---- the edits of missions in the resident map: item and target footprints
    def map_paint(self, edits, stream=None) -> dict:
        """paintSquare / paintBox / ... for a host list, as if one edit after the other.  edits: an EDIT_DTYPE array, or rows
        (cx, cy, hx, hy, make_obs).  The list is uploaded and the call waits; returns the counters (paint_counters)."""
        if isinstance(edits, np.ndarray) and edits.dtype == EDIT_DTYPE:
            e = np.ascontiguousarray(edits)
        else:
            rows = np.asarray(edits, np.float64).reshape(-1, 5)
            e = np.zeros(len(rows), EDIT_DTYPE)
            for k, name in enumerate(("cx", "cy", "hx", "hy")):
                e[name] = rows[:, k]
            e["make_obs"] = rows[:, 4] != 0
        self._check(self.L.alore_backend_map_paint(self.h, e.ctypes.data if len(e) else None, len(e), None, 0, _stream(stream)))
        return self.paint_counters()

    def map_paint_device(self, edits, d_count, capacity: int | None = None, stream=None):
        """the same for a list in DEVICE memory (a torch tensor or an address) of `capacity` entries of 40 bytes whose length is the
        device int at d_count; nothing waits, the counters stay on the device (paint_counters fetches them)"""
        if capacity is None:
            capacity = int(edits.numel() * edits.element_size() // C.sizeof(MapEditC))
        self._check(self.L.alore_backend_map_paint(self.h, _dev(edits), int(capacity), _dev(d_count), 1, _stream(stream)))

    def paint_counters(self) -> dict:
        """n_changed, box (min_x, min_y, max_x, max_y) and n_skipped of the last paint; waits"""
        out = (C.c_int * 6)()
        self._check(self.L.alore_backend_map_paint_counters(self.h, out))
        return {"n_changed": out[0], "box": (out[1], out[2], out[3], out[4]), "n_skipped": out[5]}

    def mission_create(self, params: MissionParamsC | None = None, **fields):
        """the slab of max_problems missions on the resident map; fields: single parameters to change (item_half=0.3, ...)"""
        p = default_mission_params()
        if params is not None:
            C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
        for k, v in fields.items():
            if k not in dict(MissionParamsC._fields_):
                raise TypeError(f"alore_backend_mission_params has no field {k}")
            setattr(p, k, v)
        self._check(self.L.alore_backend_mission_create(self.h, C.byref(p)))
        self.mission_params = p

    def mission_set(self, n_tasks, points, kinds=None, mask=None, stream=None):
        """items and targets of missions 0..count-1 from host rows [count][1 + 2 T][2] (the layout of task_plan; point 0 is
        ignored), then "items -> OBS" in the map.  kinds: [count][T] of ITEM_*; mask: [count] ints.  Waits."""
        n = np.ascontiguousarray(n_tasks, np.int32)
        p = np.ascontiguousarray(points, np.float64)
        count, T = len(n), (p.shape[1] - 1) // 2
        k = None if kinds is None else np.ascontiguousarray(kinds, np.int32).reshape(count, T)
        m = None if mask is None else np.ascontiguousarray(mask, np.int32)
        self._check(self.L.alore_backend_mission_set(self.h, count, T, n.ctypes.data, p.ctypes.data, p.shape[1] * 16, None if k is None else k.ctypes.data,
                                                     0, None if m is None else m.ctypes.data, 4, _stream(stream)))

    def mission_set_device(self, count, max_tasks, n_tasks, points, point_row_stride=None, kinds=None, mask=None, mask_stride: int = 4, stream=None):
        """mission_set on DEVICE memory (torch tensors or addresses) in stream order; nothing waits"""
        ma, ms = _mask(mask, mask_stride)
        self._check(self.L.alore_backend_mission_set(self.h, int(count), int(max_tasks), _dev(n_tasks), _dev(points),
                                                     int(point_row_stride or 16 * (1 + 2 * max_tasks)), _dev(kinds), 1, ma, ms, _stream(stream)))

    def mission_set_goals(self, goal_xy, mask=None, stride=None, mask_stride: int = 4, stream=None, count=None):
        """the goal classification at a plan start.  goal_xy: a host array [count][>= 2] (waits) or, with count, a device tensor or
        address read with `stride` bytes between goals in stream order"""
        if count is None:
            g = np.ascontiguousarray(goal_xy, np.float64)
            m = None if mask is None else np.ascontiguousarray(mask, np.int32)
            self._check(self.L.alore_backend_mission_set_goals(self.h, len(g), g.ctypes.data, g.shape[1] * 8, 0, None if m is None else m.ctypes.data, 4,
                                                               _stream(stream)))
        else:
            ma, ms = _mask(mask, mask_stride)
            self._check(self.L.alore_backend_mission_set_goals(self.h, int(count), _dev(goal_xy), int(stride or 16), 1, ma, ms, _stream(stream)))

    def mission_step(self, poses, after_plan_mask=None, stride=None, mask_stride: int = 4, stream=None, count=None, esdf_odom=None,
                     esdf_range: float | None = None):
        """one tick of MapUpdateThread plus the post-plan rule, painted in the same call.  poses: a host array [count][>= 2] (waits)
        or, with count, a device tensor or address with `stride` bytes between poses (nothing waits).  esdf_odom: enqueue
        map_update_esdf behind it on the same stream, in the window esdf_odom +- esdf_range (None: the map's own)."""
        if count is None:
            p = np.ascontiguousarray(poses, np.float64)
            m = None if after_plan_mask is None else np.ascontiguousarray(after_plan_mask, np.int32)
            self._check(self.L.alore_backend_mission_step(self.h, len(p), p.ctypes.data, p.shape[1] * 8, 0, None if m is None else m.ctypes.data, 4,
                                                          _stream(stream)))
        else:
            ma, ms = _mask(after_plan_mask, mask_stride)
            self._check(self.L.alore_backend_mission_step(self.h, int(count), _dev(poses), int(stride or 16), 1, ma, ms, _stream(stream)))
        if esdf_odom is not None:
            self.map_update_esdf(esdf_odom, esdf_range, stream=stream)

    def device_mission(self) -> MissionViewC:
        v = MissionViewC()
        self._check(self.L.alore_backend_device_mission(self.h, C.byref(v)))
        return v

    def mission_state(self, count: int | None = None) -> dict:
        """status, phase, goal_item, goal_target, goal_status [count], the edit list of the last mission_set / mission_step (an
        EDIT_DTYPE array) and the counters of the last paint; waits"""
        n = self.B if count is None else int(count)
        ints = {k: np.zeros(n, np.int32) for k in ("status", "phase", "goal_item", "goal_target", "goal_status")}
        edits, ne, cnt = np.zeros(self.B * TASK_MAX_TASKS, EDIT_DTYPE), C.c_int(0), (C.c_int * 6)()
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        self._check(self.L.alore_backend_get_mission(self.h, n, ip(ints["status"]), ip(ints["phase"]), ip(ints["goal_item"]), ip(ints["goal_target"]),
                                                     ip(ints["goal_status"]), edits.ctypes.data, C.byref(ne), cnt))
        return dict(ints, edits=edits[:ne.value].copy(), n_changed=cnt[0], box=(cnt[1], cnt[2], cnt[3], cnt[4]), n_skipped=cnt[5])

    # ---- plan_manager's state machine for the fleet (csrc/fleet_manager.h)
    def manager_create(self, params: ManagerParamsC | None = None, **fields):
        """the slab of max_problems robots, all IDLE; fields: single parameters to change (replan_time=1.0, ...).  A second call only
        replaces the parameters."""
        p = default_manager_params()
        if params is not None:
            C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
        for k, v in fields.items():
            if k not in dict(ManagerParamsC._fields_):
                raise TypeError(f"alore_backend_manager_params has no field {k}")
            setattr(p, k, v)
        self._check(self.L.alore_backend_manager_create(self.h, C.byref(p)))
        self.manager_params = p

    def manager_request(self, start_xytheta=None, goal_xytheta=None, mask=None, stride=None, mask_stride: int = 4, stream=None, count=None):
        """start_callback / goal_callback.  Host arrays [count][3] (waits) or, with count, device tensors or addresses read with
        `stride` bytes between robots in stream order.  Either may be None."""
        if count is None:
            s = None if start_xytheta is None else np.ascontiguousarray(start_xytheta, np.float64).reshape(-1, 3)
            g = None if goal_xytheta is None else np.ascontiguousarray(goal_xytheta, np.float64).reshape(-1, 3)
            m = None if mask is None else np.ascontiguousarray(mask, np.int32)
            n = len(s if s is not None else g) if (s is not None or g is not None) else 0
            self._check(self.L.alore_backend_manager_request(self.h, n, None if s is None else s.ctypes.data, None if g is None else g.ctypes.data, 24, 0,
                                                             None if m is None else m.ctypes.data, 4, _stream(stream)))
        else:
            ma, ms = _mask(mask, mask_stride)
            self._check(self.L.alore_backend_manager_request(self.h, int(count), _dev(start_xytheta), _dev(goal_xytheta), int(stride or 24), 1, ma, ms,
                                                             _stream(stream)))

    def manager_begin(self, now: float, poses, collision_mask=None, stride=None, mask_stride: int = 4, stream=None, count=None):
        """the head of MainThread at `now`.  poses: a host array [count][>= 2] (waits) or, with count, a device tensor or address with
        `stride` bytes between poses (nothing waits); collision_mask: who may replan under replan_on_collision_only"""
        if count is None:
            p = np.ascontiguousarray(poses, np.float64)
            m = None if collision_mask is None else np.ascontiguousarray(collision_mask, np.int32)
            self._check(self.L.alore_backend_manager_begin(self.h, len(p), float(now), p.ctypes.data, p.shape[1] * 8, None if m is None else m.ctypes.data, 4,
                                                           0, _stream(stream)))
        else:
            ma, ms = _mask(collision_mask, mask_stride)
            self._check(self.L.alore_backend_manager_begin(self.h, int(count), float(now), _dev(poses), int(stride or 16), ma, ms, 1, _stream(stream)))

    def manager_starts(self, count, xytheta, vaj, oaj, start_yaw=None, end_yaw=None, stream=None):
        """behind predicted_state_device, on its DEVICE outputs: start states of FRESH robots in, predicted poses of REPLAN robots
        out, start_yaw / end_yaw for set_paths_device"""
        self._check(self.L.alore_backend_manager_starts(self.h, int(count), _dev(xytheta), _dev(vaj), _dev(oaj), _dev(start_yaw), _dev(end_yaw),
                                                        _stream(stream)))

    def manager_end(self, count=None, search_status=None, build_status=None, plan_ok=None, T=None, n_pieces=None, stream=None):
        """the rest of MainThread with the `now` of the matching manager_begin; each array: None (the handle's own slab) or DEVICE
        memory of the same layout (T: [count][self.P])"""
        self._check(self.L.alore_backend_manager_end(self.h, int(count or self.B), _dev(search_status), _dev(build_status), _dev(plan_ok), _dev(T),
                                                     _dev(n_pieces), _stream(stream)))

    def manager_next_legs(self, count, poses, leg_yaw, stride=None, reset_legs: bool = False, stream=None):
        """the next leg of its mission (the slab of task_plan) for every robot that is IDLE without a goal; DEVICE memory: poses
        (x, y, yaw, `stride` bytes apart) and leg_yaw [count][TASK_MAX_LEGS]"""
        self._check(self.L.alore_backend_manager_next_legs(self.h, int(count), _dev(poses), int(stride or 24), _dev(leg_yaw), int(bool(reset_legs)),
                                                           _stream(stream)))

    def manager_view(self) -> ManagerViewC:
        v = ManagerViewC()
        self._check(self.L.alore_backend_device_manager(self.h, C.byref(v)))
        return v

    def manager_mask(self, name: str):
        """(address, stride) of plan_mask, fresh_mask, replan_mask, stop_mask or after_plan_mask, for the mask arguments"""
        return int(getattr(self.manager_view(), name)), 4

    def get_manager(self, count: int | None = None) -> dict:
        """the slab copied to the host (waits): the int rows [count], goal / start / plan_start_xytheta [count][3], the times
        [count], `counters` (a dict), and the raw blocks `ints` [11][count] and `doubles` [14][count]"""
        n = self.B if count is None else int(count)
        ints, dbl, cnt = np.zeros((len(MANAGER_INT_ROWS), n), np.int32), np.zeros((14, n)), np.zeros(8, np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        self._check(self.L.alore_backend_get_manager(self.h, n, ip(ints), _dp(dbl), ip(cnt)))
        out = dict(zip(MANAGER_INT_ROWS, ints), ints=ints, doubles=dbl, counters=dict(zip(MANAGER_COUNTERS, cnt.tolist())))
        out.update(goal=dbl[0:3].T.copy(), start=dbl[3:6].T.copy(), plan_start_xytheta=dbl[6:9].T.copy())
        out.update(zip(MANAGER_DOUBLE_ROWS[3:], dbl[9:]))
        return out

    def predicted_state(self, times, resolution: float = 0.01, start_times=None, start_xytheta=None):
        """MSPlanner::get_the_predicted_state[_and_path] for the plans of the last launch"""
        t = np.ascontiguousarray(times, np.float64)
        n = t.shape[0]
        st = None if start_times is None else np.ascontiguousarray(start_times, np.float64)
        sx = None if start_xytheta is None else np.ascontiguousarray(start_xytheta, np.float64)
        xyt, vaj, oaj, fwd = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, np.int32)
        self._check(self.L.alore_backend_predicted_state(self.h, n, float(resolution), _dp(st), _dp(t), _dp(sx), _dp(xyt), _dp(vaj), _dp(oaj),
                                                         fwd.ctypes.data_as(C.POINTER(C.c_int))))
        return {"xytheta": xyt, "vaj": vaj, "oaj": oaj, "forward": fwd.astype(bool)}

    def path_points(self, panels_per_piece: int = 3, count: int | None = None):
        """MSPlanner::mincoPointPub for the plans of the last launch: list of (points [n][2], yaw [n_pieces panels]) per plan"""
        n = int(count or self.count)
        per = self.P * (panels_per_piece + 1)
        xy = np.zeros((n, per, 2)); yaw = np.zeros((n, self.P * panels_per_piece)); npts = np.zeros(n, np.int32)
        self._check(self.L.alore_backend_path_points(self.h, n, int(panels_per_piece), _dp(xy), _dp(yaw), npts.ctypes.data_as(C.POINTER(C.c_int))))
        return [(xy[b, :npts[b]].copy(), yaw[b, :(npts[b] // (panels_per_piece + 1)) * panels_per_piece].copy()) for b in range(n)]

    def path_points_device(self, xy, n_points, yaw=None, panels_per_piece: int = 3, count: int | None = None, stream=None):
        """The same on the caller's device tensors in stream order, nothing waits: xy float64 [count][P (panels_per_piece + 1)][2],
        n_points int32 [count], yaw float64 [count][P panels_per_piece] or None.  A row is written up to its n_points only.  xy and
        n_points are what BatchedTaskFsm.set_paths takes"""
        n = int(count or self.count)
        per = self.P * (int(panels_per_piece) + 1)
        if xy.element_size() != 8 or not xy.is_contiguous() or xy.numel() < n * per * 2:
            raise ValueError(f"xy: a contiguous float64 device tensor of at least [{n}][{per}][2] is needed")
        if n_points.element_size() != 4 or not n_points.is_contiguous() or n_points.numel() < n:
            raise ValueError("n_points: a contiguous int32 device tensor [count] is needed")
        if yaw is not None and (yaw.element_size() != 8 or not yaw.is_contiguous() or yaw.numel() < n * self.P * int(panels_per_piece)):
            raise ValueError("yaw: a contiguous float64 device tensor [count][P panels_per_piece] is needed")
        s = None if stream is None else (stream if isinstance(stream, int) else int(stream.cuda_stream))
        self._check(self.L.alore_backend_path_points_device(self.h, n, int(panels_per_piece), int(xy.data_ptr()),
                                                            None if yaw is None else int(yaw.data_ptr()), int(n_points.data_ptr()), s))

    def check_plans(self, t_from=None, t_to=None, min_safe_dis=None, body=False, count=None, stream=None, fetch=True) -> dict | None:
        """The final collision check of the plans of the last launch against the map as it is NOW (set_map / build_esdf since
        then): per plan, over the panels whose time interval overlaps (t_from[b], t_to[b]) (None: from 0 / to the end), whether
        one is closer than min_safe_dis (None: the configured final_min_safe_dis) and where the first one is.  body: the
        minimum over the reference point and the configured body check points instead of the reference point alone.
        fetch=False: the records stay in the device slab (device_check / check_mask), nothing waits and nothing is returned."""
        n = self.count if count is None else int(count)
        m = max(n, 0)
        tf = None if t_from is None else np.ascontiguousarray(np.broadcast_to(np.asarray(t_from, np.float64), (m,)))
        tt = None if t_to is None else np.ascontiguousarray(np.broadcast_to(np.asarray(t_to, np.float64), (m,)))
        rec = np.zeros(m, CHECK_DTYPE)
        self._check(self.L.alore_backend_check_plans(self.h, n, _dp(tf), _dp(tt), 0.0 if min_safe_dis is None else float(min_safe_dis),
                                                     int(bool(body)), rec.ctypes.data_as(C.POINTER(CheckC)) if fetch else None, _stream(stream)))
        if not fetch:
            return None
        return {k: rec[k].copy() for k in ("collision", "first_panel", "n_checked", "first_time", "first_xy", "min_dist")}

    def device_check(self) -> int:
        """device address of the records of the last check_plans (alore_backend_check[max_problems], CHECK_DTYPE)"""
        p = C.c_void_p()
        self._check(self.L.alore_backend_device_check(self.h, C.byref(p)))
        return p.value

    def check_mask(self):
        """(address, stride) of the `collision` words of the check slab: the mask of set_paths_device / plan that names the plans
        the last check_plans flagged"""
        return self.device_check(), C.sizeof(CheckC)

    # ---- problems from way-point paths, built on the device (alore_backend_set_paths)
    def set_paths(self, paths_xy, start_yaw, end_yaw, start_vaj=None, start_oaj=None, params=None, mask=None):
        """FlatTrajData of way-point paths (a list of [n][2] arrays, or one [count][K][2] array with n_points given as a pair
        (xy, n_points)) into slots 0..count-1, and the launch order; NumPy in, padded to the longest path.  mask: per slot, 0 leaves
        the slot as it is.  Raises when a path does not build (build_status() says which)."""
        if isinstance(paths_xy, tuple):
            xy, npts = np.ascontiguousarray(paths_xy[0], np.float64), np.ascontiguousarray(paths_xy[1], np.int32)
        else:
            npts = np.array([len(p) for p in paths_xy], np.int32)
            K = int(min(max(int(npts.max()), 2), MAX_PATH_POINTS))
            xy = np.zeros((len(paths_xy), K, 2))
            for b, p in enumerate(paths_xy):
                q = np.asarray(p, np.float64).reshape(-1, 2)[:K]
                xy[b, :len(q)] = q
        n = len(npts)
        sy = np.ascontiguousarray(np.broadcast_to(np.asarray(start_yaw, np.float64), (n,)))
        ey = np.ascontiguousarray(np.broadcast_to(np.asarray(end_yaw, np.float64), (n,)))
        vaj = None if start_vaj is None else np.ascontiguousarray(np.broadcast_to(np.asarray(start_vaj, np.float64), (n, 3)))
        oaj = None if start_oaj is None else np.ascontiguousarray(np.broadcast_to(np.asarray(start_oaj, np.float64), (n, 3)))
        mk = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(bool), np.int32)
        pc = PathsC(xy.shape[1], npts.ctypes.data, xy.ctypes.data, sy.ctypes.data, ey.ctypes.data,
                    None if vaj is None else vaj.ctypes.data, None if oaj is None else oaj.ctypes.data)
        self.count = n  # the handle's count changes whether or not every path builds
        self._check(self.L.alore_backend_set_paths(self.h, n, C.byref(pc), self._fe_arg(params), 0, None if mk is None else mk.ctypes.data, 4, None))

    def set_paths_device(self, count, max_points, n_points, xy, start_yaw, end_yaw, start_vaj=None, start_oaj=None, params=None, mask=None,
                         mask_stride=4, stream=None):
        """The same with everything resident: torch tensors (int32 n_points [count], float64 xy [count][max_points][2], start_yaw /
        end_yaw [count], start_vaj / start_oaj [count][3]) or raw device addresses; mask as for plan().  Nothing is copied but the
        argument block and nothing waits; build_status() has the outcome per slot."""
        pc = PathsC(int(max_points), _dev(n_points), _dev(xy), _dev(start_yaw), _dev(end_yaw), _dev(start_vaj), _dev(start_oaj))
        mp, ms = _mask(mask, mask_stride)
        self._check(self.L.alore_backend_set_paths(self.h, int(count), C.byref(pc), self._fe_arg(params), 1, mp, ms, _stream(stream)))
        self.count = int(count)

    def build_status(self, count: int | None = None) -> np.ndarray:
        """per slot of the last set_paths[_device]: 0 built, 1 masked out, -1 bad point count, -2 too many pieces (waits)"""
        n = int(count or self.count)
        out = np.zeros(n, np.int32)
        self._check(self.L.alore_backend_build_status(self.h, n, out.ctypes.data_as(C.POINTER(C.c_int))))
        return out

    def launch_order(self, count: int | None = None) -> np.ndarray:
        """the launch order of the last set_problems / set_paths[_device]: most pieces first, stable in the slot index (waits)"""
        n = int(count or self.count)
        out = np.zeros(n, np.int32)
        self._check(self.L.alore_backend_launch_order(self.h, n, out.ctypes.data_as(C.POINTER(C.c_int))))
        return out

    def device_build_status(self) -> int:
        p = C.c_void_p()
        self._check(self.L.alore_backend_device_build_status(self.h, C.byref(p)))
        return p.value

    def problems(self, count: int | None = None) -> dict:
        """the problem slots as they lie on the device (waits)"""
        n, P = int(count or self.count), self.P
        out = {"n_pieces": np.zeros(n, np.int32), "inner": np.zeros((n, P - 1, 2)), "init_T": np.zeros(n), "positions": np.zeros((n, P, 2)),
               "head": np.zeros((n, 2, 3)), "tail": np.zeros((n, 2, 3)), "start_xytheta": np.zeros((n, 3)), "final_xy": np.zeros((n, 2)),
               "if_cut": np.zeros(n, np.int32)}
        ip = C.POINTER(C.c_int)
        self._check(self.L.alore_backend_get_problems(self.h, n, out["n_pieces"].ctypes.data_as(ip), _dp(out["inner"]), _dp(out["init_T"]),
                                                      _dp(out["positions"]), _dp(out["head"]), _dp(out["tail"]), _dp(out["start_xytheta"]),
                                                      _dp(out["final_xy"]), out["if_cut"].ctypes.data_as(ip)))
        return out

    # ---- laser scans of a resident world cloud (alore_backend_laser_*)
    def laser_create(self, max_scans: int, max_points_per_scan: int = 0, params: LaserParamsC | None = None, **fields):
        """The reference's laser simulator for batches of up to max_scans poses.  params: a LaserParamsC (None: the defaults),
        fields: single members to change (if_perspective=0, sensing_horizon=10.0, ...).  max_points_per_scan: the slots of a scan
        in perspective mode (range mode has hrz x vtc).  Replaces a sensor created before, cloud included."""
        p = LaserParamsC()
        if params is None:
            self.L.alore_backend_laser_default_params(C.byref(p))
        else:
            C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
        for k, v in fields.items():
            if k not in dict(LaserParamsC._fields_):
                raise TypeError(f"alore_backend_laser_params has no field {k}")
            setattr(p, k, v)
        self._check(self.L.alore_backend_laser_create(self.h, C.byref(p), int(max_scans), int(max_points_per_scan)))
        self.laser_params = p
        self.laser_count = 0

    def laser_set_cloud(self, points, stream=None, stride_bytes: int | None = None):
        """The world cloud: NumPy [n][3 or 4] (converted to float32, uploaded, waits), a torch float32 device tensor [n][k >= 3]
        with unit stride along k, or a raw device address given as (address, n) with stride_bytes (default 12); device points are
        copied in stream order."""
        if isinstance(points, tuple):
            ptr, n, stride, dev = int(points[0]) or None, int(points[1]), int(stride_bytes or 12), 1
        elif isinstance(points, np.ndarray) or not hasattr(points, "data_ptr"):
            q = np.asarray(points, np.float32)
            q = np.ascontiguousarray(q.reshape(len(q), -1)) if q.size else np.zeros((0, 3), np.float32)
            ptr, n, stride, dev = q.ctypes.data if q.size else None, q.shape[0], int(stride_bytes or q.shape[1] * 4), 0
        else:
            if str(points.dtype) != "torch.float32" or points.dim() != 2 or (points.shape[0] and points.stride(1) != 1):
                raise BackendError("laser_set_cloud: device points must be a float32 tensor [n][k >= 3] with unit stride along k")
            ptr, n, dev = int(points.data_ptr()) if points.shape[0] else None, int(points.shape[0]), 1
            stride = int(stride_bytes or (points.stride(0) * 4 if n else 12))
        self._check(self.L.alore_backend_laser_set_cloud(self.h, ptr, n, stride, dev, _stream(stream)))

    def laser_scan(self, poses, count: int | None = None, stream=None, pose_stride_bytes: int | None = None):
        """Renders one scan per pose (x, y, yaw).  poses: NumPy [count][>= 3] (uploaded with the argument block; waits), a torch
        float64 device tensor [count][>= 3] (its own row stride: the xytheta of predicted_state_device serves as it lies) or a raw
        device address with count and pose_stride_bytes (default 24); device poses are read in stream order and nothing waits.
        laser_results() / laser_device_view() have the outcome; every scan has its own status."""
        if isinstance(poses, int):
            n, ptr, stride, dev = int(count), poses, int(pose_stride_bytes or 24), 1
        elif hasattr(poses, "data_ptr"):
            if str(poses.dtype) != "torch.float64" or poses.dim() != 2 or poses.stride(1) != 1:
                raise BackendError("laser_scan: device poses must be a float64 tensor [count][>= 3] with unit stride along the row")
            n, ptr, dev = int(count or poses.shape[0]), int(poses.data_ptr()), 1
            stride = int(pose_stride_bytes or poses.stride(0) * 8)
        else:
            q = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(len(poses), -1))
            n, ptr, stride, dev = int(count or q.shape[0]), q.ctypes.data, q.strides[0], 0
        self.laser_count = n
        self._check(self.L.alore_backend_laser_scan(self.h, n, ptr, stride, dev, _stream(stream)))

    def laser_view(self) -> LaserViewC:
        v = LaserViewC()
        self._check(self.L.alore_backend_device_laser(self.h, C.byref(v)))
        return v

    def laser_device_view(self) -> dict:
        """torch views on the device slabs (no copy): range_image [max_scans][hrz][vtc] (None in perspective mode), laser_points,
        world_points and compact_points [max_scans][slots][3], index [max_scans][slots], n_points and status [max_scans].  A row
        of world_points goes straight into map_integrate([(row, pose)]): NaN slots are skipped there."""
        import torch
        v = self.laser_view()
        S, n = v.max_scans, v.slots

        def view(ptr, shape, typestr):
            return torch.as_tensor(_DeviceArray(ptr, shape, typestr), device="cuda") if ptr else None
        p = self.laser_params
        return {"range_image": view(v.range_image, (S, p.hrz_laser_line_num, p.vtc_laser_line_num), "<f8"),
                "laser_points": view(v.laser_points, (S, n, 3), "<f4"), "world_points": view(v.world_points, (S, n, 3), "<f4"),
                "index": view(v.index, (S, n), "<i4"), "compact_points": view(v.compact_points, (S, n, 3), "<f4"),
                "n_points": view(v.n_points, (S,), "<i4"), "status": view(v.status, (S,), "<i4")}

    def laser_results(self, count: int | None = None) -> dict:
        """the slabs of the last scans copied to the host (waits): the arrays of laser_device_view() with count for max_scans;
        range_image is None in perspective mode"""
        n = int(count or getattr(self, "laser_count", 0))
        v, p = self.laser_view(), self.laser_params
        out = {"range_image": np.zeros((n, p.hrz_laser_line_num, p.vtc_laser_line_num)) if v.range_image else None,
               "laser_points": np.zeros((n, v.slots, 3), np.float32), "world_points": np.zeros((n, v.slots, 3), np.float32),
               "index": np.zeros((n, v.slots), np.int32), "compact_points": np.zeros((n, v.slots, 3), np.float32),
               "n_points": np.zeros(n, np.int32), "status": np.zeros(n, np.int32)}
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        self._check(self.L.alore_backend_get_laser(self.h, n, _dp(out["range_image"]), out["laser_points"].ctypes.data_as(fp),
                                                   out["world_points"].ctypes.data_as(fp), out["index"].ctypes.data_as(ip),
                                                   out["compact_points"].ctypes.data_as(fp), out["n_points"].ctypes.data_as(ip),
                                                   out["status"].ctypes.data_as(ip)))
        return out

    # ---- way-point paths by grid search on the handle's map (alore_backend_search_paths)
    def search_paths(self, start_xy, goal_xy, safe_dis=None, window_margin=None, mask=None):
        """Shortest 8-connected paths on the current map from start_xy [count][>= 2] to goal_xy [count][>= 2] (NumPy; x, y first),
        pruned like removeCornerPts, into the device slab of device_paths().  safe_dis / window_margin None: 0.3 / 3.0.  mask: per
        slot, 0 leaves the slot out.  Waits; raises when a slot fails (search_status() says which and why)."""
        st = np.ascontiguousarray(np.asarray(start_xy, np.float64).reshape(len(start_xy), -1))
        gl = np.ascontiguousarray(np.asarray(goal_xy, np.float64).reshape(len(goal_xy), -1))
        if st.shape[0] != gl.shape[0] or st.shape[1] < 2 or gl.shape[1] < 2:
            raise BackendError("search_paths: start_xy and goal_xy must be [count][>= 2] arrays of one length")
        mk = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(bool), np.int32)
        p = _search_params(safe_dis, window_margin)
        self.search_count = st.shape[0]
        self._check(self.L.alore_backend_search_paths(self.h, st.shape[0], st.ctypes.data, st.strides[0], gl.ctypes.data, gl.strides[0],
                                                      C.byref(p), 0, None if mk is None else mk.ctypes.data, 4, None))

    def search_paths_device(self, count, start_xy, goal_xy, start_stride=None, goal_stride=None, safe_dis=None, window_margin=None,
                            mask=None, mask_stride=4, stream=None):
        """The same with everything resident: float64 torch tensors [count][>= 2] (their own row stride; the xytheta [count][3] of
        predicted_state_device serves as the starts as it lies) or raw device addresses with a stride in bytes (default 16); mask
        as for plan().  Nothing is copied but the argument block and nothing waits; search_status() has the outcome per slot."""
        def stride(a, given):
            if given is not None:
                return int(given)
            return 16 if a is None or isinstance(a, int) else int(a.stride(0) * a.element_size())
        p = _search_params(safe_dis, window_margin)
        mp, ms = _mask(mask, mask_stride)
        self.search_count = int(count)
        self._check(self.L.alore_backend_search_paths(self.h, int(count), _dev(start_xy), stride(start_xy, start_stride), _dev(goal_xy),
                                                      stride(goal_xy, goal_stride), C.byref(p), 1, mp, ms, _stream(stream)))

    def search_reserve(self, max_cells: int, slots: int = 1):
        """Opt in to windows of more than SEARCH_MAX_CELLS cells: reserves `slots` slabs of max_cells words of device memory
        (max_cells in (32768, 1 << 22], slots in [1, 1024], at most 1 GiB in all).  From then on search_paths and
        search_paths_device search a slot whose window has up to max_cells cells instead of giving it SEARCH_E_WINDOW, `slots`
        of them at a time; smaller windows go the way they went.  A second call replaces the first, max_cells = 0 releases it."""
        self._check(self.L.alore_backend_search_reserve(self.h, int(max_cells), int(slots)))

    def search_reserved(self) -> tuple:
        """(max_cells, slots) of the reservation, (0, 0) without one"""
        a, b = C.c_int(), C.c_int()
        self._check(self.L.alore_backend_search_reserved(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def device_paths(self) -> PathsC:
        """the device slab of searched paths as alore_backend_paths: max_points 31, n_points and xy set, the yaws and start
        derivatives None for the caller to fill (set_paths_device(count, v.max_points, v.n_points, v.xy, start_yaw, end_yaw, ...))"""
        v = PathsC()
        self._check(self.L.alore_backend_device_paths(self.h, C.byref(v)))
        return v

    def device_search_status(self) -> int:
        p = C.c_void_p()
        self._check(self.L.alore_backend_device_search_status(self.h, C.byref(p)))
        return p.value

    def search_status(self, count: int | None = None) -> np.ndarray:
        """per slot of the last search: 0 found, 1 masked out, -1 end point, -2 same cell, -3 window, -4 no path, -5 points,
        -6 range (wide route only) (waits)"""
        n = int(count or getattr(self, "search_count", 0))
        out = np.zeros(n, np.int32)
        self._check(self.L.alore_backend_search_status(self.h, n, out.ctypes.data_as(C.POINTER(C.c_int))))
        return out

    def search_sweeps(self, count: int | None = None) -> np.ndarray:
        """diagnostic: sweeps over the window until the field stood still, per slot of the last search; visits of tiles for a slot
        searched on the wide route (waits)"""
        n = int(count or getattr(self, "search_count", 0))
        out = np.zeros(n, np.int32)
        self._check(self.L.alore_backend_search_sweeps(self.h, n, out.ctypes.data_as(C.POINTER(C.c_int))))
        return out

    def search_wide_ticks(self, count: int | None = None) -> np.ndarray:
        """diagnostic, reserved handles: [count][2] ticks of the 100 MHz device clock of the slots searched on the wide route, whole
        slot and its walk and pruning (waits)"""
        n = int(count or getattr(self, "search_count", 0))
        out = np.zeros((n, 2), np.int64)
        self._check(self.L.alore_backend_search_wide_ticks(self.h, n, out.ctypes.data_as(C.POINTER(C.c_longlong))))
        return out

    def paths(self, count: int | None = None) -> dict:
        """the slab of searched paths copied to the host (waits): n_points [count], xy [count][31][2], cost_ab [count][2]"""
        n = int(count or getattr(self, "search_count", 0))
        out = {"n_points": np.zeros(n, np.int32), "xy": np.zeros((n, MAX_PATH_POINTS, 2)), "cost_ab": np.zeros((n, 2), np.int32)}
        ip = C.POINTER(C.c_int)
        self._check(self.L.alore_backend_get_paths(self.h, n, out["n_points"].ctypes.data_as(ip), _dp(out["xy"]), out["cost_ab"].ctypes.data_as(ip)))
        return out

    # ---- the visit order of rearrangement missions from path costs on the handle's map (alore_backend_task_plan)
    def task_plan(self, n_tasks, points, assignment=None, mode=None, safe_dis=None, window_margin=None, mask=None, check=True):
        """plan_manager's task planning for a batch of missions (NumPy in): n_tasks [count]; points [count][1 + 2 max_tasks][2], per
        mission the robot, its n items, its n targets, packed at the beginning of the row; assignment [count][max_tasks] (optimal
        mode; None: the identity); mode TASK_GREEDY (None), TASK_OPTIMAL, TASK_ASSIGNED (the assignment of least carrying distance,
        then the optimal order for it) or TASK_JOINT (assignment and order together, n <= 5), the last two with their choice in
        task_assignment(); safe_dis / window_margin None: 0.3 / 3.0; mask: per
        mission, 0 leaves it out.  Waits.  Raises when a mission fails unless check is False; task_result() has the outcome."""
        pts = np.ascontiguousarray(np.asarray(points, np.float64))
        nt = np.ascontiguousarray(np.asarray(n_tasks, np.int32).reshape(-1))
        if pts.ndim != 3 or pts.shape[2] != 2 or pts.shape[1] < 3 or pts.shape[1] % 2 == 0 or pts.shape[0] != nt.shape[0]:
            raise BackendError("task_plan: points must be [count][1 + 2 max_tasks][2], n_tasks [count]")
        max_tasks = (pts.shape[1] - 1) // 2
        asg = None
        if assignment is not None:
            asg = np.ascontiguousarray(np.asarray(assignment, np.int32))
            if asg.shape != (nt.shape[0], max_tasks):
                raise BackendError("task_plan: assignment must be [count][max_tasks]")
        mk = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(bool), np.int32)
        p = _task_params(safe_dis, window_margin, mode)
        self.task_count = nt.shape[0]
        rc = self.L.alore_backend_task_plan(self.h, nt.shape[0], max_tasks, nt.ctypes.data, pts.ctypes.data, pts.strides[0],
                                            None if asg is None else asg.ctypes.data, C.byref(p), 0, None if mk is None else mk.ctypes.data,
                                            4, None)
        if rc != 0 and not check and self.L.alore_backend_last_error(self.h).decode().startswith("task_plan: mission failed"):
            return                                                       # the launch ran and a mission failed: its status says why
        self._check(rc)                                                  # anything else launched nothing: always raised

    def task_plan_device(self, count, max_tasks, n_tasks, points, point_row_stride=None, assignment=None, mode=None, safe_dis=None,
                         window_margin=None, mask=None, mask_stride=4, stream=None):
        """The same with everything resident: n_tasks int32 [count], points float64 [count][>= 1 + 2 max_tasks][2] (its own row
        stride), assignment int32 [count][max_tasks] or None: torch tensors, or raw device addresses (points then with
        point_row_stride in bytes); mask as for plan().  Nothing is copied but the argument block and nothing waits;
        task_result() / device_task() have the outcome per mission."""
        if point_row_stride is None:
            point_row_stride = 16 * (1 + 2 * int(max_tasks)) if isinstance(points, int) else int(points.stride(0) * points.element_size())
        p = _task_params(safe_dis, window_margin, mode)
        mp, ms = _mask(mask, mask_stride)
        self.task_count = int(count)
        self._check(self.L.alore_backend_task_plan(self.h, int(count), int(max_tasks), _dev(n_tasks), _dev(points), int(point_row_stride),
                                                   _dev(assignment), C.byref(p), 1, mp, ms, _stream(stream)))

    def device_task(self) -> TaskViewC:
        """the device slab of the missions (alore_backend_task_view).  Leg l of every mission goes into search_paths_device as it
        lies: start v.leg_start_xy + 16 l, goal v.leg_goal_xy + 16 l, both strides 16 * v.max_legs bytes"""
        v = TaskViewC()
        self._check(self.L.alore_backend_device_task(self.h, C.byref(v)))
        return v

    def task_result(self, count: int | None = None, res: float | None = None) -> dict:
        """the slab of the missions copied to the host (waits): status, n_order, fields, sweeps [count]; matrix [count][21][21][2]
        (the pairs (a, b), (-1, -1) for no path; entries beyond a mission's points are not written); order [count][20]; total
        [count][2]; leg_start_xy, leg_goal_xy [count][20][2]; and cost_m [count][21][21] = (a + b sqrt 2) res in metres, inf where
        there is no path (res: the cell size, None: the one of the map this planner was given)"""
        n = int(count or getattr(self, "task_count", 0))
        P, L = TASK_MAX_POINTS, TASK_MAX_LEGS
        out = {"status": np.zeros(n, np.int32), "matrix": np.zeros((n, P, P, 2), np.int32), "order": np.zeros((n, L), np.int32),
               "n_order": np.zeros(n, np.int32), "total": np.zeros((n, 2), np.int32), "leg_start_xy": np.zeros((n, L, 2)),
               "leg_goal_xy": np.zeros((n, L, 2)), "fields": np.zeros(n, np.int32), "sweeps": np.zeros(n, np.int32)}
        ip = C.POINTER(C.c_int)
        i = lambda k: out[k].ctypes.data_as(ip)
        self._check(self.L.alore_backend_get_task(self.h, n, i("status"), i("matrix"), i("order"), i("n_order"), i("total"),
                                                  _dp(out["leg_start_xy"]), _dp(out["leg_goal_xy"]), i("fields"), i("sweeps")))
        res = getattr(self, "map_res", None) if res is None else float(res)
        if res is not None:
            a, b = out["matrix"][..., 0].astype(np.float64), out["matrix"][..., 1].astype(np.float64)
            out["cost_m"] = np.where(out["matrix"][..., 0] < 0, np.inf, (a + b * np.sqrt(2.0)) * res)
        return out

    def task_reorder(self, stream=None):
        """diagnostic: the order phase of the last task_plan / task_plan_device launch again, alone, on the matrices in the slab"""
        self._check(self.L.alore_backend_task_reorder(self.h, _stream(stream)))

    def task_reserve(self, max_cells: int, slots: int = 1):
        """Opt in to missions on windows of more than SEARCH_MAX_CELLS cells: reserves `slots` slabs of max_cells words of device
        memory for task_plan (its own; search_reserve's stay the search's; max_cells in (32768, 1 << 22], slots in [1, 1024], at
        most 1 GiB in all).  From then on task_plan and task_plan_device plan a mission whose window has up to max_cells cells
        instead of giving it TASK_E_WINDOW, the fields of `slots` (mission, source point) pairs at a time; smaller windows go the
        way they went.  One status is new on that route, TASK_E_RANGE.  A second call replaces the first, max_cells = 0 releases
        it.  The legs of such a mission need search_reserve if they are to be searched afterwards."""
        self._check(self.L.alore_backend_task_reserve(self.h, int(max_cells), int(slots)))

    def task_reserved(self) -> tuple:
        """(max_cells, slots) of the task reservation, (0, 0) without one"""
        a, b = C.c_int(), C.c_int()
        self._check(self.L.alore_backend_task_reserved(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def task_wide_ticks(self, count: int | None = None) -> np.ndarray:
        """diagnostic (task_reserve only): [count][TASK_MAX_LEGS] ticks of the device's 100 MHz clock that the fields of a source
        point took on the wide route; waits"""
        n = int(count or getattr(self, "task_count", 0))
        out = np.zeros((n, TASK_MAX_LEGS), np.int64)
        self._check(self.L.alore_backend_task_wide_ticks(self.h, n, out.ctypes.data_as(C.POINTER(C.c_longlong))))
        return out

    def device_task_assign(self) -> TaskAssignViewC:
        """the device rows of the assignment that the last TASK_ASSIGNED / TASK_JOINT launch chose (alore_backend_task_assign_view)"""
        v = TaskAssignViewC()
        self._check(self.L.alore_backend_device_task_assign(self.h, C.byref(v)))
        return v

    def task_assignment(self, count: int | None = None) -> dict:
        """those rows copied to the host (waits): assignment [count][10], the target of item i for i < n, and assign_total
        [count][2], the pair (a, b) of the sum of its carry legs.  Written by missions that are OK in the mode TASK_ASSIGNED or
        TASK_JOINT (TASK_ASSIGNED: also where the chosen assignment has no finite order); untouched otherwise"""
        n = int(count or getattr(self, "task_count", 0))
        out = {"assignment": np.zeros((n, TASK_MAX_TASKS), np.int32), "assign_total": np.zeros((n, 2), np.int32)}
        ip = C.POINTER(C.c_int)
        self._check(self.L.alore_backend_get_task_assign(self.h, n, out["assignment"].ctypes.data_as(ip), out["assign_total"].ctypes.data_as(ip)))
        return out

    def predicted_state_device(self, count, times, xytheta, vaj, oaj, forward, resolution: float = 0.01, start_times=None, start_xytheta=None,
                               stream=None):
        """predicted_state with device inputs (times [count], start_times [count] or None, start_xytheta [count][3] or None) and
        outputs (xytheta, vaj, oaj [count][3] float64, forward [count] int32): torch tensors or addresses; no copy, nothing waits"""
        self._check(self.L.alore_backend_predicted_state_device(self.h, int(count), float(resolution), _dev(start_times), _dev(times),
                                                                _dev(start_xytheta), _dev(xytheta), _dev(vaj), _dev(oaj), _dev(forward),
                                                                _stream(stream)))

    def set_free_map(self, half: float = 40.0, res: float = 0.1, value: float = 100.0):
        n = int(round(2 * half / res))
        self.set_map(np.full((n, n), value), -half, -half, res)

    def set_problems(self, flat_trajs):
        n = len(flat_trajs)
        arr = (FlatTrajC * n)()
        keep = []
        for b, ft in enumerate(flat_trajs):
            pts = np.ascontiguousarray(ft.traj_pts, dtype=np.float64).reshape(-1, 3)
            pos = np.ascontiguousarray(ft.positions, dtype=np.float64).reshape(-1, 3)
            keep += [pts, pos]
            a = arr[b]
            a.n_pieces = len(pts) + 1
            a.traj_pts = pts.ctypes.data
            a.positions = pos.ctypes.data
            a.init_T = ft.init_T
            for d in range(2):
                for k in range(3):
                    a.start_state[d][k] = ft.start_state[d, k]
                    a.final_state[d][k] = ft.final_state[d, k]
            for k in range(3):
                a.start_xytheta[k] = ft.start_xytheta[k]
                a.final_xytheta[k] = ft.final_xytheta[k]
            a.if_cut = int(ft.if_cut)
        self._keep = keep
        self._check(self.L.alore_backend_set_problems(self.h, n, arr, None))
        self.count = n
        self._pieces = np.array([a.n_pieces for a in arr])

    def plan(self, count: int | None = None, mask=None, mask_stride: int = 4, stream=None):
        """mask (device memory: a torch int32 tensor, an address with mask_stride bytes between the words, or check_mask()):
        only the slots whose word is not 0 are planned, the others keep their stored plan bit for bit"""
        if mask is None:
            self._check(self.L.alore_backend_plan(self.h, count or self.count, _stream(stream)))
            return
        mp, ms = _mask(mask, mask_stride)
        self._check(self.L.alore_backend_plan_masked(self.h, count or self.count, mp, ms, _stream(stream)))

    def replan_mask(self, out_mask, count: int | None = None, stream=None):
        """out_mask (int32 device tensor [count] or an address) <- 1 where the last check_plans flags a collision AND the slot was
        searched, built and planned with success, else 0: the slots whose NEW plan may be delivered
        (BatchedNmpc.refs_set_pending_from_backend takes it as its mask).  Nothing waits."""
        self._check(self.L.alore_backend_replan_mask(self.h, int(count or self.count), _dev(out_mask), _stream(stream)))

    def last_plan_ms(self) -> float:
        ms = C.c_float()
        self._check(self.L.alore_backend_last_plan_ms(self.h, C.byref(ms)))
        return ms.value

    def results(self, count: int | None = None, stream=None) -> dict:
        n = count or self.count
        st = (StatusC * n)()
        inner = np.zeros((n, self.P - 1, 2))
        T = np.zeros((n, self.P))
        coef = np.zeros((n, self.P * 6, 2))
        self._check(self.L.alore_backend_results(self.h, n, st, _dp(inner), _dp(T), _dp(coef), _stream(stream)))
        out = {k: np.array([getattr(s, k) for s in st]) for k in
               ("ok", "attempts", "alm_rounds", "evals", "lbfgs_ret", "path_ret", "collision", "n_pieces", "cost", "min_dist", "tail_s")}
        out["xy_err"] = np.array([[s.xy_err[0], s.xy_err[1]] for s in st])
        out["inner"], out["T"], out["coef"] = inner, T, coef
        return out

    def minco_plan(self, flat_trajs) -> dict:
        self.set_problems(flat_trajs)
        self.plan()
        return self.results()

    def device_view(self) -> DeviceView:
        v = DeviceView()
        self._check(self.L.alore_backend_device_results(self.h, C.byref(v)))
        return v

    # ---- pieces of the optimiser for parity tests
    def pack_x(self, xs) -> np.ndarray:
        out = np.zeros((len(xs), 3 * self.P))
        for b, x in enumerate(xs):
            out[b, :len(x)] = x
        return out

    def _configured(self, value, of_cfg):
        """safe_dis / time_weight of eval and lbfgs: a given value holds for every slot; None is the configured one -- the
        handle's config's, or with a class table NaN, which the library resolves to the slot's class's"""
        if value is not None:
            return float(value)
        return float("nan") if self.n_classes else of_cfg

    def eval(self, stage: int, xs, lam=None, rho=None, safe_dis=None, time_weight=None):
        n = len(xs)
        X = self.pack_x(xs)
        cost = np.zeros(n); grad = np.zeros_like(X); err = np.zeros((n, 2))
        lam = None if lam is None else np.ascontiguousarray(np.broadcast_to(lam, (n, 2)), dtype=np.float64)
        rho = None if rho is None else np.ascontiguousarray(np.broadcast_to(rho, (n, 2)), dtype=np.float64)
        self._check(self.L.alore_backend_eval(self.h, n, stage, _dp(X), _dp(lam), _dp(rho),
                                              self._configured(safe_dis, self.cfg.safe_dis),
                                              self._configured(time_weight, self.cfg.w_time), _dp(cost), _dp(grad),
                                              _dp(err), None))
        return {"cost": cost, "grad": [grad[b, :len(xs[b])] for b in range(n)], "xy_err": err}

    def lbfgs(self, stage: int, xs, lam=None, rho=None, max_iter=0, safe_dis=None, time_weight=None):
        n = len(xs)
        X = self.pack_x(xs)
        cost = np.zeros(n); err = np.zeros((n, 2))
        ret = (C.c_int * n)(); it = (C.c_int * n)(); ev = (C.c_int * n)()
        lam = None if lam is None else np.ascontiguousarray(np.broadcast_to(lam, (n, 2)), dtype=np.float64)
        rho = None if rho is None else np.ascontiguousarray(np.broadcast_to(rho, (n, 2)), dtype=np.float64)
        self._check(self.L.alore_backend_lbfgs(self.h, n, stage, _dp(X), _dp(lam), _dp(rho),
                                               self._configured(safe_dis, self.cfg.safe_dis),
                                               self._configured(time_weight, self.cfg.w_time), max_iter, _dp(cost),
                                               ret, it, ev, _dp(err), None))
        return {"x": [X[b, :len(xs[b])] for b in range(n)], "cost": cost, "ret": np.array(ret[:]), "iters": np.array(it[:]),
                "evals": np.array(ev[:]), "xy_err": err}

    # ---- the message plan_manager publishes from the result (plan_manager.hpp:784-831)
    def polynomes(self, flat_trajs, res: dict, traj_start_time: float = 0.0) -> list:
        """One dict per problem with the fields of carstatemsgs/Polynome."""
        out = []
        for b, ft in enumerate(flat_trajs):
            M = int(res["n_pieces"][b])
            tail = ft.final_state.copy()
            tail[1, 0] = res["tail_s"][b]
            icr = (0.0, 0.0, 0.0) if self.cfg.standard_diff else (0.0, 0.0, self.cfg.icr_xv)
            out.append({"innerpoints": res["inner"][b, :M - 1].copy(), "t_pts": res["T"][b, :M].copy(),
                        "init_pva": np.array([ft.start_state[0, 0], ft.start_state[1, 0], ft.start_state[0, 1], ft.start_state[1, 1],
                                              ft.start_state[0, 2], ft.start_state[1, 2]]),
                        "tail_pva": np.array([tail[0, 0], tail[1, 0], tail[0, 1], tail[1, 1], tail[0, 2], tail[1, 2]]),
                        "start_position": np.array(ft.start_xytheta, dtype=np.float64), "ICR": np.array(icr),
                        "traj_start_time": traj_start_time})
        return out
