"""One replan cycle of a device-resident fleet, enqueued on one stream without a host wait.

What plan_manager does for one robot when its trajectory collides with the map of now (plan_manager.hpp:585-588, 686-727): check the
stored plan, predict the state at current + max_replan_time, search a path from there, build the problem, plan, and publish the new
trajectory stamped with current + max_replan_time, which the controller swaps in once that time has passed (mpc.cpp:177-182).  Here
for every robot of a BatchedMSPlanner / BatchedNmpc pair at once:

  1. check_plans             which stored plans collide, from where each robot is now (t_from = now - active start time)
  2. predicted_state_device  the state to replan from, at now + max_replan_time - start along the stored plan
  3. search_paths_device     a way-point path from there to the goal, flagged slots only
  4. set_paths_device        the problems of the flagged slots
  5. plan (masked)           the flagged slots; every other slot keeps its plan bit for bit
  6. replan_mask             the delivery mask: flagged AND searched, built and planned with success
  7. refs_set_pending_from_backend   pending slots of the masked robots, traj_start_time = now + max_replan_time

in the order the header of alore_backend_set_paths prescribes (check and predict, then paths, then plan).  A robot whose replan failed
keeps its colliding trajectory; the reference goes to EMERGENCY_STOP there (plan_manager.hpp:662-666): that stays with the caller, who
reads the collision words (planner.device_check()) and the mask."""
from __future__ import annotations

import numpy as np


class ReplanWork:
    """the device tensors a cycle works on, allocated once: nothing is allocated in a cycle that is given one"""

    def __init__(self, count: int, device="cuda"):
        import torch
        f64 = dict(dtype=torch.float64, device=device)
        self.count = int(count)
        self.times = torch.zeros(count, **f64)          # time along the stored plan of the predicted state
        self.xytheta = torch.zeros(count, 3, **f64)     # predicted state: the start of the replan
        self.vaj = torch.zeros(count, 3, **f64)
        self.oaj = torch.zeros(count, 3, **f64)
        self.start_yaw = torch.zeros(count, **f64)
        self.forward = torch.zeros(count, dtype=torch.int32, device=device)
        self.mask = torch.zeros(count, dtype=torch.int32, device=device)   # the delivery mask of the last cycle
        self.h_times = torch.zeros(count, dtype=torch.float64).pin_memory()
        self.h_times_read = torch.cuda.Event()          # the last cycle's copy out of h_times


def replan_cycle(planner, nmpc, now: float, max_replan_time: float, goals_xy, end_yaw, start_times=0.0, work: ReplanWork | None = None,
                 count: int | None = None, min_safe_dis=None, body: bool = False, xv=0.0, state_seq_res: float = 0.1,
                 integral_res_int: int = 4, resolution: float = 0.01, safe_dis=None, params=None, mark=None) -> ReplanWork:
    """Enqueues the seven steps on the stream of `nmpc` (torch's current stream) and returns at once; work.mask is the delivery mask.

    goals_xy [count][>= 2], end_yaw [count]: float64 device tensors.  start_times: the start times of the ACTIVE trajectories as the
    caller delivered them (host scalar or array [count]); a robot whose pending entry has been promoted since has that entry's
    start time.  xv: the ICR offset the store integrates the delivered plans with, a float for every slot or a float64 device
    tensor with an entry per slot (planner.class_xv() on a handle with object classes).  mark: None, or a callable that is given
    the name of every step after it has been enqueued (tools/traj_handoff.py records an event there)."""
    mark = mark or (lambda name: None)
    n = int(count or planner.count)
    w = work or ReplanWork(n, goals_xy.device)
    s = nmpc._stream().value                               # raw hipStream_t (None: the default stream)
    start = np.broadcast_to(np.asarray(start_times, np.float64), (n,))
    planner.check_plans(t_from=now - start, min_safe_dis=min_safe_dis, body=body, count=n, stream=s, fetch=False)
    mark("check_plans")
    w.h_times_read.synchronize()                           # the cycle before has read the pinned block (never waits in practice)
    w.h_times[:n] = nmpc.torch.from_numpy(now + max_replan_time - start)
    w.times[:n].copy_(w.h_times[:n], non_blocking=True)   # pinned: enqueued, the host goes on
    w.h_times_read.record()
    planner.predicted_state_device(n, w.times, w.xytheta, w.vaj, w.oaj, w.forward, resolution, stream=s)
    mark("predicted_state")
    planner.search_paths_device(n, w.xytheta, goals_xy, safe_dis=safe_dis, mask=planner.check_mask(), stream=s)
    mark("search_paths")
    w.start_yaw[:n].copy_(w.xytheta[:n, 2])
    v = planner.device_paths()
    planner.set_paths_device(n, v.max_points, v.n_points, v.xy, w.start_yaw, end_yaw, w.vaj, w.oaj, params=params,
                             mask=planner.check_mask(), stream=s)
    mark("set_paths")
    planner.plan(count=n, mask=planner.check_mask(), stream=s)
    mark("plan_masked")
    planner.replan_mask(w.mask, count=n, stream=s)
    mark("replan_mask")
    nmpc.refs_set_pending_from_backend(planner, count=n, mask=w.mask, traj_start_time=now + max_replan_time, xv=xv,
                                       state_seq_res=state_seq_res, integral_res_int=integral_res_int)
    mark("set_pending")
    return w


class ManagerWork:
    """the device tensors a manager period works on, allocated once, and torch views of the manager's slab (planner.manager_create
    first): nothing is allocated in a period that is given one"""

    def __init__(self, planner, count: int | None = None, device="cuda"):
        import torch
        from .backend import _DeviceArray
        n = self.count = int(count or planner.B)
        f64 = dict(dtype=torch.float64, device=device)
        self.xytheta = torch.zeros(n, 3, **f64)         # predicted state, then the start of every plan of the period
        self.vaj = torch.zeros(n, 3, **f64)
        self.oaj = torch.zeros(n, 3, **f64)
        self.start_yaw = torch.zeros(n, **f64)
        self.end_yaw = torch.zeros(n, **f64)
        self.goal_xy = torch.zeros(n, 2, **f64)         # the goals as the search reads them
        self.forward = torch.zeros(n, dtype=torch.int32, device=device)
        self.run_mask = torch.zeros(n, dtype=torch.int32, device=device)    # plan_mask AND searched AND built: the slots the optimiser runs
        v, B = planner.manager_view(), planner.B
        ints = lambda a: torch.as_tensor(_DeviceArray(a, (B,), "<i4"), device=device)
        self.goal = torch.as_tensor(_DeviceArray(v.goal, (3, B), "<f8"), device=device)
        self.time = v.time                               # address: the d_time of predicted_state_device
        self.plan_mask, self.fresh_mask, self.replan_mask, self.stop_mask, self.after_plan_mask = (
            ints(a) for a in (v.plan_mask, v.fresh_mask, v.replan_mask, v.stop_mask, v.after_plan_mask))
        self.search_status = ints(planner.device_search_status())
        self.build_status = ints(planner.device_build_status())
        self.planned = False                             # a plan has been launched on the handle: the predicted state exists


def manager_cycle(planner, nmpc, now: float, poses, work: ManagerWork | None = None, count: int | None = None, collision_mask=None,
                  pose_stride: int = 24, nmpc_plant: bool = True, ltv=None, xv=0.0, state_seq_res: float = 0.1, integral_res_int: int = 4,
                  resolution: float = 0.01, safe_dis=None, window_margin=None, params=None, mark=None) -> ManagerWork:
    """One period of plan_manager's MainThread for every robot of a BatchedMSPlanner (manager_create first) / BatchedNmpc pair,
    enqueued on the stream of `nmpc` (torch's current stream); returns at once.  Who plans, from where, what is delivered under which
    start time and who is stopped is decided on the device (csrc/fleet_manager.h); there is no per-robot state on the host.

      1. manager_begin            FRESH, REPLAN or nothing for every robot, and the time of the predicted state
      2. predicted_state_device   (from the handle's first plan on) the state to replan from
      3. manager_starts           FRESH robots start from their requested start; start_yaw / end_yaw; then the goals for the search
      4. mission_set_goals        (a handle with missions) under plan_mask
      5. search_paths_device      under plan_mask
      6. set_paths_device         under plan_mask
      7. plan (masked)            the slots of plan_mask that were searched and built: a slot whose search failed is not planned again
      8. manager_end              the delivery masks, the stop flags, the finish rule
      9. refs_set_pending_from_backend   twice: fresh_mask with start time now, replan_mask with now + max_replan_time
     10. refs_stop, plant_stop    under stop_mask (nmpc_plant False: the NMPC handle has no plant; ltv: a BatchedLtvMpc whose plant
                                  is stopped as well)
     11. mission_step             (a handle with missions) with after_plan_mask

    poses: float64 device tensor [count][>= 2] or an address with pose_stride bytes between robots (x, y first).  collision_mask: who
    may replan under replan_on_collision_only (planner.check_mask() after a check_plans of the caller's).  xv: as for
    replan_cycle, a float or a float64 device tensor per slot (planner.class_xv()), for both deliveries.  The cold start of a robot
    that had no trajectory stays with the caller (alore_nmpc.h)."""
    mark = mark or (lambda name: None)
    n = int(count or planner.B)
    w = work or ManagerWork(planner, n)
    s = nmpc._stream().value
    if not isinstance(poses, int):
        pose_stride = int(poses.stride(0) * poses.element_size())
    planner.manager_begin(now, poses, collision_mask, stride=pose_stride, count=n, stream=s)
    mark("manager_begin")
    if w.planned and planner.count >= n:
        planner.predicted_state_device(n, w.time, w.xytheta, w.vaj, w.oaj, w.forward, resolution, stream=s)
        mark("predicted_state")
    planner.manager_starts(n, w.xytheta, w.vaj, w.oaj, w.start_yaw, w.end_yaw, stream=s)
    w.goal_xy[:n].copy_(w.goal[:2, :n].T)
    mark("manager_starts")
    missions = hasattr(planner, "mission_params")
    if missions:
        planner.mission_set_goals(w.goal_xy, mask=w.plan_mask, stride=16, count=n, stream=s)
        mark("mission_set_goals")
    planner.search_paths_device(n, w.xytheta, w.goal_xy, safe_dis=safe_dis, window_margin=window_margin, mask=w.plan_mask, stream=s)
    mark("search_paths")
    v = planner.device_paths()
    planner.set_paths_device(n, v.max_points, v.n_points, v.xy, w.start_yaw, w.end_yaw, w.vaj, w.oaj, params=params, mask=w.plan_mask,
                             stream=s)
    mark("set_paths")
    w.run_mask[:n].copy_((w.plan_mask[:n] != 0) & (w.search_status[:n] == 0) & (w.build_status[:n] == 0))
    planner.plan(count=n, mask=w.run_mask, stream=s)
    w.planned = True
    mark("plan_masked")
    planner.manager_end(n, stream=s)
    mark("manager_end")
    kw = dict(count=n, xv=xv, state_seq_res=state_seq_res, integral_res_int=integral_res_int)
    nmpc.refs_set_pending_from_backend(planner, mask=w.fresh_mask, traj_start_time=now, **kw)
    nmpc.refs_set_pending_from_backend(planner, mask=w.replan_mask, traj_start_time=now + planner.manager_params.max_replan_time, **kw)
    mark("set_pending")
    nmpc.refs_stop(w.stop_mask)
    if nmpc_plant:
        nmpc.plant_stop(w.stop_mask)
    if ltv is not None:
        ltv.plant_stop(w.stop_mask, n)
    mark("stop")
    if missions:
        planner.mission_step(poses, after_plan_mask=w.after_plan_mask, stride=pose_stride, count=n, stream=s)
        mark("mission_step")
    return w
