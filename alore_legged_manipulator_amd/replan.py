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
                 count: int | None = None, min_safe_dis=None, body: bool = False, xv: float = 0.0, state_seq_res: float = 0.1,
                 integral_res_int: int = 4, resolution: float = 0.01, safe_dis=None, params=None, mark=None) -> ReplanWork:
    """Enqueues the seven steps on the stream of `nmpc` (torch's current stream) and returns at once; work.mask is the delivery mask.

    goals_xy [count][>= 2], end_yaw [count]: float64 device tensors.  start_times: the start times of the ACTIVE trajectories as the
    caller delivered them (host scalar or array [count]); a robot whose pending entry has been promoted since has that entry's
    start time.  mark: None, or a callable that is given the name of every step after it has been enqueued (tools/traj_handoff.py
    records an event there)."""
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
