"""Timing of the task FSM's tick and of its callbacks against the routes through the host (profiles/task_fsm.txt).

    python tools/task_fsm.py [--out FILE]

Device: HIP events around one call with device pointers.  Two routes that are compared are timed ALTERNATELY (A B A B ...) after a
warm-up, and the median of each is reported with its minimum and maximum.  Tick: 64 / 512 / 4096 robots with no robot, one robot and
every robot in GRASPING with the IK running (the arm's default parameters: 200 iterations).  The host route of a tick is what a fleet
did before: alore_arm_get_grasp, the NumPy oracle of tests/task_fsm_cases.py for every robot that does not grasp, and the upload of
its commands (wall clock, the device idle in between).  Paths: path_points_device -> set_paths on one stream against path_points ->
NumPy -> a host-pointer set_paths.

THE ONE CONDITION: a tick with no robot in GRASPING costs less than a tenth of a tick with all of them grasping (launch-bound against
200 dependent float64 IK iterations): the early exit of a wavefront without a grasping lane works.  The tool prints it and exits
with status 1 if it does not hold."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import arm_ik_cases as arm_cases  # noqa: E402
from tests import task_fsm_cases as cases  # noqa: E402

REPEATS, WARMUP = 9, 3


def alternate(routes):
    """routes: name -> (fn, 'event' | 'wall').  Returns name -> (median, min, max) in ms, the routes taken in turn"""
    import torch
    for _ in range(WARMUP):
        for fn, _ in routes.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in routes}
    for _ in range(REPEATS):
        for k, (fn, how) in routes.items():
            if how == "event":
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                out[k].append(a.elapsed_time(b))
            else:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                out[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def fleet(n, grasping):
    """n robots, chair / table / box in turn, in ROBOT_TRACKING on a two-point path but for the first `grasping`, which are in GRASPING
    past the approach and the wait with a reachable grasp pose: their IK runs on every tick"""
    import torch
    from alore_legged_manipulator_amd import arm, task_fsm
    h = arm.BatchedArm(n)
    h.set_classes([arm.PRESETS[k] for k in arm.PRESET_NAMES])
    rows = arm_cases.grasp_scene()
    pick = [rows[i % 3] for i in range(n)]
    h.set_robot_classes(np.array([r["class_index"] for r in pick], np.int32))
    f = task_fsm.BatchedTaskFsm(h, 2, 1, 24)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda")
    pose = np.zeros((n, 4))
    pose[:, 0:2] = [r["robot_xy"][-1] for r in pick]
    args = (dev(pose), dev(np.array([r["object_pose"] for r in pick])[:, None, :]), dev(np.array([r["arm_base_pose"] for r in pick])),
            dev(np.tile(arm_cases.Q0, (n, 1))))                      # the measured joints stay at q0: every timed tick is the same work
    view = f.view()
    path = np.zeros((n, 24, 2))
    path[:, 0], path[:, 1] = pose[:, 0:2] + [30.0, 4.0], pose[:, 0:2] + [60.0, 8.0]      # far away: tracking never reaches a point
    view["robot_path"].copy_(dev(path))
    view["n_robot_path"].fill_(2)
    view["task_state"].fill_(task_fsm.ROBOT_TRACKING)
    if grasping:
        view["task_state"][:grasping] = task_fsm.GRASPING
        gv = h.grasp_view()
        gv["flag"][:grasping] = 1
        gv["grasp_time"][:grasping] = arm_cases.WAIT_TICKS
    torch.cuda.synchronize()
    return h, f, args


def host_tick(h, f, n, pose, objs):
    """the route through the host: the grasp state down, the oracle's tracking tick per robot, the commands up"""
    import torch
    g = h.get_grasp(n)
    s = f.get(n)
    vel = g["robot_vel_cmd"].copy()
    for b in range(n):
        if s["task_state"][b] != 2:
            continue
        m = cases.TaskFsm(arm_cases.class_row("chair"), [0.0, 0.0], n_objects=1)
        m.task_state, m.robot_path, m.robot_path_index = "ROBOT_TRACKING", [cases.Point(*p) for p in s["robot_path"][b, :s["n_robot_path"][b]]], int(s["robot_path_index"][b])
        m.reach_threshold = float(s["reach_threshold"][b])
        m.tick(pose[b], objs[b], [0, 0, 0, 0, 0, 0, 1.0], arm_cases.Q0)
        vel[b] = m.g.robot_vel_cmd
    h.grasp_view()["robot_vel_cmd"][:n].copy_(torch.tensor(vel, device="cuda"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    lines = ["device: %s" % torch.cuda.get_device_name(0),
             "HIP events (wall clock for the host routes), routes taken in turn, median of %d after %d warm-up rounds (min, max)" % (REPEATS, WARMUP),
             "one tick, device pointers, state resident (the arm's default IK parameters: a grasping robot runs 200 iterations):"]
    ok = True
    for n in (64, 512, 4096):
        made = {k: fleet(n, g) for k, g in (("none", 0), ("one", 1), ("all", n))}
        routes = {k: ((lambda f=f, a=a: f.tick(*a)), "event") for k, (h, f, a) in made.items()}
        if n == 64:
            h0, f0, a0 = made["none"]
            pose, objs = a0[0].cpu().numpy(), a0[1].cpu().numpy()
            routes["host"] = ((lambda: host_tick(h0, f0, n, pose, objs)), "wall")
        res = alternate(routes)
        s = made["all"][0].get_grasp(n)
        assert (s["ik_status"] == 1).all() and (s["ik_iterations"] == 200).all(), "the grasping fleet did not run its IK to the limit"
        assert (made["none"][1].get(n)["task_state"] == 2).all() and (made["none"][0].get_grasp(n)["ik_status"] == 3).all()
        ratio = res["none"][0] / res["all"][0]
        ok = ok and ratio < 0.1
        lines.append("  %5d robots: none grasping %7.3f ms (%.3f, %.3f)   one %7.3f ms (%.3f, %.3f)   all %7.3f ms (%.3f, %.3f)   none / all = %.4f %s"
                     % ((n,) + res["none"] + res["one"] + res["all"] + (ratio, "< 0.1: holds" if ratio < 0.1 else ">= 0.1: DOES NOT HOLD")))
        if "host" in res:
            lines.append("               the host route for the 64 tracking robots (get_grasp, get, the NumPy oracle, upload): %.3f ms (%.3f, %.3f): x%.0f of the tick"
                         % (res["host"] + (res["host"][0] / res["none"][0],)))
        for h, f, _ in made.values():
            f.close()
            h.close()
    # ---- marker points: the device route against the host route ---------------------------------------------------------------------
    from alore_legged_manipulator_amd import arm, task_fsm
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    from alore_legged_manipulator_amd.flat_traj import monte_carlo_goals
    try:
        from oracle.backend_driver import EsdfGrid
        n, panels = 64, 3
        fts = monte_carlo_goals(n, seed=9)
        grid = EsdfGrid.free(half=20.0)
        pl = BatchedMSPlanner(n, 16)
        pl.set_map(grid.dist, grid.x_lo, grid.y_lo, grid.res)
        res = pl.minco_plan(fts)
        per = pl.P * (panels + 1)
        h = arm.BatchedArm(n)
        f = task_fsm.BatchedTaskFsm(h, 2, 1, per)
        view = f.view()
        xy = torch.zeros((n, per, 2), dtype=torch.float64, device="cuda")
        npts = torch.zeros(n, dtype=torch.int32, device="cuda")

        def device_route():
            view["task_state"].fill_(task_fsm.WAIT_ROBOT_PATH)
            pl.path_points_device(xy, npts, None, panels)
            f.set_paths(xy, npts)

        def host_route():
            view["task_state"].fill_(task_fsm.WAIT_ROBOT_PATH)
            got = pl.path_points(panels)
            hx, hn = np.zeros((n, per, 2)), np.zeros(n, np.int32)
            for b, (p, _) in enumerate(got):
                hx[b, :len(p)], hn[b] = p, len(p)
            f.set_paths(hx, hn)

        r = alternate({"device": (device_route, "event"), "host": (host_route, "wall")})
        lines.append("marker points of %d plans (%d accepted) into the FSM, %d panels per piece:" % (n, int(res["ok"].sum()), panels))
        lines.append("  path_points_device -> set_paths, one stream: %.3f ms (%.3f, %.3f)   path_points -> NumPy -> set_paths from the host: %.3f ms (%.3f, %.3f)"
                     % (r["device"] + r["host"]))
        f.close()
        h.close()
    except Exception as e:  # the planner's oracle library is the only optional piece
        lines.append("marker points: NOT MEASURED (%s: %s)" % (type(e).__name__, e))
    lines.append("condition (a tick with no robot grasping below a tenth of a tick with all grasping): %s" % ("holds" if ok else "DOES NOT HOLD"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
