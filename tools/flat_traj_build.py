#!/usr/bin/env python3
"""Times the device FlatTrajData builder and the masked replan on one GPU, for the 8192 Monte-Carlo goals of configs[4]
(flat_traj.monte_carlo_goals: two-point paths, 3-8 m).  Prints what profiles/flat_traj_build.txt records.

  device route   set_paths_device (build_problems_kernel + launch_order_kernel), inputs resident, HIP events on a stream
  host route     what it replaces on the same box: monte_carlo_goals (NumPy, one path at a time) + set_problems, wall clock
  masked replan  after a map change (a disc in the middle of the start area): check_plans, then set_paths_device + plan with the
                 check slab as the mask (HIP events around the two), against planning all slots again

usage: tools/flat_traj_build.py [count] [runs]"""
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def goals_as_paths(count, seed=20260206):
    """the draws of flat_traj.monte_carlo_goals as path arrays"""
    rng = np.random.default_rng(seed)
    xy, sy, ey = np.zeros((count, 3, 2)), np.zeros(count), np.zeros(count)
    for b in range(count):
        sx, s_y = rng.uniform(-5, 5, 2)
        sy[b] = rng.uniform(-math.pi, math.pi)
        dist, bearing = rng.uniform(3.0, 8.0), rng.uniform(-math.pi, math.pi)
        ey[b] = rng.uniform(-math.pi, math.pi)
        xy[b, 0] = (sx, s_y)
        xy[b, 1] = (sx + dist * math.cos(bearing), s_y + dist * math.sin(bearing))
    return xy, sy, ey


def spread(v):
    v = np.asarray(v, np.float64)
    return f"median {np.median(v):.4g}  min {v.min():.4g}  max {v.max():.4g}  (n = {len(v)})"


def main():
    import torch
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    from alore_legged_manipulator_amd.flat_traj import monte_carlo_goals
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    pl = BatchedMSPlanner(B, 16)
    half, res = 20.0, 0.1
    n = int(round(2 * half / res))
    pl.set_map(np.full((n, n), 100.0), -half, -half, res)
    xy, sy, ey = goals_as_paths(B)
    s = torch.cuda.Stream()
    d_n = torch.full((B,), 2, dtype=torch.int32, device="cuda")
    d_xy, d_sy, d_ey = torch.from_numpy(xy).cuda(), torch.from_numpy(sy).cuda(), torch.from_numpy(ey).cuda()
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); fn(); e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    build = lambda: pl.set_paths_device(B, 3, d_n, d_xy, d_sy, d_ey, stream=s)
    timed(build)
    dev_us = [timed(build) for _ in range(runs)]
    host_issue_us = []
    for _ in range(runs):
        t0 = time.perf_counter(); build(); host_issue_us.append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()
    status = pl.build_status()
    dev = pl.problems()
    print(f"B = {B}; built {int((status == 0).sum())}, status histogram {dict(zip(*np.unique(status, return_counts=True)))}")
    print(f"device route, set_paths_device + launch order [us, HIP events]: {spread(dev_us)}")
    print(f"device route, host time of the call [us]: {spread(host_issue_us)}")

    host_ms, front_ms, upload_ms = [], [], []
    for _ in range(runs):
        t0 = time.perf_counter(); trajs = monte_carlo_goals(B); t1 = time.perf_counter(); pl.set_problems(trajs); t2 = time.perf_counter()
        front_ms.append((t1 - t0) * 1e3); upload_ms.append((t2 - t1) * 1e3); host_ms.append((t2 - t0) * 1e3)
    print(f"host route, monte_carlo_goals + set_problems [ms, wall]: {spread(host_ms)}")
    print(f"  of which monte_carlo_goals [ms]: {spread(front_ms)};  set_problems [ms]: {spread(upload_ms)}")
    hp = pl.problems()
    print(f"device-built against host-built slots: piece counts differ in {int((hp['n_pieces'] != dev['n_pieces']).sum())} of {B}, "
          f"max |difference| of the other fields {max(float(np.abs(hp[k] - dev[k]).max()) for k in ('inner', 'init_T', 'positions', 'head', 'tail')):.3g}")

    # ---- masked replan
    build(); torch.cuda.synchronize()
    all_ms = []
    for _ in range(runs):
        pl.plan(stream=s); all_ms.append(pl.last_plan_ms())
    c = (np.arange(n) + 0.5) * res - half
    X, Y = np.meshgrid(c, c, indexing="ij")
    for radius in (0.5, 1.5):
        pl.set_map(np.minimum(np.hypot(X, Y) - radius, 100.0), -half, -half, res)
        flags = pl.check_plans()["collision"].astype(bool)
        # detour: a way-point 1 m to the left of the middle of the segment, from the state predicted at 0.5 s
        mid = 0.5 * (xy[:, 0] + xy[:, 1])
        d = xy[:, 1] - xy[:, 0]
        left = np.stack([-d[:, 1], d[:, 0]], 1) / np.linalg.norm(d, axis=1, keepdims=True)
        det = np.stack([xy[:, 0], mid + left, xy[:, 1]], 1)
        t_xy = torch.from_numpy(det).cuda()
        t_n = torch.full((B,), 3, dtype=torch.int32, device="cuda")
        times = torch.full((B,), 0.5, dtype=torch.float64, device="cuda")
        xyt, vaj, oaj = (torch.zeros(B, 3, dtype=torch.float64, device="cuda") for _ in range(3))
        fwd = torch.zeros(B, dtype=torch.int32, device="cuda")
        syd = torch.zeros(B, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rebuild_us, replan_ms = [], []
        for _ in range(runs):
            with torch.cuda.stream(s):
                # the mask stays the slab of the check above: every run rebuilds and replans the same slots
                pl.predicted_state_device(B, times, xyt, vaj, oaj, fwd, 0.01, stream=s)
                t_xy[:, 0, :] = xyt[:, :2]
                syd.copy_(xyt[:, 2])
                rebuild_us.append(timed(lambda: pl.set_paths_device(B, 3, t_n, t_xy, syd, d_ey, vaj, oaj, mask=pl.check_mask(), stream=s)))
                pl.plan(mask=pl.check_mask(), stream=s)
            replan_ms.append(pl.last_plan_ms())
        st = pl.build_status()
        print(f"map change (disc of radius {radius} m at the origin): {int(flags.sum())} of {B} plans flagged ({100.0 * flags.mean():.1f} %); "
              f"rebuilt {int((st == 0).sum())}, too many pieces {int((st == -2).sum())}")
        print(f"  masked rebuild [us]: {spread(rebuild_us)}")
        print(f"  masked plan launch [ms]: {spread(replan_ms)}")
    print(f"planning all {B} slots again [ms]: {spread(all_ms)}")


if __name__ == "__main__":
    main()
