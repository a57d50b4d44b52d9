#!/usr/bin/env python3
"""Times the grid search for way-point paths on one GPU and closes the replan cycle with it: an 800 x 800 map at 0.1 m (+-40 m),
the 8192 Monte-Carlo goals of tools/flat_traj_build.py (two-point paths, 3-8 m, starts within +-5 m) planned on the free map, then
discs appear in the start area.  Prints what profiles/path_search.txt records.

  flagged      check_plans, then search_paths_device with the check slab as the mask, from the state predicted at 0.5 s (HIP events)
  all          search_paths_device for all slots, from the start positions
  host         the same problems through csrc/path_search.h built with g++ -O2 (tools/micro/path_search_host.cpp), one core
  cycle        set_paths_device on the searched slab and plan with the same mask; then check_plans again: how many of the flagged
               slots' new plans pass (an observation about the optimiser, not a property of the search)

usage: tools/path_search.py [count] [runs] [host problems]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
NX = NY = 800
RES, LO = 0.1, -40.0


def disc_map(seed=5, discs=14):
    rng = np.random.default_rng(seed)
    c = (np.arange(NX) + 0.5) * RES + LO
    X, Y = np.meshgrid(c, c, indexing="ij")
    d = np.full((NX, NY), 100.0)
    for _ in range(discs):
        cx, cy, r = rng.uniform(-9, 9), rng.uniform(-9, 9), rng.uniform(0.4, 1.5)
        d = np.minimum(d, np.hypot(X - cx, Y - cy) - r)
    return d


def spread(v):
    v = np.asarray(v, np.float64)
    return f"median {np.median(v):.4g}  min {v.min():.4g}  max {v.max():.4g}  (n = {len(v)})"


def histogram(st):
    return {int(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))}


def main():
    import torch
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    from flat_traj_build import goals_as_paths
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    n_host = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    pl = BatchedMSPlanner(B, 16)
    pl.set_map(np.full((NX, NY), 100.0), LO, LO, RES)
    xy, sy, ey = goals_as_paths(B)
    s = torch.cuda.Stream()
    d_n = torch.full((B,), 2, dtype=torch.int32, device="cuda")
    d_xy, d_sy, d_ey = torch.from_numpy(xy).cuda(), torch.from_numpy(sy).cuda(), torch.from_numpy(ey).cuda()
    d_start, d_goal = torch.from_numpy(np.ascontiguousarray(xy[:, 0])).cuda(), torch.from_numpy(np.ascontiguousarray(xy[:, 1])).cuda()
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); fn(); e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)  # ms

    pl.set_paths_device(B, 3, d_n, d_xy, d_sy, d_ey, stream=s)
    pl.plan(stream=s)
    print(f"map {NX} x {NY} at {RES} m; B = {B}; planning all slots on the free map {pl.last_plan_ms():.4g} ms; {runs} runs after one warm-up")
    dist = disc_map()
    pl.set_map(dist, LO, LO, RES)
    flags = pl.check_plans()["collision"].astype(bool)
    times = torch.full((B,), 0.5, dtype=torch.float64, device="cuda")
    xyt, vaj, oaj = (torch.zeros(B, 3, dtype=torch.float64, device="cuda") for _ in range(3))
    fwd = torch.zeros(B, dtype=torch.int32, device="cuda")
    syd = torch.zeros(B, dtype=torch.float64, device="cuda")
    pl.predicted_state_device(B, times, xyt, vaj, oaj, fwd, 0.01, stream=s)
    torch.cuda.synchronize()

    # ---- all slots, from the start positions
    search_all = lambda: pl.search_paths_device(B, d_start, d_goal, stream=s)
    timed(search_all)
    all_ms = [timed(search_all) for _ in range(runs)]
    st, sw, paths = pl.search_status(B), pl.search_sweeps(B), pl.paths(B)
    print(f"search of all {B} slots [ms, HIP events]: {spread(all_ms)}")
    print(f"  status histogram {histogram(st)}; way-points of the found paths: median {np.median(paths['n_points'][st == 0]):.0f}, "
          f"max {paths['n_points'].max()}; sweeps: median {np.median(sw[sw > 0]):.0f}, the slowest problem {sw.max()}")

    # ---- the flagged slots, from the predicted state
    search_flagged = lambda: pl.search_paths_device(B, xyt, d_goal, mask=pl.check_mask(), stream=s)
    timed(search_flagged)
    flagged_ms = [timed(search_flagged) for _ in range(runs)]
    st, sw = pl.search_status(B), pl.search_sweeps(B)
    print(f"map change ({int(flags.sum())} of {B} plans flagged, {100.0 * flags.mean():.1f} %): search of the flagged slots [ms]: {spread(flagged_ms)}")
    print(f"  status histogram {histogram(st)}; sweeps of the slowest problem {sw[flags].max() if flags.any() else 0}")

    # ---- the host, one core
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "path_search_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc"),
                           os.path.join(ROOT, "tools", "micro", "path_search_host.cpp"), "-o", exe])
    dist.tofile(os.path.join(tmp, "map.bin"))
    m = min(n_host, B)
    np.ascontiguousarray(xy[:m, :2].reshape(m, 4)).tofile(os.path.join(tmp, "problems.bin"))
    out = subprocess.check_output([exe, os.path.join(tmp, "map.bin"), str(NX), str(NY), repr(LO), repr(LO), repr(RES),
                                   os.path.join(tmp, "problems.bin"), "0.3", "3.0"], text=True).split("\n")
    n, total_us, host_sweeps = out[0].split()
    print(f"host, one core, the first {n} of the same problems: {float(total_us) / 1e3:.4g} ms, {float(total_us) / int(n):.4g} us per problem "
          f"(statuses 0 .. -5: {out[1].strip()}; most sweeps {host_sweeps}); scaled to {B}: {float(total_us) / int(n) * B / 1e3:.4g} ms")

    # ---- the cycle closed: searched paths into set_paths, masked plan, check again
    v = pl.device_paths()
    with torch.cuda.stream(s):
        syd.copy_(xyt[:, 2])
        pl.set_paths_device(B, v.max_points, v.n_points, v.xy, syd, d_ey, vaj, oaj, mask=pl.check_mask(), stream=s)
        pl.plan(mask=pl.check_mask(), stream=s)
    replan_ms = pl.last_plan_ms()
    build = pl.build_status(B)
    ok = pl.results(B)["ok"].astype(bool)
    again = pl.check_plans()["collision"].astype(bool)
    solved = flags & (st == 0)
    print(f"cycle: of {int(flags.sum())} flagged slots the search solved {int(solved.sum())}; rebuilt {int((build[solved] == 0).sum())}, "
          f"too many pieces {int((build[solved] == -2).sum())}; masked plan launch {replan_ms:.4g} ms")
    rebuilt = solved & (build == 0)
    print(f"  of the {int(rebuilt.sum())} rebuilt and replanned slots the optimiser accepted {int(ok[rebuilt].sum())}, and "
          f"{int((~again[rebuilt]).sum())} pass check_plans on the new map ({int((ok & ~again)[rebuilt].sum())} both)")


if __name__ == "__main__":
    main()
