#!/usr/bin/env python3
"""Times the grid search for way-point paths on one GPU and closes the replan cycle with it: an 800 x 800 map at 0.1 m (+-40 m),
the 8192 Monte-Carlo goals of tools/flat_traj_build.py (two-point paths, 3-8 m, starts within +-5 m) planned on the free map, then
discs appear in the start area.  Prints what profiles/path_search.txt records.

  flagged      check_plans, then search_paths_device with the check slab as the mask, from the state predicted at 0.5 s (HIP events)
  all          search_paths_device for all slots, from the start positions
  host         the same problems through csrc/path_search.h built with g++ -O2 (tools/micro/path_search_host.cpp), one core
  cycle        set_paths_device on the searched slab and plan with the same mask; then check_plans again: how many of the flagged
               slots' new plans pass (an observation about the optimiser, not a property of the search)

usage: tools/path_search.py [count] [runs] [host problems]

tools/path_search.py wide [runs] [host problems] [library of the parent commit] times the route for windows beyond LDS
(alore_backend_search_reserve) on the same map and prints what profiles/path_search_wide.txt records: 256 and 2048 problems with
end points 20 to 60 m apart and a 10 m margin, the visits of tiles, the share of the walk and pruning, the same header on one
host core (tools/micro/path_search_wide_host.cpp), and what a reservation costs the 8192-goal call that has no wide slot."""
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


# ---- windows beyond LDS (alore_backend_search_reserve): tools/path_search.py wide [runs] [host problems] [library of the parent commit]
WIDE_MARGIN = 10.0


def wide_problems(dist, n, seed=11):
    """end points within +-38 m, 20 to 60 m apart, both at least 0.5 m from a disc"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        p = rng.uniform(-38.0, 38.0, 4)
        if not 20.0 <= np.hypot(p[2] - p[0], p[3] - p[1]) <= 60.0:
            continue
        c = ((p - LO) / RES).astype(int)
        if dist[c[0], c[1]] >= 0.5 and dist[c[2], c[3]] >= 0.5:
            out.append(p)
    return np.array(out)


def planner_of(lib_path, B):
    """a planner on another build of the library in this process (the parent commit's, which lacks the reservation calls)"""
    import ctypes as C
    from alore_legged_manipulator_amd import _lib, backend
    ours = _lib.load()
    other = C.CDLL(lib_path)
    for name, res, args in _lib.SYMBOLS:
        fn = getattr(other, name)
        fn.restype, fn.argtypes = res, args
    for name in ("alore_backend_search_reserve", "alore_backend_search_reserved", "alore_backend_search_wide_ticks"):
        if not hasattr(other, name):
            setattr(other, name, getattr(ours, name))   # never called on that planner
    _lib._lib = other
    try:
        return backend.BatchedMSPlanner(B, 16)
    finally:
        _lib._lib = ours


def wide_main():
    import torch
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    from flat_traj_build import goals_as_paths
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    n_host = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    parent = sys.argv[4] if len(sys.argv) > 4 else None
    dist = disc_map()
    s = torch.cuda.Stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); fn(); e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)  # ms

    # ---- throughput of the wide route
    N, SLOTS, CELLS = 2048, 256, NX * NY
    prob = wide_problems(dist, N)
    cells = ((np.abs(prob[:, 2] - prob[:, 0]) + 2 * WIDE_MARGIN) / RES).clip(max=NX) * ((np.abs(prob[:, 3] - prob[:, 1]) + 2 * WIDE_MARGIN) / RES).clip(max=NY)
    pl = BatchedMSPlanner(N, 16)
    pl.set_map(dist, LO, LO, RES)
    pl.search_reserve(CELLS, SLOTS)
    d_start, d_goal = torch.from_numpy(np.ascontiguousarray(prob[:, :2])).cuda(), torch.from_numpy(np.ascontiguousarray(prob[:, 2:])).cuda()
    torch.cuda.synchronize()
    print(f"wide route: map {NX} x {NY} at {RES} m, end points 20 to 60 m apart, window_margin {WIDE_MARGIN}; reservation {CELLS} cells x {SLOTS} "
          f"slabs; windows of about {np.median(cells):.0f} cells (median), {cells.max():.0f} (max); {runs} runs after one warm-up")
    for n in (256, N):
        go = lambda: pl.search_paths_device(n, d_start, d_goal, window_margin=WIDE_MARGIN, stream=s)
        timed(go)
        ms = [timed(go) for _ in range(runs)]
        st, visits, ticks, paths = pl.search_status(n), pl.search_sweeps(n), pl.search_wide_ticks(n), pl.paths(n)
        share = ticks[:, 1] / np.maximum(ticks[:, 0], 1)
        print(f"search of {n} wide slots [ms, HIP events]: {spread(ms)}; {np.median(ms) / n:.4g} ms per problem amortised")
        print(f"  status histogram {histogram(st)}; way-points median {np.median(paths['n_points'][st == 0]):.0f}, max {paths['n_points'].max()}; "
              f"visits of tiles: median {np.median(visits):.0f}, max {visits.max()}")
        print(f"  per slot in its workgroup [ms, 100 MHz device clock]: {spread(ticks[:, 0] / 1e5)}")
        print(f"  walk and pruning by thread 0, share of the slot's time: median {np.median(share):.3f}, max {share.max():.3f}; "
              f"of the summed time {ticks[:, 1].sum() / ticks[:, 0].sum():.3f}")
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "path_search_wide_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc"),
                           os.path.join(ROOT, "tools", "micro", "path_search_wide_host.cpp"), "-o", exe])
    dist.tofile(os.path.join(tmp, "map.bin"))
    m = min(n_host, N)
    np.ascontiguousarray(prob[:m]).tofile(os.path.join(tmp, "problems.bin"))
    out = subprocess.check_output([exe, os.path.join(tmp, "map.bin"), str(NX), str(NY), repr(LO), repr(LO), repr(RES),
                                   os.path.join(tmp, "problems.bin"), "0.3", repr(WIDE_MARGIN), str(CELLS)], text=True).split("\n")
    n, total_us, host_visits = out[0].split()
    print(f"host, one core, search_one_wide with tiles of 126 x 126, the first {n} of the same problems: {float(total_us) / 1e3:.4g} ms, "
          f"{float(total_us) / int(n) / 1e3:.4g} ms per problem (statuses 0 .. -6: {out[1].strip()}; most visits {host_visits})")
    del pl

    # ---- what a reservation costs a call without wide slots: the 8192 goals of the narrow run
    B = 8192
    xy, _, _ = goals_as_paths(B)
    g_start, g_goal = torch.from_numpy(np.ascontiguousarray(xy[:, 0])).cuda(), torch.from_numpy(np.ascontiguousarray(xy[:, 1])).cuda()
    handles = {"unreserved": BatchedMSPlanner(B, 16), "reserved": BatchedMSPlanner(B, 16)}
    handles["reserved"].search_reserve(80000, SLOTS)
    if parent:
        handles["parent"] = planner_of(parent, B)
    for h in handles.values():
        h.set_map(dist, LO, LO, RES)
    torch.cuda.synchronize()
    ms = {k: [] for k in handles}
    for r in range(2 * runs + 2):
        for k, h in handles.items():
            t = timed(lambda: h.search_paths_device(B, g_start, g_goal, stream=s))
            if r >= 1:
                ms[k].append(t)
    print(f"narrow call, {B} goals, handles alternating in one process (reservation 80000 cells x {SLOTS} slabs):")
    for k, v in ms.items():
        print(f"  {k:<10} [ms]: {spread(v)}")
    ref = handles["unreserved"].paths(B)
    for k, h in handles.items():
        got = h.paths(B)
        same = all(got[q].tobytes() == ref[q].tobytes() for q in ("n_points", "xy", "cost_ab")) and (h.search_status(B) == handles["unreserved"].search_status(B)).all()
        print(f"  {k:<10} slab of paths and statuses bit-equal to the unreserved handle's: {same}")


if __name__ == "__main__":
    wide_main() if len(sys.argv) > 1 and sys.argv[1] == "wide" else main()
