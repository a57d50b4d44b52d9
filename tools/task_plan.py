#!/usr/bin/env python3
"""Times the task planning of rearrangement missions on one GPU: the 800 x 800 map at 0.1 m with discs of tools/path_search.py, 512
missions of n = 5 and of n = 10 tasks with all points inside a 10 m box and 0.4 m clear of the discs, both modes.  Prints what profiles/task_plan.txt records.

  device   task_plan_device, both kernels (HIP events), and the fields / sweeps diagnostics
  host     the same missions through csrc/task_plan.h built with g++ -O2 (tools/micro/task_plan_host.cpp), one core
  pairs    what could be done before: the P (P - 1) / 2 pair searches of each mission through search_paths_device on the same GPU
           (each in its own, smaller window), in launches of at most 8192

usage: tools/task_plan.py [missions] [runs] [host missions]

tools/task_plan.py wide [runs] [host missions] [library of the parent commit] times missions on windows beyond LDS
(alore_backend_task_reserve) on the same map and prints what profiles/task_plan_wide.txt records: 64 and 512 missions of n = 5 whose
points span 20 to 60 m, window_margin 10 m, on 256 slabs; the same header on one host core; the 55 pair searches per mission on
the wide route of the search; and what a task reservation costs the 512-mission call above, against the parent commit's library."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from path_search import LO, NX, NY, RES, disc_map, histogram, spread  # noqa: E402

BATCH = 8192
HOST_REPS = 5


def main():
    import torch
    from alore_legged_manipulator_amd.backend import TASK_GREEDY, TASK_OPTIMAL, BatchedMSPlanner
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    n_host = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    pl = BatchedMSPlanner(BATCH, 16)
    dist = disc_map()
    pl.set_map(dist, LO, LO, RES)
    s = torch.cuda.Stream()
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "task_plan_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc"),
                           os.path.join(ROOT, "tools", "micro", "task_plan_host.cpp"), "-o", exe])
    dist.tofile(os.path.join(tmp, "map.bin"))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); fn(); e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)  # ms

    print(f"map {NX} x {NY} at {RES} m with discs; {count} missions, points inside a 10 m box; {runs} runs after one warm-up")
    for n in (5, 10):
        P = 1 + 2 * n
        rng = np.random.default_rng(100 + n)
        pts = rng.uniform(-5.0, 5.0, (count, P, 2))
        for _ in range(64):                                              # points at least 0.4 m clear of the discs: no clamp, no point inside one
            cell = np.floor((pts - LO) / RES).astype(int)
            bad = dist[cell[..., 0], cell[..., 1]] < 0.4
            if not bad.any():
                break
            pts[bad] = rng.uniform(-5.0, 5.0, (int(bad.sum()), 2))
        d_pts, d_n = torch.from_numpy(pts).cuda(), torch.full((count,), n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for mode, label in ((TASK_GREEDY, "greedy"), (TASK_OPTIMAL, "optimal")):
            call = lambda: pl.task_plan_device(count, n, d_n, d_pts, mode=mode, stream=s)
            timed(call)
            ms = [timed(call) for _ in range(runs)]
            r = pl.task_result(count)
            ok = r["status"] == 0
            print(f"n = {n}, {label}: device [ms, HIP events]: {spread(ms)}; per mission {np.median(ms) / count * 1e3:.4g} us")
            print(f"  status histogram {histogram(r['status'])}; fields per mission: median {np.median(r['fields'])}, max {r['fields'].max()} "
                  f"(P - 1 = {P - 1}; more than that in {int((r['fields'] > P - 1).sum())} missions); sweeps of the slowest field: "
                  f"median {np.median(r['sweeps'])}, max {r['sweeps'].max()}; missions with a pair without a path: "
                  f"{int((r['matrix'][:, :P, :P, 0] < 0).any(axis=(1, 2)).sum())}; legs in the orders of the ok missions: median "
                  f"{np.median(r['n_order'][ok]) if ok.any() else 0}")
            m = min(n_host, count)
            pts[:m].tofile(os.path.join(tmp, "missions.bin"))
            reps = [subprocess.check_output([exe, os.path.join(tmp, "map.bin"), str(NX), str(NY), repr(LO), repr(LO), repr(RES),
                                             os.path.join(tmp, "missions.bin"), str(n), str(mode), "0.3", "3.0"], text=True).split()
                    for _ in range(HOST_REPS)]
            out, us = reps[0], float(np.median([float(r[1]) for r in reps]))
            print(f"  host, one core, the first {out[0]} of the same missions, median of {HOST_REPS} runs "
                  f"({', '.join('%.4g' % (float(r[1]) / 1e3) for r in reps)} ms): {us / 1e3:.4g} ms, {us / int(out[0]) / 1e3:.4g} ms per mission "
                  f"(fields {out[2]}, most sweeps {out[3]}, ok {out[4]}, no order {out[5]}); scaled to {count}: {us / int(out[0]) * count / 1e3:.4g} ms")
        # the pair searches of every mission, as alore_backend_search_paths does them
        i, j = np.triu_indices(P, 1)
        starts, goals = np.ascontiguousarray(pts[:, i].reshape(-1, 2)), np.ascontiguousarray(pts[:, j].reshape(-1, 2))
        d_s, d_g = torch.from_numpy(starts).cuda(), torch.from_numpy(goals).cuda()
        torch.cuda.synchronize()
        total = len(starts)

        def pairs():
            for at in range(0, total, BATCH):
                k = min(BATCH, total - at)
                pl.search_paths_device(k, d_s[at:at + k], d_g[at:at + k], stream=s)
        timed(pairs)
        ms = [timed(pairs) for _ in range(runs)]
        print(f"n = {n}: the {total} pair searches ({P * (P - 1) // 2} per mission) in launches of {BATCH} [ms]: {spread(ms)}; "
              f"per mission {np.median(ms) / count * 1e3:.4g} us")


# ---- windows beyond LDS (alore_backend_task_reserve): tools/task_plan.py wide [runs] [host missions] [library of the parent commit]
NEW_CALLS = ("alore_backend_search_reserve", "alore_backend_search_reserved", "alore_backend_search_wide_ticks", "alore_backend_task_reserve",
             "alore_backend_task_reserved", "alore_backend_task_wide_ticks")


def planner_of(lib_path, B):
    """a planner on another build of the library in this process (the parent commit's, which lacks the task reservation)"""
    import ctypes as C
    from alore_legged_manipulator_amd import _lib, backend
    ours = _lib.load()
    other = C.CDLL(lib_path)
    for name, res, args in _lib.SYMBOLS:
        fn = getattr(other, name)
        fn.restype, fn.argtypes = res, args
    for name in NEW_CALLS:
        if not hasattr(other, name):
            setattr(other, name, getattr(ours, name))   # never called on that planner
    _lib._lib = other
    try:
        return backend.BatchedMSPlanner(B, 16)
    finally:
        _lib._lib = ours


def wide_missions(dist, count, n, seed=21):
    """missions whose windows are those of tools/path_search.py wide: two anchor points 20 to 60 m apart (the robot and the last
    target), the other points anywhere in their bounding box, all at least 0.5 m from a disc"""
    from path_search import wide_problems
    rng = np.random.default_rng(seed)
    anchors = wide_problems(dist, count)
    P = 1 + 2 * n
    pts = np.zeros((count, P, 2))
    for m, a in enumerate(anchors):
        lo, hi = np.minimum(a[:2], a[2:]), np.maximum(a[:2], a[2:])
        pts[m, 0], pts[m, P - 1] = a[:2], a[2:]
        for k in range(1, P - 1):
            while True:
                q = rng.uniform(lo, hi)
                c = ((q - LO) / RES).astype(int)
                if dist[c[0], c[1]] >= 0.5:
                    break
            pts[m, k] = q
    return pts


def wide_main():
    import torch
    from alore_legged_manipulator_amd.backend import TASK_GREEDY, BatchedMSPlanner
    from path_search import WIDE_MARGIN
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    n_host = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    parent = sys.argv[4] if len(sys.argv) > 4 else None
    dist = disc_map()
    s = torch.cuda.Stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); fn(); e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)  # ms

    N, n, SLOTS, CELLS = 512, 5, 256, NX * NY
    P = 1 + 2 * n
    pts = wide_missions(dist, N, n)
    span = (pts.max(axis=1) - pts.min(axis=1) + 2 * WIDE_MARGIN) / RES
    cells = span[:, 0].clip(max=NX) * span[:, 1].clip(max=NY)
    pl = BatchedMSPlanner(max(N * P * (P - 1) // 2 // 8, N), 16)
    pl.set_map(dist, LO, LO, RES)
    pl.task_reserve(CELLS, SLOTS)
    d_pts, d_n = torch.from_numpy(pts).cuda(), torch.full((N,), n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    print(f"wide missions: map {NX} x {NY} at {RES} m, n = {n}, points spanning 20 to 60 m, window_margin {WIDE_MARGIN}; reservation {CELLS} cells x "
          f"{SLOTS} slabs; windows of about {np.median(cells):.0f} cells (median), {cells.max():.0f} (max); {runs} runs after one warm-up")
    for count in (64, N):
        go = lambda: pl.task_plan_device(count, n, d_n, d_pts, mode=TASK_GREEDY, window_margin=WIDE_MARGIN, stream=s)
        timed(go)
        ms = [timed(go) for _ in range(runs)]
        order_ms = [timed(lambda: pl.task_reorder(stream=s)) for _ in range(runs)]
        r, ticks = pl.task_result(count), pl.task_wide_ticks(count)[:, :P - 1]
        busy = np.zeros(SLOTS)
        np.add.at(busy, (np.arange(count)[:, None] * 2 * n + np.arange(P - 1)[None, :]).reshape(-1) % SLOTS, ticks.reshape(-1))
        print(f"{count} missions, greedy: the whole call [ms, HIP events]: {spread(ms)}; per mission {np.median(ms) / count:.4g} ms; the order "
              f"phase alone (task_reorder) {np.median(order_ms):.4g} ms")
        print(f"  the wide kernel alone, the busiest workgroup's sources summed [ms, 100 MHz device clock]: {busy.max() / 1e5:.4g}; the least busy "
              f"{busy.min() / 1e5:.4g}")
        print(f"  status histogram {histogram(r['status'])}; fields per mission: median {np.median(r['fields'])}, max {r['fields'].max()} "
              f"(P - 1 = {P - 1}); visits of tiles of the slowest field per mission: median {np.median(r['sweeps'])}, max {r['sweeps'].max()}")
        print(f"  per source (its fields, {r['fields'].sum() / ticks.size:.3g} on average) in its workgroup [ms]: {spread(ticks.reshape(-1) / 1e5)}")
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "task_plan_wide_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc"),
                           os.path.join(ROOT, "tools", "micro", "task_plan_wide_host.cpp"), "-o", exe])
    dist.tofile(os.path.join(tmp, "map.bin"))
    m = min(n_host, N)
    pts[:m].tofile(os.path.join(tmp, "missions.bin"))
    out = subprocess.check_output([exe, os.path.join(tmp, "map.bin"), str(NX), str(NY), repr(LO), repr(LO), repr(RES), os.path.join(tmp, "missions.bin"),
                                   str(n), str(TASK_GREEDY), "0.3", repr(WIDE_MARGIN), str(CELLS)], text=True).split()
    us = float(out[1])
    print(f"host, one core, plan_one_wide with tiles of 126 x 126, the first {out[0]} of the same missions: {us / 1e3:.4g} ms, "
          f"{us / int(out[0]) / 1e3:.4g} ms per mission, {us / max(int(out[2]), 1) / 1e3:.4g} ms per field (fields {out[2]}, most visits {out[3]}, ok {out[4]}, "
          f"range {out[5]}); scaled to {N}: {us / int(out[0]) * N / 1e3:.4g} ms")
    # the only device route there was: the P (P - 1) / 2 pair searches of each mission on the wide route of the search
    pl.task_reserve(0, 0)
    pl.search_reserve(CELLS, SLOTS)
    i, j = np.triu_indices(P, 1)
    for count in (64, N):
        starts, goals = np.ascontiguousarray(pts[:count, i].reshape(-1, 2)), np.ascontiguousarray(pts[:count, j].reshape(-1, 2))
        d_s, d_g = torch.from_numpy(starts).cuda(), torch.from_numpy(goals).cuda()
        torch.cuda.synchronize()
        total, batch = len(starts), pl.B

        def pairs():
            for at in range(0, total, batch):
                k = min(batch, total - at)
                pl.search_paths_device(k, d_s[at:at + k], d_g[at:at + k], window_margin=WIDE_MARGIN, stream=s)
        ms = [timed(pairs) for _ in range(2)]
        print(f"{count} missions: the {total} pair searches ({P * (P - 1) // 2} per mission, each in its own window) through search_paths_device "
              f"on {SLOTS} slabs, launches of {batch} [ms]: {spread(ms)}; per mission {np.median(ms) / count:.4g} ms")
    del pl

    # ---- what a task reservation costs a call without wide missions: the 512 missions of n = 5 of the narrow run
    count = 512
    rng = np.random.default_rng(100 + n)
    near = rng.uniform(-5.0, 5.0, (count, P, 2))
    for _ in range(64):
        cell = np.floor((near - LO) / RES).astype(int)
        bad = dist[cell[..., 0], cell[..., 1]] < 0.4
        if not bad.any():
            break
        near[bad] = rng.uniform(-5.0, 5.0, (int(bad.sum()), 2))
    g_pts = torch.from_numpy(near).cuda()
    handles = {"unreserved": BatchedMSPlanner(count, 16), "reserved": BatchedMSPlanner(count, 16)}
    handles["reserved"].task_reserve(80000, SLOTS)
    if parent:
        handles["parent"] = planner_of(parent, count)
    for h in handles.values():
        h.set_map(dist, LO, LO, RES)
    torch.cuda.synchronize()
    ms = {k: [] for k in handles}
    for r in range(4 * runs + 2):
        for k, h in handles.items():
            t = timed(lambda: h.task_plan_device(count, n, d_n, g_pts, mode=TASK_GREEDY, stream=s))
            if r >= 2:
                ms[k].append(t)
    print(f"narrow call, {count} missions of n = {n} inside a 10 m box, greedy, handles alternating in one process (reservation 80000 cells x {SLOTS} slabs):")
    for k, v in ms.items():
        print(f"  {k:<10} [ms]: {spread(v)}")
    if parent:
        lo, hi = min(ms["parent"]), max(ms["parent"])
        for k in ("unreserved", "reserved"):
            print(f"  median of {k} inside the parent's own range [{lo:.4g}, {hi:.4g}] ms: {lo <= np.median(ms[k]) <= hi}")
    ref = handles["unreserved"].task_result(count)
    for k, h in handles.items():
        got = h.task_result(count)
        same = all(got[q].tobytes() == ref[q].tobytes() for q in ("status", "matrix", "order", "n_order", "total", "leg_start_xy", "leg_goal_xy", "fields"))
        print(f"  {k:<10} slab of missions bit-equal to the unreserved handle's (all but the sweep counts of the LDS kernel, which depend on "
              f"the timing of its wavefronts: {int((got['sweeps'] != ref['sweeps']).sum())} of {count} differ): {same}")


if __name__ == "__main__":
    wide_main() if len(sys.argv) > 1 and sys.argv[1] == "wide" else main()
