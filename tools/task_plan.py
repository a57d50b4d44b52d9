#!/usr/bin/env python3
"""Times the task planning of rearrangement missions on one GPU: the 800 x 800 map at 0.1 m with discs of tools/path_search.py, 512
missions of n = 5 and of n = 10 tasks with all points inside a 10 m box and 0.4 m clear of the discs, both modes.  Prints what profiles/task_plan.txt records.

  device   task_plan_device, both kernels (HIP events), and the fields / sweeps diagnostics
  host     the same missions through csrc/task_plan.h built with g++ -O2 (tools/micro/task_plan_host.cpp), one core
  pairs    what could be done before: the P (P - 1) / 2 pair searches of each mission through search_paths_device on the same GPU
           (each in its own, smaller window), in launches of at most 8192

usage: tools/task_plan.py [missions] [runs] [host missions]"""
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


if __name__ == "__main__":
    main()
