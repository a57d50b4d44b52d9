#!/usr/bin/env python3
"""Times the resident occupancy map on one GPU: an 800 x 800 map at 0.1 m (the launch file's +-40 m), detection range 27 m, lidar-
like clouds of 360, 4096 and 65536 points (a room of walls 8-22 m away, a tenth of the rays beyond the range), the sensor near the
middle.  Prints what profiles/map_integrate.txt records.

  whole        map_integrate (one scan, ESDF included), device points, HIP events on a stream
  no ESDF      the same with update_esdf = 0: the ray kernel and the two cell kernels
  cells        a scan with no points: the two cell kernels alone (the ray kernel is the difference to the line above)
  ESDF         map_update_esdf alone in the scan's window
  perspective  map_integrate in perspective mode without the ESDF: the window kernel and the points kernel
  host         the same scans through csrc/occupancy_update.h built with g++ -O2 (tools/micro/occupancy_host.cpp), one core of the
               same box, no ESDF

usage: tools/map_integrate.py [runs]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NX = NY = 800
RES, LO, RANGE = 0.1, -40.0, 27.0
POSE = (1.37, -2.21, 0.3)


def cloud(n, seed=3):
    rng = np.random.default_rng(seed)
    ang = np.linspace(-np.pi, np.pi, n, endpoint=False)
    r = 15.0 + 7.0 * np.sin(3 * ang) * np.cos(5 * ang)            # walls 8 .. 22 m away
    r = np.where(rng.uniform(size=n) < 0.1, 60.0, r)              # no return within the range
    return np.stack([POSE[0] + r * np.cos(ang), POSE[1] + r * np.sin(ang)], 1).astype(np.float32)


def spread(v):
    v = np.asarray(v, np.float64)
    return f"median {np.median(v):.4g}  min {v.min():.4g}  max {v.max():.4g}  (n = {len(v)})"


def host_times(pts, perspective, runs, exe, tmp):
    path = os.path.join(tmp, "points.bin")
    pts.tofile(path)
    out = subprocess.check_output([exe, path, str(NX), str(NY), repr(LO), repr(LO), repr(RES), repr(RANGE), str(int(perspective)),
                                   repr(POSE[0]), repr(POSE[1]), str(runs)], text=True).split("\n")
    return [float(v) for v in out[0].split()], int(out[1])


def main():
    import torch
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    s = torch.cuda.Stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); fn(); e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    def series(fn):
        timed(fn)
        return [timed(fn) for _ in range(runs)]

    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "occupancy_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc"),
                           os.path.join(ROOT, "tools", "micro", "occupancy_host.cpp"), "-o", exe])
    print(f"map {NX} x {NY} at {RES} m, detection range {RANGE} m, sensor at {POSE[:2]}; {runs} runs after one warm-up, times in us")
    ray = BatchedMSPlanner(1, 16)
    ray.map_create(NX, NY, LO, LO, RES, detection_range=RANGE, perspective=0)
    per = BatchedMSPlanner(1, 16)
    per.map_create(NX, NY, LO, LO, RES, detection_range=RANGE, perspective=1)
    none = torch.zeros((0, 2), dtype=torch.float32, device="cuda")
    for n in (360, 4096, 65536):
        pts = cloud(n)
        d = torch.from_numpy(pts).cuda()
        torch.cuda.synchronize()
        whole = series(lambda: ray.map_integrate([(d, POSE)], update_esdf=True, stream=s))
        no_esdf = series(lambda: ray.map_integrate([(d, POSE)], update_esdf=False, stream=s))
        cells = series(lambda: ray.map_integrate([(none, POSE)], update_esdf=False, stream=s))
        esdf = series(lambda: ray.map_update_esdf(POSE, stream=s))
        persp = series(lambda: per.map_integrate([(d, POSE)], update_esdf=False, stream=s))
        host, occupied = host_times(pts, False, runs + 1, exe, tmp)
        host_p, _ = host_times(pts, True, runs + 1, exe, tmp)
        st = ray.map_state()
        print(f"\n{n} points; occupied cells after all scans so far {int((st['grid'] == 2).sum())} (the map keeps accumulating over the runs)")
        print(f"  whole map_integrate, ESDF included: {spread(whole)}")
        print(f"  no ESDF (ray + cell kernels):       {spread(no_esdf)}")
        print(f"  cell kernels alone (no points):     {spread(cells)}")
        print(f"  ray kernel (difference of medians): {np.median(no_esdf) - np.median(cells):.4g}")
        print(f"  ESDF alone (map_update_esdf):       {spread(esdf)}   share of the whole {100.0 * np.median(esdf) / np.median(whole):.0f} %")
        print(f"  perspective mode, no ESDF:          {spread(persp)}")
        print(f"  host, one core, raycast, no ESDF:   {spread(host[1:])}")
        print(f"  host, one core, perspective:        {spread(host_p[1:])}")


if __name__ == "__main__":
    main()
