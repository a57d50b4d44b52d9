#!/usr/bin/env python3
"""Times the edits of missions in the resident map on one GPU: an 800 x 800 map at 0.1 m (the launch file's +-40 m), 64, 512 and
4096 missions of 5 tasks spread over +-35 m, every mission heading to its first item.  Prints what profiles/mission_map.txt records.

  step         mission_step with none, a quarter and all of the robots within item_free_dist of their item (0, B / 4, B edits), poses
               in device memory: device time (HIP events on a stream) and the time until the host returns from the call
  paint        map_paint_device alone on the edit list the step left on the device
  step + ESDF  mission_step followed by map_update_esdf in a 27 m window round the origin, device time
  host route   what the calls replace: map_get (state grid) -> the same edits in NumPy (one slice per edit: cheaper than the
               reference's lattice, which favours this route) -> map_set_grid, wall time, in the same process, alternating with the
               step

usage: tools/mission_map.py [runs]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NX = NY = 800
RES, LO, RANGE, TASKS = 0.1, -40.0, 27.0, 5


def spread(v):
    v = np.asarray(v, np.float64)
    return f"median {np.median(v):9.4g}  min {v.min():9.4g}  max {v.max():9.4g}"


def numpy_edits(grid, edits):
    for e in edits:
        x0, x1 = int((e["cx"] - e["hx"] - LO) / RES), int((e["cx"] + e["hx"] - LO) / RES)
        y0, y1 = int((e["cy"] - e["hy"] - LO) / RES), int((e["cy"] + e["hy"] - LO) / RES)
        grid[max(x0, 0):x1 + 1, max(y0, 0):y1 + 1] = 2 if e["make_obs"] else 1


def main():
    import torch
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    s = torch.cuda.Stream()

    def device_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); fn(); e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def host_us(fn):
        s.synchronize()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        s.synchronize()
        return (t1 - t0) * 1e6

    print(f"map {NX} x {NY} at {RES} m, {TASKS} tasks per mission, {runs} runs each, times in microseconds")
    for B in (64, 512, 4096):
        rng = np.random.default_rng(B)
        pl = BatchedMSPlanner(B, 16)
        pl.map_create(NX, NY, LO, LO, RES, detection_range=RANGE, perspective=0)
        pl.mission_create()
        pts = rng.uniform(-35.0, 35.0, (B, 1 + 2 * TASKS, 2))
        pl.mission_set(np.full(B, TASKS, np.int32), pts)
        pl.mission_set_goals(pts[:, 1])
        view = pl.device_mission()
        grid_buf = np.zeros((NX, NY), np.uint8)
        gp = grid_buf.ctypes.data_as(C.POINTER(C.c_ubyte))
        for label, near in (("none", 0), ("a quarter", B // 4), ("all", B)):
            poses = pts[:, 1] + 100.0
            poses[:near] = pts[:near, 1] + (1.0, 0.0)
            d_poses = torch.from_numpy(np.ascontiguousarray(poses)).cuda()
            step = lambda: pl.mission_step(d_poses, stride=16, stream=s, count=B)
            paint = lambda: pl.map_paint_device(view.edits, view.n_edits, capacity=2 * B, stream=s)
            both = lambda: pl.mission_step(d_poses, stride=16, stream=s, count=B, esdf_odom=(0.0, 0.0), esdf_range=RANGE)
            step(); both(); s.synchronize()
            edits = pl.mission_state()["edits"]
            assert len(edits) == near

            def host_route():
                pl._check(pl.L.alore_backend_map_get(pl.h, gp, None, None))
                numpy_edits(grid_buf, edits)
                pl.map_set_grid(grid_buf)

            t = {k: [] for k in ("step", "step host", "paint", "both", "route")}
            for _ in range(runs):
                t["step"].append(device_us(step))
                t["route"].append(host_us(host_route))
                t["step host"].append(host_us(step))
                t["paint"].append(device_us(paint))
                t["both"].append(device_us(both))
            print(f"B = {B:4d}, {label} within reach ({near} edits)")
            print(f"  step, device            {spread(t['step'])}")
            print(f"  step, host returns      {spread(t['step host'])}")
            print(f"  paint alone, device     {spread(t['paint'])}")
            print(f"  step + ESDF 27 m        {spread(t['both'])}")
            print(f"  host route, wall        {spread(t['route'])}")
        pl.close()


if __name__ == "__main__":
    main()
