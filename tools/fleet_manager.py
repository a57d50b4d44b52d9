#!/usr/bin/env python3
"""Times the fleet's plan_manager state machine on one GPU: 64, 512 and 4096 robots that all have a far goal and a manager whose
replan_time is shorter than a period, so that every robot plans in every period (the most work the kernels can have).  The outcome
of the plans is scripted through the pointer arguments of manager_end.  Prints what profiles/fleet_manager.txt records.

  device       manager_begin + manager_starts + manager_end of one period, device time (HIP events on a stream)
  host returns the time until the host is back from those three calls
  host route   the same decisions driven by the host: alore_backend_get_manager (state, waits) -> the Python oracle of the tests
               (tests/fleet_manager_cases.py: begin and end for every robot) -> upload of the five masks, wall time, in the same
               process, alternating with the device route, after a warm-up

The whole replan.manager_cycle (search, problems, optimiser, deliveries) is not timed here: its device time is that of the steps
tools/traj_handoff.py and tools/path_search.py time.

usage: tools/fleet_manager.py [runs]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARAMS = dict(replan_time=0.125, max_replan_time=0.5)
T0, DT, P = 100.0, 0.25, 16


def spread(v):
    v = np.asarray(v, np.float64)
    return f"median {np.median(v):9.4g}  min {v.min():9.4g}  max {v.max():9.4g}"


def main():
    import torch
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    from tests import fleet_manager_cases as cases
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    s = torch.cuda.Stream()
    print(f"every robot plans in every period, {runs} periods each after 3 of warm-up, times in microseconds")
    for B in (64, 512, 4096):
        rng = np.random.default_rng(B)
        pl = BatchedMSPlanner(B, P)
        pl.manager_create(**PARAMS)
        start = rng.uniform(-3.0, 3.0, (B, 3))
        goal = start + (40.0, 30.0, 0.5)
        pl.manager_request(start, goal)
        oracle = cases.Fleet(B, dict(cases.DEFAULT_PARAMS, **PARAMS))
        oracle.request(start, goal)
        f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
        poses = torch.as_tensor(start).cuda()
        xyt, vaj, oaj = (torch.as_tensor(rng.uniform(-1.0, 1.0, (B, 3))).cuda() for _ in range(3))
        sy, ey = torch.zeros(B, **f64), torch.zeros(B, **f64)
        zeros, ones, two = torch.zeros(B, **i32), torch.ones(B, **i32), torch.full((B,), 2, **i32)
        T = torch.zeros(B, P, **f64)
        T[:, :2] = 50.0
        h_T, h = T.cpu().numpy(), [a.cpu().numpy() for a in (xyt, vaj, oaj)]      # the oracle's copies of the predicted-state arrays
        tick = [0]

        def period():
            now = T0 + DT * tick[0]
            pl.manager_begin(now, poses, stride=24, count=B, stream=s)
            pl.manager_starts(B, xyt, vaj, oaj, sy, ey, stream=s)
            pl.manager_end(B, zeros, zeros, ones, T, two, stream=s)

        def host_route():
            now = T0 + DT * tick[0]
            state = pl.get_manager(B)                                    # what a host-side manager has to read every period
            oracle.begin(now, start)
            h[:] = oracle.starts(*h)[:3]
            oracle.end(np.zeros(B, int), np.zeros(B, int), np.ones(B, int), h_T, np.full(B, 2))
            ints = oracle.snapshot()[0]
            masks = [torch.as_tensor(ints[r]).cuda() for r in range(6, 11)]
            torch.cuda.synchronize()
            return state, masks

        t = {k: [] for k in ("device", "host", "route")}
        for k in range(runs + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.synchronize()
            h0 = time.perf_counter()
            e0.record(s); period(); e1.record(s)
            h1 = time.perf_counter()
            e1.synchronize()
            r0 = time.perf_counter()
            host_route()
            r1 = time.perf_counter()
            tick[0] += 1
            if k >= 3:
                t["device"].append(e0.elapsed_time(e1) * 1e3)
                t["host"].append((h1 - h0) * 1e6)
                t["route"].append((r1 - r0) * 1e6)
        got, want = pl.get_manager(B), oracle.snapshot()
        assert np.array_equal(got["ints"], want[0]) and got["doubles"].tobytes() == want[1].tobytes(), "the two routes must agree"
        c = got["counters"]
        print(f"B = {B:4d}: {c['fresh']} fresh and {c['replan']} replan plans, {c['delivered']} delivered")
        print(f"  begin + starts + end, device   {spread(t['device'])}")
        print(f"  begin + starts + end, host     {spread(t['host'])}")
        print(f"  host route, wall               {spread(t['route'])}")
        pl.close()


if __name__ == "__main__":
    main()
