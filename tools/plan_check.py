#!/usr/bin/env python3
"""Time of alore_backend_check_plans on 8192 stored plans (one GPU's share of BASELINE configs[4]: bench.py's Monte-Carlo goals, seed
44) after a map change, by HIP events around REPS back-to-back launches without a host copy (out = NULL), next to last_plan_ms of
the same handle: full window and t_from at half of each plan's duration, reference point alone and with the body points; then
one synchronous call (records copied to the host, wall clock).  Also prints the registers / scratch / LDS of the kernels of
backend_kernels.hip as the compiler reports them with the flags of the csrc Makefile.
usage: plan_check.py [B plans] [REPS]      (output kept in profiles/plan_check.txt)"""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

from alore_legged_manipulator_amd.backend import DP, BatchedMSPlanner
from alore_legged_manipulator_amd.flat_traj import monte_carlo_goals


def resources():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc")
    flags = None
    for line in open(os.path.join(csrc, "Makefile")):
        if line.startswith("FLAGS"):
            flags = [f.replace("$(ARCH)", "gfx950") for f in line.split(":=", 1)[1].split()]
    if not os.path.exists(hipcc) or not flags:
        print("resources: no hipcc here")
        return
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "backend_kernels.hip"),
                        "-o", os.devnull], capture_output=True, text=True)
    cur = {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
        else:
            cur[m.group(1)] = m.group(2)
        if m.group(1).startswith("LDS"):
            print("resources: " + ", ".join(f"{k} {v}" for k, v in cur.items()))


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    fts = monte_carlo_goals(B, seed=44)
    pl = BatchedMSPlanner(B, 16)
    pl.set_free_map(half=20.0)
    res = pl.minco_plan(fts)
    plan_ms = pl.last_plan_ms()
    total = np.array([res["T"][b, :res["n_pieces"][b]].sum() for b in range(B)])
    panels = 16 * int(res["n_pieces"].sum())
    print(f"{B} plans, {panels} panels ({panels / B:.0f} per plan), ok {int(res['ok'].sum())}; last_plan_ms {plan_ms:.2f}")
    # the map changes: discs of 0.5 m on a 4 m lattice (the start poses lie in [-5, 5]^2, the goals 3 to 8 m away)
    n, cell, half = 400, 0.1, 20.0
    c = (np.arange(n) + 0.5) * cell - half
    X, Y = np.meshgrid(c, c, indexing="ij")
    field = np.hypot((X + 2.0) % 4.0 - 2.0, (Y + 2.0) % 4.0 - 2.0) - 0.5
    pl.set_map(field, -half, -half, cell)
    half_t = np.ascontiguousarray(0.5 * total)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, tf, body in (("full window", None, 0), ("t_from = half the duration", half_t, 0), ("full window, body points", None, 1),
                           ("t_from = half the duration, body points", half_t, 1)):
        tfp = None if tf is None else tf.ctypes.data_as(DP)
        for _ in range(3):
            assert pl.L.alore_backend_check_plans(pl.h, B, tfp, None, 0.0, body, None, None) == 0
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(reps):
            assert pl.L.alore_backend_check_plans(pl.h, B, tfp, None, 0.0, body, None, None) == 0
        ev1.record()
        torch.cuda.synchronize()
        ms = ev0.elapsed_time(ev1) / reps
        t0 = time.perf_counter()
        got = pl.check_plans(t_from=tf, body=bool(body))
        wall = (time.perf_counter() - t0) * 1e3
        print(f"{name}: {ms * 1e3:.1f} us per check of {B} plans (HIP events, upload of the windows included, {reps} launches; "
              f"last_plan_ms {plan_ms:.2f} ms = {plan_ms / ms:.0f} x); with the records on the host {wall:.2f} ms wall; "
              f"flagged {int(got['collision'].sum())}, panels looked at {int(got['n_checked'].sum())}")
    resources()


if __name__ == "__main__":
    main()
