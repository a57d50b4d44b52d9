#!/usr/bin/env python3
"""Measures the ICR EKF on one GPU and prints what profiles/icr_ekf.txt records.

  resources  registers, scratch and LDS of the kernels of csrc/icr_ekf.hip (hipcc -save-temps with the Makefile's flags for that
             file, tools/kernel_resources.py; LDS from -Rpass-analysis=kernel-resource-usage).  Needs no GPU.
  step       alore_nmpc_ekf_step for B = 64 / 512 / 4096 robots, a pose update on every call and on none: LAUNCHES calls back to
             back between two HIP events on a stream, per call
  error      the largest |device - oracle| / max(1, |oracle|) over the oracle's groups (tests/test_icr_ekf_gpu.py measures it)
  tick       alore_nmpc_ekf_closed_loop_run against alore_nmpc_closed_loop_run with ALORE_NMPC_CLOSED_LOOP_SERIAL=1 (sampler,
             solve, plant: three kernels in a row) on the same fleet of arcs, TICKS ticks between two events, per tick
  host       the same header through tools/micro/icr_ekf_host.cpp (g++ -O2, one core of the same box), per robot and step

usage: tools/icr_ekf.py [resources] [gpu]      (both when neither is given)"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc")
COUNTS = (64, 512, 4096)
LAUNCHES, TICKS, RUNS = 200, 100, 7


def spread(v):
    v = np.asarray(v, np.float64)
    return f"median {np.median(v):.4g}  min {v.min():.4g}  max {v.max():.4g}  (n = {len(v)})"


def resources():
    tmp = tempfile.mkdtemp()
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-fPIC"]       # csrc/Makefile: build/icr_ekf.o
    r = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-save-temps=obj", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, "icr_ekf.hip"), "-o", os.path.join(tmp, "icr_ekf.o")], capture_output=True, text=True, check=True)
    print("kernel resources (hipcc " + " ".join(flags) + " -save-temps, tools/kernel_resources.py; one thread per robot, 64 per workgroup)")
    asm = os.path.join(tmp, "icr_ekf-hip-amdgcn-amd-amdhsa-gfx950.s")
    print(subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), asm, "icrekf"], text=True), end="")
    names, lds, occ, sspill = [], [], [], []
    for line in r.stderr.split("\n"):
        for key, out in (("Function Name:", names), ("LDS Size [bytes/block]:", lds), ("Occupancy [waves/SIMD]:", occ), ("SGPRs Spill:", sspill)):
            if key in line:
                out.append(line.split(key)[1].split("[")[0].strip())
    for n, l, o, s in zip(names, lds, occ, sspill):
        print(f"  {n}: LDS {l} B, {o} wave(s) per SIMD, {s} SGPRs spilled")


def gpu():
    os.environ["ALORE_NMPC_CLOSED_LOOP_SERIAL"] = "1"
    import torch
    from alore_legged_manipulator_amd.host import Polynome
    from alore_legged_manipulator_amd.nmpc import BatchedNmpc
    from tests import test_icr_ekf_gpu as tg
    s = torch.cuda.Stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); fn(); e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)  # ms

    def series(fn, prepare=lambda: None):
        out = []
        for k in range(RUNS + 1):   # the first is the warm-up
            prepare()
            torch.cuda.synchronize()
            out.append(timed(fn))
        return out[1:]

    print(f"\nekf_step, {LAUNCHES} calls back to back between two HIP events, {RUNS} runs after one warm-up; us per call")
    rng = np.random.default_rng(3)
    with torch.cuda.stream(s):
        for B in COUNTS:
            eng = tg.engine(B, tg.cases.DEFAULT)
            pose = np.stack([rng.uniform(-5, 5, B), rng.uniform(-5, 5, B), rng.uniform(-3, 3, B)], 1)
            wheel = torch.from_numpy(rng.uniform(0.5, 1.5, (B, 2))).cuda()
            meas = torch.from_numpy(pose + rng.normal(0, 0.01, (B, 3))).cuda()
            for label, z in (("a pose update in every call", meas), ("no pose update", None)):
                t = series(lambda: [eng.ekf_step(wheel, 0.01, z) for _ in range(LAUNCHES)], lambda: eng.ekf_reset(pose=pose))
                assert (eng.ekf_get()["status"] == 0).all()
                print(f"  B = {B:5d}, {label:28s}: {spread(np.array(t) * 1e3 / LAUNCHES)}")
            eng.close()
    worst = tg.run_groups(tg.MAIN, 70)
    print(f"\nforecast: largest |device - oracle| / max(1, |oracle|) over the oracle's groups, B = 70: {worst:.3e}")

    print(f"\nclosed loop, N = 20, {TICKS} ticks between two HIP events, {RUNS} runs after one warm-up; us per tick")
    with torch.cuda.stream(s):
        for B in COUNTS:
            msgs = []
            for b in range(B):
                v, w = rng.uniform(0.4, 1.2), rng.uniform(-0.8, 0.8)
                Tp = np.array([0.5, 0.5, 0.5]); Tc = np.cumsum(Tp)
                msgs.append(Polynome(np.stack([w * Tc[:-1], v * Tc[:-1]], 1), Tp, [0, 0, w, v, 0, 0], [w * Tc[-1], v * Tc[-1], w, v, 0, 0],
                                     [0, 0, 0], [-0.3, 0.3, 0.1], 0.0))
            pose0 = np.stack([rng.uniform(-0.05, 0.05, B), rng.uniform(-0.05, 0.05, B), rng.uniform(-0.1, 0.1, B)], 1)
            icr = np.tile([0.1, -0.3, 0.3], (B, 1))
            eng = BatchedNmpc(B, 20, 0.01)
            eng.load({"W": np.tile(np.diag([10, 10, 0.5, 0.1, 0.1]).astype(np.float32), (B, 20, 1, 1)),
                      "WN": np.tile(np.diag([10, 10, 0.5]).astype(np.float32), (B, 1, 1))})
            eng.refs_init(max_pieces=4, max_checkpoints=32)
            eng.refs_set_polynomes(np.arange(B), msgs)
            eng.plant_init()
            eng.ekf_init()

            def prepare():
                eng.plant_set_state(pose0, icr)
                eng.closed_loop_reset()
                eng.ekf_reset()
            t_ekf = series(lambda: eng.ekf_closed_loop_run(0.01, 0.01, TICKS), prepare)
            assert (eng.ekf_get()["status"] == 0).all()
            t_plain = series(lambda: eng.closed_loop_run(0.01, 0.01, TICKS), prepare)
            print(f"  B = {B:5d}, EKF tick (sampler from the estimate, solve, plant + filter): {spread(np.array(t_ekf) * 1e3 / TICKS)}")
            print(f"  B = {B:5d}, plain tick (sampler, solve, plant: three kernels in a row):   {spread(np.array(t_plain) * 1e3 / TICKS)}")
            eng.close()

    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "icr_ekf_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tools", "micro", "icr_ekf_host.cpp"), "-o", exe])
    print("\nhost: csrc/icr_ekf.h, g++ -O2, one core; ns per robot and step (B = 4096, 200 steps)")
    for every in (1, 10):
        ns = [float(subprocess.check_output([exe, "4096", "200", str(every)], text=True).split()[0]) for _ in range(3)]
        print(f"  a pose update on every {every:2d}th step: {spread(ns)}")


if __name__ == "__main__":
    want = sys.argv[1:] or ["resources", "gpu"]
    if "resources" in want:
        resources()
    if "gpu" in want:
        gpu()
