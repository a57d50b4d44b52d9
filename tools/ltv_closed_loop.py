#!/usr/bin/env python3
"""LTV-MPC closed loop on the device (alore_ltv_closed_loop_run) against the host-driven tick that was the only route before it.
The fleet of tools/ltv_converged.py -- arcs, half of the robots start on their arc, half 0.3 m / 0.5 rad off it -- as trajectories
in the device store, B = 64, 512 and 4096 robots, T = 30, delay_num 1, the Euler unicycle as the plant (follow = 1, one substep of
dt).  Five fixed passes and du_th = 0.01.  Microseconds per tick over a run of 100 warm ticks (20 ticks, the first with reset, come
before them), the median of seven runs after a warm-up run:
  (a) closed_loop_run, by HIP events around the call;
  (b) the same in a child process with ALORE_LTV_CLOSED_LOOP_SERIAL=1 (the pieces as separate launches);
  (c) refs_from_store + tick (tick_converge) + a NumPy plant driven from the host, wall clock.
usage: ltv_closed_loop.py [--host-only] [--root DIR]
  --host-only  (c) alone: needs nothing this tool's commit added, so it runs on the commit before it as well
  --root DIR   import the package from DIR instead of this tree (a build of another commit)"""
import os
import subprocess
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ARGS = sys.argv[1:]
ROOT = os.path.abspath(ARGS[ARGS.index("--root") + 1]) if "--root" in ARGS else os.path.join(HERE, "..")
sys.path.insert(0, ROOT)

from alore_legged_manipulator_amd.ltv_mpc import BatchedLtvMpc, default_config  # noqa: E402
from alore_legged_manipulator_amd.nmpc import BatchedNmpc  # noqa: E402

T, DT, LEAD, TICKS, RUNS, MAX_RELIN = 30, 0.01, 20, 100, 7, 150
MODES = (("fixed 5 passes", 5, None), ("du_th 0.01", MAX_RELIN, 0.01))


def fleet(B):
    rng = np.random.default_rng(1)
    v, w = rng.uniform(0.3, 3.2, B), rng.uniform(0.3, 2.5, B) * rng.choice([-1.0, 1.0], B)
    state = np.zeros((B, 3))
    off = np.arange(B) % 2 == 1
    ang = rng.uniform(0, 2 * np.pi, B)
    state[off] = np.stack([0.3 * np.cos(ang), 0.3 * np.sin(ang), 0.5 * rng.choice([-1.0, 1.0], B)], axis=1)[off]
    Tp = np.array([0.5, 0.5, 0.5]); Tc = np.cumsum(Tp)
    # Polynome messages (flat space theta, s): three pieces of 0.5 s, constant twist, no ICR offset
    msgs = [types.SimpleNamespace(innerpoints=np.stack([w[b] * Tc[:-1], v[b] * Tc[:-1]], 1), t_pts=Tp, init_pva=[0, 0, w[b], v[b], 0, 0],
                                  tail_pva=[w[b] * Tc[-1], v[b] * Tc[-1], w[b], v[b], 0, 0], start_position=[0, 0, 0], ICR=[-0.3, 0.3, 0.0],
                                  traj_start_time=0.0) for b in range(B)]
    store = BatchedNmpc(B, 20, DT)
    store.refs_init(max_pieces=4, max_checkpoints=32)
    store.refs_set_polynomes(np.arange(B), msgs)
    return store, state


def device_runs(B, store, state, n_relin, du_th):
    import torch
    eng = BatchedLtvMpc(B, default_config(predict_steps=T, delay_num=1))
    eng.plant_init(state_propa_period=DT, substeps=1, follow=1)
    us = []
    for _ in range(RUNS + 1):
        eng.plant_set_state(state)
        eng.closed_loop_run(store, DT, DT, LEAD, n_relin, du_th, reset=True)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.closed_loop_run(store, DT + LEAD * DT, DT, TICKS, n_relin, du_th)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / TICKS)
    pose, vw, goal = eng.plant_get_state()
    st = eng.results()["status"]
    eng.close()
    return float(np.median(us[1:])), int((st != 0).sum()), pose


def host_runs(B, store, state0, n_relin, du_th):
    eng = BatchedLtvMpc(B, default_config(predict_steps=T, delay_num=1))
    us = []
    for _ in range(RUNS + 1):
        state = state0.copy()
        for k in range(LEAD + TICKS):
            if k == LEAD:
                t0 = time.perf_counter()
            eng.refs_from_store(store, DT + k * DT, state)
            if du_th is None:
                cmd, st = eng.tick(state, n_relin=n_relin, reset=(k == 0))
            else:
                cmd, st, _ = eng.tick_converge(state, max_relin=n_relin, du_th=du_th, reset=(k == 0))
            state += np.stack([cmd[:, 0] * np.cos(state[:, 2]) * DT, cmd[:, 0] * np.sin(state[:, 2]) * DT, cmd[:, 1] * DT], axis=1)
        us.append((time.perf_counter() - t0) * 1e6 / TICKS)
    eng.close()
    return float(np.median(us[1:])), int((st != 0).sum()), state


def main():
    host_only = "--host-only" in ARGS
    serial = os.environ.get("ALORE_LTV_CLOSED_LOOP_SERIAL") == "1"
    for B in (64, 512, 4096):
        store, state = fleet(B)
        for name, n_relin, du_th in MODES:
            if host_only:
                us, bad, _ = host_runs(B, store, state, n_relin, du_th)
                print(f"B={B:5d} {name:15s} (c) host-driven tick          {us:8.1f} us per tick   status != 0 {bad}", flush=True)
                continue
            us, bad, pose = device_runs(B, store, state, n_relin, du_th)
            tag = "(b) closed_loop_run, SERIAL=1" if serial else "(a) closed_loop_run          "
            print(f"B={B:5d} {name:15s} {tag} {us:8.1f} us per tick   status != 0 {bad}", flush=True)
            if not serial:
                us, bad, pose_h = host_runs(B, store, state, n_relin, du_th)
                print(f"B={B:5d} {name:15s} (c) host-driven tick          {us:8.1f} us per tick   status != 0 {bad}   "
                      f"max |pose - pose of (a)| {np.max(np.abs(pose - pose_h)):.1e}", flush=True)
    if not host_only and not serial:
        subprocess.check_call([sys.executable, os.path.abspath(__file__)] + ARGS, env=dict(os.environ, ALORE_LTV_CLOSED_LOOP_SERIAL="1"))


if __name__ == "__main__":
    main()
