#!/usr/bin/env python3
"""Measures the LTV-MPC closed loop on the ICR EKF's estimate on one GPU and prints what profiles/ltv_ekf_loop.txt records.

  resources  registers, scratch and spills of the kernels of csrc/ltv_ekf_loop.hip (hipcc with the Makefile's flags for that file,
             -Rpass-analysis=kernel-resource-usage).  Needs no GPU.
  gpu        the fleet of tools/ltv_closed_loop.py (arcs, half of the robots 0.3 m / 0.5 rad off theirs), B = 64 / 512 / 4096,
             T = 30, delay_num 1, three fixed passes, the launch file's plant (follow = 0, five substeps), odom_every = 10.
             Microseconds per tick over TICKS warm ticks (LEAD ticks, the first with reset, come before them); the four routes
             alternate inside every repeat, RUNS repeats after one warm-up:
               (a) alore_ltv_closed_loop_run (true pose, no filter, no noise): the yardstick, by HIP events
               (b) alore_ltv_ekf_closed_loop_run, noise_stddev = 0.01 and measurement noise on, by HIP events
               (c) the pieces of (b) as separate calls (refs_from_store_est, get_cmd_est, plant_ekf_step), by HIP events
               (d) the host-driven route: ekf_get, refs_from_store, tick, a NumPy plant with a NumPy Philox, ekf_step; wall clock
             then the fleet statistic at B = 512 over 300 ticks, noise on and off: RMS distance of the true pose to its arc and of
             the estimate to the true pose.

usage: tools/ltv_ekf_loop.py [resources] [gpu]      (both when neither is given)"""
import math
import os
import subprocess
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc")
COUNTS = (64, 512, 4096)
T, DT, LEAD, TICKS, RUNS, N_RELIN, ODOM = 30, 0.01, 20, 100, 5, 3, 10
NOISE, MEAS, SEED = 0.01, (0.004, 0.004, 0.002), 2026
ICR = (0.2, -0.3, 0.3)                            # (xv, yr, yl) of the plant: alore_ltv_plant_init's


def spread(v):
    v = np.asarray(v, np.float64)
    return f"median {np.median(v):8.1f}  min {v.min():8.1f}  max {v.max():8.1f}"


def resources():
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-fPIC"]       # csrc/Makefile: build/ltv_ekf_loop.o
    tmp = tempfile.mkdtemp()
    r = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "ltv_ekf_loop.hip"),
                        "-o", os.path.join(tmp, "ltv_ekf_loop.o")], capture_output=True, text=True, check=True)
    print("kernel resources (hipcc " + " ".join(flags) + " -Rpass-analysis=kernel-resource-usage; one thread per robot, 64 per workgroup)")
    keys = ("Function Name:", "VGPRs:", "AGPRs:", "TotalSGPRs:", "ScratchSize [bytes/lane]:", "VGPRs Spill:", "SGPRs Spill:", "LDS Size [bytes/block]:",
            "Occupancy [waves/SIMD]:")
    for line in r.stderr.split("\n"):
        for k in keys:
            if k in line:
                print(("  " if k == keys[0] else "      ") + k + " " + line.split(k)[1].split("[-R")[0].strip())


# ---- the noise of csrc/sim_noise.h for a whole fleet at once (tests/sim_noise_cases.py states it one draw at a time)
def normal2_np(seed, robots, event, stream):
    M = np.uint64(0xFFFFFFFF)
    c = [np.full(robots.shape, event & 0xFFFFFFFF, np.uint64), np.full(robots.shape, event >> 32, np.uint64), robots.astype(np.uint64),
         np.full(robots.shape, stream, np.uint64)]
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & M, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & M]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF

    def uni(a, b):
        return ((a >> np.uint64(6)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64) + 0.5) * 2.0 ** -52
    r, a = np.sqrt(-2.0 * np.log(uni(c[0], c[1]))), 6.28318530717958647692 * uni(c[2], c[3])
    return r * np.cos(a), r * np.sin(a)


def plant_np(state, cmd, goal, event, noise):
    """tests/sim_noise_cases.plant_step_noisy for the fleet: state (B, 7) = x, y, th, v, w, dv, dw, in place; follow = 0"""
    B = len(state)
    c = np.where(goal[:, None], 0.0, cmd)
    v, w = c[:, 0].copy(), c[:, 1].copy()
    if noise > 0.0:
        z0, z1 = normal2_np(SEED, np.arange(B), event, 0)
        v += (v * noise) * z0
        w += (w * noise) * z1
    for _ in range(5):
        for val, des, lim in ((v, state[:, 5], 0.01 * 2.0), (w, state[:, 6], 0.01 * 4.0)):
            far = np.abs(val - des) >= lim
            val[:] = np.where(far, val + lim * np.sign(des - val), des)
        state[:, 0] += v * 0.002 * np.cos(state[:, 2]); state[:, 1] += v * 0.002 * np.sin(state[:, 2]); state[:, 2] += w * 0.002
    state[:, 3], state[:, 4] = v, w


def fleet(B):
    from alore_legged_manipulator_amd.nmpc import BatchedNmpc
    rng = np.random.default_rng(1)
    v, w = rng.uniform(0.3, 3.2, B), rng.uniform(0.3, 2.5, B) * rng.choice([-1.0, 1.0], B)
    state = np.zeros((B, 3))
    off = np.arange(B) % 2 == 1
    ang = rng.uniform(0, 2 * np.pi, B)
    state[off] = np.stack([0.3 * np.cos(ang), 0.3 * np.sin(ang), 0.5 * rng.choice([-1.0, 1.0], B)], axis=1)[off]
    Tp = np.array([0.5, 0.5, 0.5]); Tc = np.cumsum(Tp)
    msgs = [types.SimpleNamespace(innerpoints=np.stack([w[b] * Tc[:-1], v[b] * Tc[:-1]], 1), t_pts=Tp, init_pva=[0, 0, w[b], v[b], 0, 0],
                                  tail_pva=[w[b] * Tc[-1], v[b] * Tc[-1], w[b], v[b], 0, 0], start_position=[0, 0, 0], ICR=[-0.3, 0.3, 0.0],
                                  traj_start_time=0.0) for b in range(B)]
    store = BatchedNmpc(B, 20, DT)
    store.refs_init(max_pieces=4, max_checkpoints=32)
    store.refs_set_polynomes(np.arange(B), msgs)
    store.ekf_init(odom_every=ODOM)
    return store, state, v, w


def gpu():
    import torch
    from alore_legged_manipulator_amd.ltv_mpc import BatchedLtvMpc, default_config

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / TICKS

    print(f"\nper tick, us: {TICKS} warm ticks after {LEAD}, T = {T}, {N_RELIN} fixed passes, odom_every = {ODOM}; the four routes alternate "
          f"inside each of {RUNS} repeats after one warm-up repeat")
    for B in COUNTS:
        store, state0, _, _ = fleet(B)
        eng = BatchedLtvMpc(B, default_config(predict_steps=T, delay_num=1))
        eng.plant_init()
        hosteng = BatchedLtvMpc(B, default_config(predict_steps=T, delay_num=1))

        def prepare(noise):
            eng.plant_set_state(state0)
            eng.plant_set_noise(noise, MEAS if noise else None, SEED)
            store.ekf_reset(pose=state0)

        def route_a():
            prepare(0.0)
            eng.closed_loop_run(store, DT, DT, LEAD, N_RELIN, None, reset=True)
            return timed(lambda: eng.closed_loop_run(store, DT + LEAD * DT, DT, TICKS, N_RELIN, None))

        def route_b():
            prepare(NOISE)
            eng.ekf_closed_loop_run(store, DT, DT, LEAD, N_RELIN, None, reset=True)
            return timed(lambda: eng.ekf_closed_loop_run(store, DT + LEAD * DT, DT, TICKS, N_RELIN, None))

        def route_c():
            prepare(NOISE)
            eng.ekf_closed_loop_run(store, DT, DT, LEAD, N_RELIN, None, reset=True)

            def pieces():
                for k in range(TICKS):
                    eng.refs_from_store_est(store, (DT + LEAD * DT) + k * DT)    # the run's own `now`: t0 + k * dt_tick
                    eng.get_cmd_est(store, N_RELIN, None)
                    eng.plant_ekf_step(store, DT)
            return timed(pieces)

        def route_d():
            store.ekf_reset(pose=state0)
            st = np.concatenate([state0, np.zeros((B, 4))], 1)
            for k in range(LEAD + TICKS):
                if k == LEAD:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                est = store.ekf_get()["x"][:, :3].copy()
                goal = hosteng.refs_from_store(store, DT + k * DT, est)
                cmd, _ = hosteng.tick(est, n_relin=N_RELIN, reset=(k == 0))
                plant_np(st, cmd, goal, k, NOISE)
                wheel = np.stack([st[:, 3] - st[:, 4] * ICR[2], st[:, 3] - st[:, 4] * ICR[1]], 1)
                meas = None
                if (k + 1) % ODOM == 0:
                    zx, zy = normal2_np(SEED, np.arange(B), k, 1)
                    zt, _ = normal2_np(SEED, np.arange(B), k, 2)
                    meas = torch.from_numpy(st[:, :3] + np.stack([MEAS[0] * zx, MEAS[1] * zy, MEAS[2] * zt], 1)).cuda()
                store.ekf_step(torch.from_numpy(wheel).cuda(), DT, meas=meas)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / TICKS, st

        routes = {"a": [], "b": [], "c": [], "d": []}
        for rep in range(RUNS + 1):
            a = route_a()
            b = route_b()
            pose_b = eng.plant_get_state()[0]
            c = route_c()
            pose_c = eng.plant_get_state()[0]
            d, st_d = route_d()
            assert np.array_equal(pose_b, pose_c), "the run and its pieces differ"
            if rep:
                for k, val in zip("abcd", (a, b, c, d)):
                    routes[k].append(val)
        assert (store.ekf_get()["status"] == 0).all()
        names = {"a": "(a) closed_loop_run (true pose, no filter)     ", "b": "(b) ekf_closed_loop_run, noise on              ",
                 "c": "(c) its pieces as separate calls               ", "d": "(d) host-driven (ekf_get, tick, NumPy, ekf_step)"}
        for k in "abcd":
            print(f"  B = {B:5d}  {names[k]}: {spread(routes[k])}")
        extra = np.array(routes["b"]) - np.array(routes["a"])
        print(f"  B = {B:5d}  (b) - (a), repeat by repeat                    : {spread(extra)}    "
              f"max |pose of (b) - pose of (d)| {np.max(np.abs(pose_b - st_d[:, :3])):.1e}")

        # where (b) - (a) goes: the three pieces of a tick between HIP events, on the loop on the true pose (refs_from_store_device,
        # get_cmd_device, plant_step) and on the loop on the estimate (refs_from_store_est, get_cmd_est, plant_ekf_step)
        def pieces_timed(est):
            prepare(NOISE if est else 0.0)
            if est:
                eng.ekf_closed_loop_run(store, DT, DT, LEAD, N_RELIN, None, reset=True)
            else:
                eng.closed_loop_run(store, DT, DT, LEAD, N_RELIN, None, reset=True)
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(TICKS)]
            torch.cuda.synchronize()
            for k in range(TICKS):
                now = (DT + LEAD * DT) + k * DT
                ev[k][0].record()
                eng.refs_from_store_est(store, now) if est else eng.refs_from_store_device(store, now)
                ev[k][1].record()
                eng.get_cmd_est(store, N_RELIN, None) if est else eng.get_cmd_device(N_RELIN, None)
                ev[k][2].record()
                eng.plant_ekf_step(store, DT) if est else eng.plant_step()
                ev[k][3].record()
            torch.cuda.synchronize()
            return [float(np.mean([ev[k][i].elapsed_time(ev[k][i + 1]) for k in range(TICKS)])) * 1e3 for i in range(3)]

        parts = {False: [], True: []}
        for rep in range(4):
            for est in (False, True):
                t = pieces_timed(est)
                if rep:
                    parts[est].append(t)
        for est, label in ((False, "on the true pose "), (True, "on the estimate  ")):
            m = np.median(np.array(parts[est]), 0)
            print(f"  B = {B:5d}  pieces between events, loop {label}: sampling {m[0]:7.1f}  solve {m[1]:7.1f}  plant{' + filter' if est else '         '} {m[2]:7.1f}")
        eng.close(); hosteng.close(); store.close()

    B, ticks = 512, 300
    from alore_legged_manipulator_amd.scenarios import arc_pose
    store, state0, v, w = fleet(B)
    dur = 1.5
    ref = np.array([[arc_pose(v[b], w[b], 0.0, min(DT * (k + 2), dur)) for b in range(B)] for k in range(ticks)])    # the pose due at the end of tick k
    print(f"\nfleet statistic, B = {B}, {ticks} ticks (the arcs last {dur} s; past their end the reference is their last pose), RMS over robots and ticks")
    for label, run in (("closed_loop_run (true pose, no noise)", "plain"), ("ekf loop, noise off", 0.0), ("ekf loop, noise_stddev 0.01", NOISE)):
        eng = BatchedLtvMpc(B, default_config(predict_steps=T, delay_num=1))
        eng.plant_init(max_trace_ticks=ticks)
        eng.plant_set_state(state0)
        if run == "plain":
            eng.closed_loop_run(store, DT, DT, ticks, N_RELIN, None, reset=True)
        else:
            eng.plant_set_noise(run, MEAS if run else None, SEED)
            store.ekf_reset(pose=state0)
            eng.ekf_closed_loop_run(store, DT, DT, ticks, N_RELIN, None, reset=True)
        pose = eng.plant_trace(ticks)["pose"]
        line = f"  {label:38s}: true pose - arc {math.sqrt(np.mean(np.sum((pose[:, :, :2] - ref[:, :, :2]) ** 2, -1))):.6f} m"
        if run != "plain":
            tr = eng.plant_trace_est(ticks)
            assert (tr["ekf_status"] == 0).all()
            line += f"   estimate - true pose {math.sqrt(np.mean(np.sum((tr['est'][:, :, :2] - pose[:, :, :2]) ** 2, -1))):.6f} m, " \
                    f"{math.sqrt(np.mean((tr['est'][:, :, 2] - pose[:, :, 2]) ** 2)):.6f} rad"
            x = store.ekf_get()["x"]
            line += f"   estimated (yr, yl, xv) mean {np.mean(x[:, 3]):.4f}, {np.mean(x[:, 4]):.4f}, {np.mean(x[:, 5]):.4f} (true {ICR[1]}, {ICR[2]}, {ICR[0]})"
            if run == 0.0:
                quiet = pose
            else:
                line += f"\n  {'':38s}  true pose with noise - true pose without: RMS {math.sqrt(np.mean(np.sum((pose[:, :, :2] - quiet[:, :, :2]) ** 2, -1))):.6f} m, " \
                        f"largest {np.max(np.abs(pose - quiet)):.6f}"
        print(line)
        eng.close()


if __name__ == "__main__":
    want = sys.argv[1:] or ["resources", "gpu"]
    if "resources" in want:
        resources()
    if "gpu" in want:
        gpu()
