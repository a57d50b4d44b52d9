#!/usr/bin/env python3
"""LTV-MPC ticks that relinearise until du <= du_th (alore_ltv_tick_converge) against the fixed n_relin = 5 of alore_ltv_tick:
B = 4096 robots, T = 30, delay_num 1, on the arc references of tests/test_ltv_mpc.py (half of the robots start on their arc,
half 0.3 m / 0.5 rad off it), one cold tick (reset) and 20 warm ticks with the unicycle plant in the loop; microseconds per tick
(the C call alone: upload, kernel, download, wait) and the mean / max of the passes the robots took.
usage: ltv_converged.py [--fixed-only]     (--fixed-only: just the fixed-count ticks, for a build without the converged calls)"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

from alore_legged_manipulator_amd.ltv_mpc import BatchedLtvMpc, default_config

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
B, T, DT, WARM, REPS, MAX_RELIN = 4096, 30, 0.01, 20, 4, 150


def arc_refs(v, w, t0):
    """(B, T, 3), (B, T, 2): the arcs of tests/test_ltv_mpc.py::arc_refs, sampled from time t0 on"""
    ts = t0 + (np.arange(T) + 1) * DT
    a = w[:, None] * ts[None, :]
    xref = np.stack([v[:, None] / w[:, None] * np.sin(a), v[:, None] / w[:, None] * (1 - np.cos(a)), a], axis=2)
    dref = np.stack([np.repeat(v[:, None], T, 1), np.repeat(w[:, None], T, 1)], axis=2)
    return np.ascontiguousarray(xref), np.ascontiguousarray(dref)


def run(eng, du_th):
    """one cold and WARM warm ticks; du_th None: the fixed five passes.  -> (us cold, us per warm tick, |relin_iters| of the cold tick,
    of all warm ticks, robot-ticks that never met the threshold, robot-ticks with a non-zero status)"""
    rng = np.random.default_rng(1)
    v, w = rng.uniform(0.3, 3.2, B), rng.uniform(0.3, 2.5, B) * rng.choice([-1.0, 1.0], B)
    state = np.zeros((B, 3))
    off = np.arange(B) % 2 == 1
    ang = rng.uniform(0, 2 * np.pi, B)
    state[off] = np.stack([0.3 * np.cos(ang), 0.3 * np.sin(ang), 0.5 * rng.choice([-1.0, 1.0], B)], axis=1)[off]
    cmd = np.zeros((B, 2)); st = np.zeros(B, np.int32); it = np.zeros(B, np.int32)
    us, iters, capped = [], [], 0
    for tick in range(WARM + 1):
        eng.set_refs(*arc_refs(v, w, tick * DT))
        t0 = time.perf_counter()
        if du_th is None:
            rc = eng.L.alore_ltv_tick(eng.h, B, state.ctypes.data_as(DP), 5, 1 if tick == 0 else 0, cmd.ctypes.data_as(DP), st.ctypes.data_as(IP), None)
        else:
            rc = eng.L.alore_ltv_tick_converge(eng.h, B, state.ctypes.data_as(DP), MAX_RELIN, du_th, 1 if tick == 0 else 0, cmd.ctypes.data_as(DP),
                                               st.ctypes.data_as(IP), it.ctypes.data_as(IP), None)
        us.append((time.perf_counter() - t0) * 1e6)
        eng._check(rc)
        capped += int((st != 0).sum())
        iters.append(it.copy())
        state += np.stack([cmd[:, 0] * np.cos(state[:, 2]) * DT, cmd[:, 0] * np.sin(state[:, 2]) * DT, cmd[:, 1] * DT], axis=1)
    iters = np.array(iters)
    return us[0], float(np.mean(us[1:])), np.abs(iters[0]), np.abs(iters[1:]), int((iters < 0).sum()), capped


def main():
    fixed_only = "--fixed-only" in sys.argv[1:]
    eng = BatchedLtvMpc(B, default_config(predict_steps=T, delay_num=1))
    base = None
    for du_th in (None,) if fixed_only else (None, 0.1, 0.01, 1e-3):
        runs = [run(eng, du_th) for _ in range(REPS)][1:]       # the first repetition warms the runtime up
        cold, warm = min(r[0] for r in runs), min(r[1] for r in runs)
        if du_th is None:
            base = (cold, warm)
            print(f"B={B} T={T} fixed n_relin 5 : cold {cold:8.1f} us  warm {warm:8.1f} us per tick  status != 0 {runs[-1][5]}", flush=True)
        else:
            _, _, kc, kw, never, capped = runs[-1]
            print(f"B={B} T={T} du_th {du_th:7.0e}   : cold {cold:8.1f} us ({cold / base[0]:.2f} x fixed)  warm {warm:8.1f} us per tick ({warm / base[1]:.2f} x fixed)  "
                  f"passes cold mean {kc.mean():.2f} max {kc.max()}  warm mean {kw.mean():.2f} max {kw.max()}  never met {never}  status != 0 {capped}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
