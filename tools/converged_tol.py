#!/usr/bin/env python3
"""Converged solves to a KKT tolerance (alore_nmpc_rti_many_converge) against the fixed 15 iterations of rti_range: B = 4096 problems
of bench.py's distribution per batch, 20 batches in one grid; microseconds per batch and the mean / max of the iterations the problems
took, at N = 20 (packed mapping) and N = 50 (automatic mapping).  usage: converged_tol.py [K batches]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from alore_legged_manipulator_amd.nmpc import BatchedNmpc
from alore_legged_manipulator_amd.scenarios import make_batch


def main():
    B, K, MAXS = 4096, int(sys.argv[1]) if len(sys.argv) > 1 else 20, 15
    dev = torch.device("cuda:0")
    for N in (20, 50):
        eng = BatchedNmpc(B, N, device=0, slots=K)
        eng.load(make_batch(B, N), slot=None)
        keep = {k: eng.ts[k].clone() for k in ("x", "u", "dual")}

        def restore():
            for k, v in keep.items():
                eng.ts[k].copy_(v)
        base = None
        for tol in (None, 1e-3, 1e-4, 1e-6):
            ts = []
            for rep in range(5):
                restore()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                if tol is None:
                    eng.rti_range(0, K, MAXS)
                else:
                    eng.rti_range_converge(0, K, MAXS, tol)
                torch.cuda.synchronize(dev)
                ts.append((time.perf_counter() - t0) / K * 1e6)
            us = min(ts[1:])
            info = eng.launch_info()
            if tol is None:
                base = us
                print(f"N={N} K={K} fixed {MAXS:2d}      : {us:8.2f} us per batch of {B}  lanes {info['lanes_per_problem']:#x}", flush=True)
            else:
                it = eng.sqp_iters.cpu().numpy()
                k = abs(it)  # -15: never met
                never = int((it < 0).sum())
                print(f"N={N} K={K} tol {tol:7.0e} : {us:8.2f} us per batch ({us / base:.2f} x fixed)  iterations mean {k.mean():.2f} "
                      f"max {k.max()}  never met {never}  lanes {info['lanes_per_problem']:#x}", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
