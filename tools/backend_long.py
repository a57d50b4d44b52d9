#!/usr/bin/env python3
"""Routes of 20 to 60 m through the whole back_end on one GPU: the disc scene of tools/path_search.py wide (an 800 x 800 map at
0.1 m), searched on the wide route, built and planned on a 64-piece handle.  Prints what profiles/backend_long.txt records.

  chain        search_paths_device -> set_paths_device -> plan -> check_plans for 256 and 2048 routes: how many slots build, how many
               need more than 64 pieces or more than 31 way-points, how many plans the optimiser and check_plans accept; time per
               launch of the optimiser (the handle's HIP events) and evaluations per plan
  host         the oracle's minco_plan (oracle/backend_oracle.c) on the first problems of the same launch, one core of this machine
  neutrality   the 8192-plan launch of bench.py --full's back_end row (16-piece build) and a 32-piece launch, alternating in one
               process between this library and one built from the parent commit, the order inside a round reversed every round,
               with a second handle of this library as the control: times and whether the result slabs are bit-equal

usage: tools/backend_long.py [runs] [host problems] [library of the parent commit]

Registers, scratch and LDS of the three builds come from the compiler's own report (make -C alore_legged_manipulator_amd/csrc
backend-resource-usage) and are written into the profile by hand."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from path_search import LO, NX, NY, RES, WIDE_MARGIN, disc_map, histogram, spread, wide_problems  # noqa: E402

RESULT_KEYS = ("ok", "attempts", "alm_rounds", "evals", "lbfgs_ret", "path_ret", "collision", "n_pieces", "cost", "min_dist", "tail_s",
               "xy_err", "inner", "T", "coef")


def planner_of(lib_path, B, P):
    """a planner on another build of the library in this process (the parent commit's)"""
    import ctypes as C
    from alore_legged_manipulator_amd import _lib, backend
    ours = _lib.load()
    other = C.CDLL(lib_path)
    for name, res, args in _lib.SYMBOLS:
        fn = getattr(other, name)
        fn.restype, fn.argtypes = res, args
    if not hasattr(other, "alore_backend_launch_order"):
        setattr(other, "alore_backend_launch_order", getattr(ours, "alore_backend_launch_order"))   # never called on that planner
    _lib._lib = other
    try:
        return backend.BatchedMSPlanner(B, P)
    finally:
        _lib._lib = ours


def long_goals(n, seed=32):
    """two-point routes of 14 to 26 m from starts within +-5 m: 17 to 32 pieces at the default front end"""
    from alore_legged_manipulator_amd.flat_traj import waypoint_path
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        p0, b, d = rng.uniform(-5, 5, 2), rng.uniform(-np.pi, np.pi), rng.uniform(14.0, 26.0)
        ft = waypoint_path([p0, p0 + d * np.array([np.cos(b), np.sin(b)])], b + rng.uniform(-0.5, 0.5), b + rng.uniform(-0.5, 0.5))
        if 16 < ft.pieces <= 32:
            out.append(ft)
    return out


def chain(dist, runs, n_host):
    import torch
    from alore_legged_manipulator_amd import flat_traj
    from alore_legged_manipulator_amd.backend import (BUILD_E_PIECES, BUILD_OK, SEARCH_E_POINTS, BatchedMSPlanner)
    from oracle.backend_driver import BackendOracle, EsdfGrid
    N, SLOTS, CELLS = 2048, 256, NX * NY
    prob = wide_problems(dist, N)
    pl = BatchedMSPlanner(N, 64)
    pl.set_map(dist, LO, LO, RES)
    pl.search_reserve(CELLS, SLOTS)
    d_start, d_goal = torch.from_numpy(np.ascontiguousarray(prob[:, :2])).cuda(), torch.from_numpy(np.ascontiguousarray(prob[:, 2:])).cuda()
    yaw = torch.zeros(N, dtype=torch.float64, device="cuda")
    prm = flat_traj.FrontEndParams()
    print(f"long routes: map {NX} x {NY} at {RES} m with 14 discs, end points 20 to 60 m apart (median {np.median(np.hypot(prob[:, 2] - prob[:, 0], prob[:, 3] - prob[:, 1])):.1f} m), "
          f"window_margin {WIDE_MARGIN}, start and end yaw 0, from rest; handle of 64 pieces; {runs} runs after one warm-up")
    keep = None
    for n in (256, N):
        pl.search_paths_device(n, d_start, d_goal, window_margin=WIDE_MARGIN)
        v = pl.device_paths()
        pl.set_paths_device(n, v.max_points, v.n_points, v.xy, yaw, yaw, params=prm)
        torch.cuda.synchronize()
        sst, bst = pl.search_status(n), pl.build_status(n)
        built = bst == BUILD_OK
        mask = torch.from_numpy(built.astype(np.int32)).cuda()
        torch.cuda.synchronize()
        ms = []
        for r in range(runs + 1):
            pl.plan(n, mask=mask)
            t = pl.last_plan_ms()
            if r:
                ms.append(t)
        res = pl.results(n)
        chk = pl.check_plans(count=n)
        pieces = pl.problems(n)["n_pieces"][built]
        ok = res["ok"][built] == 1
        print(f"{n} routes: search status {histogram(sst)} ({int((sst == SEARCH_E_POINTS).sum())} need more than 31 way-points); build status {histogram(bst)}: "
              f"{int(built.sum())} build, {int((bst == BUILD_E_PIECES).sum())} need more than 64 pieces")
        print(f"  pieces of the built slots: median {np.median(pieces):.0f}, min {pieces.min()}, max {pieces.max()}; {int((pieces > 32).sum())} have more than 32")
        print(f"  optimiser: {int(ok.sum())} of {int(built.sum())} accepted (attempts {histogram(res['attempts'][built])}); "
              f"check_plans on the same map: {int(chk['collision'][built][ok].sum())} of the accepted collide")
        print(f"  launch of the optimiser [ms, HIP events]: {spread(ms)}; {np.median(ms) / max(int(built.sum()), 1):.4g} ms per plan amortised")
        ev = res["evals"][built]
        print(f"  evaluations per plan: median {np.median(ev):.0f}, mean {ev.mean():.0f}, max {ev.max()}")
        if n == 256:
            keep = (pl.paths(n), built.copy(), res, np.median(ms))
    # ---- the oracle on one host core, the first built problems of the 256-route launch
    paths, built, res, ms256 = keep
    orc = BackendOracle()
    grid = EsdfGrid(dist, LO, LO, RES)
    idx = np.nonzero(built)[0][:n_host]
    fts = [flat_traj.with_time(flat_traj.sample_path(paths["xy"][b, :paths["n_points"][b]], 0.0, 0.0), prm, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)) for b in idx]
    assert all(ft.pieces == res["n_pieces"][b] for ft, b in zip(fts, idx))
    t0 = time.perf_counter()
    refs = [orc.minco_plan(grid, ft) for ft in fts]
    host_ms = (time.perf_counter() - t0) * 1e3
    dev_cost = [abs(res["cost"][b] - r["cost"]) / abs(r["cost"]) for b, r in zip(idx, refs)]
    print(f"host, one core, the oracle's minco_plan on the first {len(idx)} built problems of the 256-route launch: {host_ms:.4g} ms, "
          f"{host_ms / len(idx):.4g} ms per plan ({sum(bool(r['ok']) for r in refs)} accepted, {int(res['ok'][idx].sum())} of the same on the device; "
          f"evaluations mean {np.mean([r['evals'] for r in refs]):.0f} against {res['evals'][idx].mean():.0f}; cost apart by median {np.median(dev_cost):.2e}, max {max(dev_cost):.2e})")
    print(f"  the device's launch of 256 routes takes {ms256:.4g} ms: {ms256 / max(int(built.sum()), 1):.4g} ms per plan amortised")
    pl.close()


def neutrality(runs, parent):
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    from alore_legged_manipulator_amd.flat_traj import monte_carlo_goals
    for label, P, fts, half in (("8192 plans, 16-piece build (bench.py --full, back_end row)", 16, monte_carlo_goals(8192, seed=44), 20.0),
                                ("1024 plans of 17 to 32 pieces, 32-piece build", 32, long_goals(1024), 40.0)):
        B = len(fts)
        # a second handle of this library is the control: what two handles of ONE library differ by (their slabs lie elsewhere)
        handles = {"this": BatchedMSPlanner(B, P)}
        if parent:
            handles["parent"] = planner_of(parent, B, P)
        handles["this, 2"] = BatchedMSPlanner(B, P)
        for h in handles.values():
            h.set_free_map(half=half)
            h.set_problems(fts)
        ms = {k: [] for k in handles}
        for r in range(2 * runs + 1):
            turn = list(handles.items())
            for k, h in (turn if r % 2 else turn[::-1]):                # the order within a round alternates
                h.plan()
                t = h.last_plan_ms()
                if r:
                    ms[k].append(t)
        res = {k: h.results() for k, h in handles.items()}
        pieces = res["this"]["n_pieces"]
        print(f"{label}; pieces mean {pieces.mean():.1f}, max {pieces.max()}; {int(res['this']['ok'].sum())} accepted; handles alternating in one process:")
        for k, v in ms.items():
            print(f"  {k:<8} [ms]: {spread(v)}")
        for k in handles:
            same = all(np.ascontiguousarray(res[k][q]).tobytes() == np.ascontiguousarray(res["this"][q]).tobytes() for q in RESULT_KEYS)
            print(f"  {k:<8} result slabs bit-equal to this library's: {same}")
        for h in handles.values():
            h.close()


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n_host = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    parent = sys.argv[3] if len(sys.argv) > 3 else None
    chain(disc_map(), runs, n_host)
    neutrality(runs, parent)


if __name__ == "__main__":
    main()
