#!/usr/bin/env python3
"""Measurements of the back_end's object classes (alore_backend_set_classes) on the GPU; profiles/backend_classes.txt keeps the output.

  plan-worker --root TREE --sizes 8192,2048 --reps 3
      one process: imports the package from TREE (this tree, or a build of the parent commit), plans the configs[4] problems
      (monte_carlo_goals(n, seed=44), free map, no class table) and prints the duration of every timed launch
      (alore_backend_last_plan_ms: device events round the launch) after one warm-up launch per size
  class-free --parent TREE [--runs 5]
      plan-worker on TREE and on this tree in alternating processes, `runs` each: median and range per build and size
  classes [--n 8192] [--runs 5]
      this build: the n plans without a table, with a one-class table and with the four interleaved classes of configs[4] in ONE launch,
      against four launches of n / 4 on four single-class handles (device time: the sum of the four launches; host time: a clock round
      the four launches and one synchronise), alternating, `runs` each
  stats [--n 8192] [--runs 20]
      alore_backend_class_stats (kernel, 4 records copied down) against copying the status slab and the piece times and reducing them
      in NumPy, host clock round each, after a warm-up; the two results are compared
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES_XV = (0.0, 0.2, 0.1, 0.3)   # tests/test_config4_pipeline.py: CLASSES


def spread(v):
    return f"median {statistics.median(v):.3f} ms, range {min(v):.3f} .. {max(v):.3f} ms over {len(v)}"


def plan_worker(a):
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np  # noqa: F401
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    from alore_legged_manipulator_amd.flat_traj import monte_carlo_goals
    out = {"root": a.root, "ms": {}}
    for n in [int(s) for s in a.sizes.split(",")]:
        fts = monte_carlo_goals(n, seed=44)
        pl = BatchedMSPlanner(n, 16)
        pl.set_free_map(half=20.0)
        pl.set_problems(fts)
        pl.plan()
        pl.last_plan_ms()
        ms = []
        for _ in range(a.reps):
            pl.plan()
            ms.append(pl.last_plan_ms())
        assert int(pl.results()["ok"].sum()) == n
        out["ms"][str(n)] = ms
        pl.close()
    print("WORKER " + json.dumps(out))


def class_free(a):
    trees = {"parent": a.parent, "this build": ROOT}
    got = {k: {} for k in trees}
    for r in range(a.runs):
        for name, tree in trees.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "plan-worker", "--root", tree, "--sizes", a.sizes, "--reps", str(a.reps)],
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-2000:])
                sys.exit(f"worker on {name} failed ({p.returncode})")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("WORKER ")][-1]
            for n, ms in json.loads(line[7:])["ms"].items():
                got[name].setdefault(n, []).append(statistics.median(ms))
    for n in a.sizes.split(","):
        print(f"class-free launch, {n} plans, one figure per process (the median of {a.reps} launches after a warm-up), processes alternating:")
        for name in trees:
            print(f"  {name:10s} {spread(got[name][n])}   [{', '.join('%.3f' % v for v in got[name][n])}]")
        lo, hi, med = min(got["parent"][n]), max(got["parent"][n]), statistics.median(got["this build"][n])
        print(f"  this build's median {med:.3f} ms lies {'INSIDE' if lo <= med <= hi else 'OUTSIDE'} the parent's run-to-run range {lo:.3f} .. {hi:.3f} ms")


def class_configs():
    from alore_legged_manipulator_amd.backend import default_config
    out = []
    for xv in CLASSES_XV:
        c = default_config()
        c.standard_diff, c.icr_xv = 0, xv
        out.append(c)
    return out


def classes(a):
    import numpy as np
    import torch
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner, default_config
    from alore_legged_manipulator_amd.flat_traj import monte_carlo_goals
    n, q = a.n, a.n // 4
    fts = monte_carlo_goals(n, seed=44)
    cfgs = class_configs()

    def handle(count, problems, cfg=None, table=None, class_of=None):
        pl = BatchedMSPlanner(count, 16, cfg)
        pl.set_free_map(half=20.0)
        if table is not None:
            pl.set_classes(table)
        if class_of is not None:
            pl.set_problem_classes(class_of)
        pl.set_problems(problems)
        pl.plan()
        pl.last_plan_ms()
        return pl
    plain = handle(n, fts)
    one = handle(n, fts, table=[default_config()])
    mixed = handle(n, fts, table=cfgs, class_of=np.arange(n, dtype=np.int32) % 4)
    singles = [handle(q, fts[k::4], cfg=cfgs[k]) for k in range(4)]
    ms = {"no table, one launch": [], "one-class table, one launch": [], "four interleaved classes, one launch": [],
          "four single-class handles, four launches (sum of the launches)": [], "four interleaved classes, one launch (host clock)": [],
          "four single-class handles, four launches (host clock)": []}
    for _ in range(a.runs):
        plain.plan(); ms["no table, one launch"].append(plain.last_plan_ms())
        one.plan(); ms["one-class table, one launch"].append(one.last_plan_ms())
        torch.cuda.synchronize(); t0 = time.perf_counter()
        mixed.plan(); torch.cuda.synchronize()
        ms["four interleaved classes, one launch (host clock)"].append((time.perf_counter() - t0) * 1e3)
        ms["four interleaved classes, one launch"].append(mixed.last_plan_ms())
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for pl in singles:
            pl.plan()
        torch.cuda.synchronize()
        ms["four single-class handles, four launches (host clock)"].append((time.perf_counter() - t0) * 1e3)
        ms["four single-class handles, four launches (sum of the launches)"].append(sum(pl.last_plan_ms() for pl in singles))
    print(f"{n} plans of configs[4] (monte_carlo_goals(seed=44), free map), planning time per route, routes alternating:")
    for k, v in ms.items():
        print(f"  {k:66s} {spread(v)}")
    rm = mixed.results()
    same = all(np.array_equal(rm[f][k::4], singles[k].results()[f]) for k in range(4) for f in ("T", "coef", "evals"))
    print(f"  the mixed launch and the four handles leave the same bits (T, coef, evals): {same}; ok: {int(rm['ok'].sum())} of {n}")
    print("  class_stats of the mixed launch:", mixed.class_stats().tolist())


def stats(a):
    import ctypes as C
    import numpy as np
    import torch
    from alore_legged_manipulator_amd.backend import CLASS_STAT_DTYPE, BatchedMSPlanner, StatusC
    from alore_legged_manipulator_amd.flat_traj import monte_carlo_goals
    n = a.n
    pl = BatchedMSPlanner(n, 16)
    pl.set_free_map(half=20.0)
    pl.set_classes(class_configs())
    class_of = np.arange(n, dtype=np.int32) % 4
    pl.set_problem_classes(class_of)
    pl.set_problems(monte_carlo_goals(n, seed=44))
    pl.plan()
    dt = np.dtype([(k, np.int32) for k in ("ok", "attempts", "alm_rounds", "evals", "lbfgs_ret", "path_ret", "collision", "n_pieces")] +
                  [("cost", np.float64), ("xy_err", np.float64, 2), ("min_dist", np.float64), ("tail_s", np.float64)])
    st, T = np.zeros(n, dt), np.zeros((n, pl.P))

    def numpy_route():
        pl._check(pl.L.alore_backend_results(pl.h, n, st.ctypes.data_as(C.POINTER(StatusC)), None, T.ctypes.data_as(C.POINTER(C.c_double)), None, None))
        out = np.zeros(4, CLASS_STAT_DTYPE)
        ok = st["ok"] != 0
        run = np.cumsum(T, axis=1)                        # sequential sums: the duration is run[b, n_pieces - 1]
        dur = run[np.arange(n), np.clip(st["n_pieces"], 1, pl.P) - 1]
        for k in range(4):
            m = class_of == k
            out[k] = (m.sum(), (ok & m).sum(), ((st["collision"] != 0) & m).sum(), st["attempts"][m].sum(), st["evals"][m].astype(np.int64).sum(),
                      st["evals"][m].max(), 0, st["min_dist"][ok & m].min() if (ok & m).any() else np.finfo(np.float64).max,
                      dur[ok & m].max() if (ok & m).any() else 0.0)
        return out

    def kernel_route():
        return pl.class_stats()
    res = {}
    for name, fn in (("class_stats kernel, 4 records copied down", kernel_route), ("status slab and piece times copied down, NumPy", numpy_route)):
        fn(); torch.cuda.synchronize()
        v = []
        for _ in range(a.runs):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            res[name] = fn()
            v.append((time.perf_counter() - t0) * 1e3)
        print(f"  {name:55s} {spread(v)}")
    a_, b_ = list(res.values())
    print(f"  per-class outcome at {n} slots; the two routes agree bit for bit: {a_.tobytes() == b_.tobytes()}")
    print("  ", a_.tolist())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    w = sub.add_parser("plan-worker"); w.add_argument("--root", default=ROOT); w.add_argument("--sizes", default="8192,2048"); w.add_argument("--reps", type=int, default=3)
    c = sub.add_parser("class-free"); c.add_argument("--parent", required=True); c.add_argument("--runs", type=int, default=5)
    c.add_argument("--sizes", default="8192,2048"); c.add_argument("--reps", type=int, default=3)
    k = sub.add_parser("classes"); k.add_argument("--n", type=int, default=8192); k.add_argument("--runs", type=int, default=5)
    s = sub.add_parser("stats"); s.add_argument("--n", type=int, default=8192); s.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    if a.cmd != "plan-worker":
        sys.path.insert(0, ROOT)
    {"plan-worker": plan_worker, "class-free": class_free, "classes": classes, "stats": stats}[a.cmd](a)


if __name__ == "__main__":
    main()
