"""What the 64-piece build of the back_end optimiser rests on, checked without a GPU: the oracle at 33 to 64 pieces, the piece
counts of the scenes, that the oracle's plans of those scenes are not on a knife edge, the launch order (csrc/launch_order.h
through tests/harness/launch_order_check.cpp) and the CPU builder at max_pieces = 64 (tests/harness/flat_traj_check.cpp)."""
import copy
import os
import subprocess

import numpy as np
import pytest

from alore_legged_manipulator_amd.flat_traj import FrontEndParams, waypoint_path
from tests import backend_eval_cases as ec
from tests import backend_long_cases as lc
from tests import flat_traj_cases
from tests.test_flat_traj_build_cpu import compare, run, write_paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc")
ORDER_SRC = os.path.join(ROOT, "tests", "harness", "launch_order_check.cpp")
BUILDER_SRC = os.path.join(ROOT, "tests", "harness", "flat_traj_check.cpp")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def orc():
    from oracle.backend_driver import BackendOracle
    return BackendOracle()


# ---- the oracle at these counts
@pytest.mark.parametrize("grid", lc.GRIDS)
@pytest.mark.parametrize("stage", [1, 2])
def test_oracle_gradient_matches_central_differences_at_33_to_64_pieces(orc, stage, grid):
    """the bounds of tests/test_backend_eval_cpu.py: 1e-5 of the largest entry on the free map, 2e-4 with the obstacle term (exact
    chain there, and the cost must not depend on that switch); stage 1 with one time weight in cost and gradient"""
    fts, xs = lc.eval_problems(grid), lc.eval_vectors(grid)
    assert sorted(ft.pieces for ft in fts) == list(lc.COUNTS) and [ft.pieces for ft in fts] != list(lc.COUNTS)
    g = lc.grid_of(grid)
    kw = dict(lam=ec.LAM, rho=ec.RHO)
    if stage == 1:
        kw["time_weight"] = orc.cfg.p_time
    bound, exact = (1e-5, 0) if grid == "free" else (2e-4, 1)
    for ft, x in zip(fts, xs):
        assert len(x) == 3 * ft.pieces - 1
        with ec.oracle_config(orc, {}, exact_chain=0):
            plain = orc.eval(g, ft, stage, x, **kw)
        with ec.oracle_config(orc, {}, exact_chain=exact):
            r = orc.eval(g, ft, stage, x, **kw)
            fd = lc.fd_grad(orc, g, ft, stage, x, **kw)             # an absolute step: see there
        assert r["cost"] == plain["cost"]
        err = float(np.max(np.abs(fd - r["grad"])) / np.max(np.abs(fd)))
        print(f"stage {stage} {grid} M {ft.pieces}: |fd - grad| / max|fd| {err:.1e} (bound {bound:.0e})")
        assert err <= bound, (stage, grid, ft.pieces, err)


def test_the_disc_problems_meet_the_obstacle(orc):
    """the obstacle term is part of the stage-2 cost of every disc problem: without the map the cost is lower"""
    far = lc.free_grid()
    for ft, x in zip(lc.eval_problems("disc"), lc.eval_vectors("disc")):
        kw = dict(lam=ec.LAM, rho=ec.RHO)
        assert orc.eval(lc.disc_grid(), ft, 2, x, **kw)["cost"] > orc.eval(far, ft, 2, x, **kw)["cost"] + 1.0, ft.pieces


# ---- the scenes
def test_the_scenes_have_the_piece_counts_they_are_used_for():
    for pieces, pts in lc.ROUTES.items():
        assert waypoint_path(pts, 0, 1).pieces == pieces
        path = lc.route_path(pieces)
        assert flat_traj_cases.oracle(path, FrontEndParams()).pieces == pieces
        assert not flat_traj_cases.on_a_knife_edge(path, FrontEndParams()), pieces
    assert 32 < lc.past_disc().pieces <= 64
    assert tuple(ft.pieces for ft in lc.boxes_problems()) == lc.BOXES_PIECES
    comb = lc.searched_paths("comb")
    assert len(comb) == 1 and flat_traj_cases.oracle(comb[0], FrontEndParams()).pieces == lc.COMB_PIECES
    assert [ft.pieces for ft in lc.lbfgs_problems()] == [33, 64]
    assert [ft.pieces for ft in lc.batch_problems()] == [1, 16, 17, 32, 33, 64]


def scene_plans():
    return ([("route-%d" % m, lc.free_grid, lambda m=m: lc.route(m)) for m in (46, 59, 64)] + [("past-disc", lc.disc_grid, lc.past_disc)] +
            [("boxes-%d" % b, lc.boxes_grid, lambda b=b: lc.boxes_problems()[b]) for b in range(len(lc.BOXES_PIECES))])


@pytest.mark.parametrize("name,grid,problem", scene_plans(), ids=[s[0] for s in scene_plans()])
def test_the_oracles_plans_of_the_scenes_are_not_on_a_knife_edge(orc, name, grid, problem):
    """twelve 1e-14 perturbations of traj_pts (the method of test_minco_plan_matches_oracle_on_monte_carlo_goals): every run keeps
    ok and attempts = 1 and the cost moves by less than 10 % -- so the GPU tests may ask for the oracle's ok and attempts and for a
    cost within 10 %"""
    g, ft = grid(), problem()
    ref = orc.minco_plan(g, ft)
    assert ref["ok"] and ref["attempts"] == 1 and ref["min_dist"] > orc.cfg.final_min_safe_dis, name
    rng = np.random.default_rng(12)
    worst = 0.0
    for _ in range(12):
        f2 = copy.deepcopy(ft)
        f2.traj_pts = ft.traj_pts * (1 + 1e-14 * rng.standard_normal(ft.traj_pts.shape))
        per = orc.minco_plan(g, f2)
        assert per["ok"] and per["attempts"] == 1, name
        worst = max(worst, abs(per["cost"] - ref["cost"]) / abs(ref["cost"]))
    print(f"{name}: {ft.pieces} pieces, min_dist {ref['min_dist']:.3f}, cost moves by at most {100 * worst:.1f} %")
    assert worst < 0.10, (name, worst)


# ---- the launch order
@pytest.fixture(scope="module")
def order_exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("launch_order")
    out = {}
    for tag, flags in (("plain", ["-O2"]), ("asan_ubsan", SANITIZE)):
        out[tag] = str(d / tag)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, ORDER_SRC, "-o", out[tag]])
    return out


def launch_order(exe, P, pieces, tmp_path):
    infile = str(tmp_path / "pieces.txt")
    with open(infile, "w") as f:
        f.write("%d %d\n" % (P, len(pieces)) + " ".join(str(int(v)) for v in pieces) + "\n")
    r = subprocess.run([exe, infile], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.array([int(v) for v in r.stdout.split()], np.int64)


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
@pytest.mark.parametrize("count", [1, 255, 256, 257, 5000])
def test_launch_order_is_a_stable_sort_by_descending_piece_count(order_exes, build, count, tmp_path):
    rng = np.random.default_rng(count)
    pieces = rng.integers(0, 65, count)
    got = launch_order(order_exes[build], 64, pieces, tmp_path)
    assert np.array_equal(got, lc.stable_order(pieces)), count
    # counts of at most 32: the shape of the 16- and 32-piece builds and that of the 64-piece build give the same order
    small = rng.integers(0, 33, count)
    a, b = launch_order(order_exes[build], 32, small, tmp_path), launch_order(order_exes[build], 64, small, tmp_path)
    assert np.array_equal(a, lc.stable_order(small)) and np.array_equal(a, b), count


def test_launch_order_clamps_counts_outside_the_buckets(order_exes, tmp_path):
    """a slot that was never built may hold anything: it sorts with the nearest count and nothing is written out of range (the
    sanitizer build)"""
    pieces = np.array([70, -3, 64, 0, 65, 33, 1 << 30, -(1 << 30)])
    got = launch_order(order_exes["asan_ubsan"], 64, pieces, tmp_path)
    assert np.array_equal(got, lc.stable_order(np.clip(pieces, 0, 64)))
    got = launch_order(order_exes["asan_ubsan"], 32, pieces, tmp_path)
    assert np.array_equal(got, lc.stable_order(np.clip(pieces, 0, 32)))


# ---- the CPU builder
@pytest.mark.parametrize("flags", [["-O2"], SANITIZE], ids=["plain", "asan_ubsan"])
def test_the_cpu_builder_takes_64_pieces_and_refuses_69(flags, tmp_path):
    exe, infile = str(tmp_path / "flat_traj_check"), str(tmp_path / "paths.txt")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, BUILDER_SRC, "-o", exe])
    prm = FrontEndParams()
    paths = [lc.route_path(64), lc.route_path(69), lc.route_path(46), lc.searched_paths("comb")[0]]
    write_paths(infile, paths, prm, 64)
    got = run(exe, infile)
    assert [g["status"] for g in got] == [0, -2, 0, -2]
    compare(got[0], flat_traj_cases.oracle(paths[0], prm), 0)
    compare(got[2], flat_traj_cases.oracle(paths[2], prm), 2)
    write_paths(infile, paths[:1] + paths[2:3], prm, 32)               # a 32-piece slot refuses both
    assert [g["status"] for g in run(exe, infile)] == [-2, -2]
