"""csrc/task_plan_wide.h (task_plan's missions on windows beyond LDS: every field on a slab, relaxed tile by tile, the range rule) on
the CPU against its oracles, and the build side of the feature.

tests/harness/task_plan_wide_check.cpp runs tplan::plan_one_wide, which computes EVERY field by the tiled iteration, at tile sizes
8 x 8, 5 x 7 and 126 x 126, compiled with g++ plain and as a stand-alone program with the address and undefined-behaviour
sanitizers.
  * every scene of tests/task_plan_cases.py and tests/task_assign_cases.py (windows of a few thousand cells, dozens of tiles at the
    small sizes) must equal those modules' expected(): oracles nobody touched pin the wiring of tiles, roots and costs.  The one
    exception is `window` (130 321 cells, E_WINDOW there): under a cap of 160 000 cells it is planned, and compared with plan_wide;
  * the wide scenes of tests/task_plan_wide_cases.py must equal plan_wide, in their own mode at every tile size and build and in
    all four modes at 126 x 126.
Every comparison is ==: status, matrix, order, n_order, total, legs, fields and the assignment rows, sentinels included."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import task_assign_cases as ta
from tests import task_plan_cases as tc
from tests import task_plan_wide_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "harness", "task_plan_wide_check.cpp")
LIB = os.path.join(ROOT, "alore_legged_manipulator_amd", "libalore_nmpc.so")
FLAGS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
TILES = ("8x8", "5x7", "126x126")
KEYS = ("matrix", "order", "total", "leg_start_xy", "leg_goal_xy", "assignment", "assign_total")
NARROW = ([(tc, n) for n in list(tc.SCENES) + [("random", tc.GREEDY), ("random", tc.OPTIMAL)]] +
          [(ta, n) for n in list(ta.SCENES) + [("random", ta.ASSIGNED), ("random", ta.JOINT)]])
WINDOW_CAP = 160000


def compile_harness(path, flags):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC, SRC, "-o", path])
    return path


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("task_plan_wide_check")
    return {name: compile_harness(str(d / name), flags) for name, flags in FLAGS.items()}


def ints(line):
    return np.array([int(v) for v in line.split()], np.int32)


def run(exe, s, path, tiles, max_cells, mode=None, inputs=None):
    """the missions of scene s (inputs: its arrays) through the harness in `mode` (None: the scene's own)"""
    m = s["map"]
    n_tasks, pts, asg = inputs if inputs is not None else cases.arrays(s)
    with open(path, "w") as f:
        f.write("%d %d %r %r %r %d %d %d %r %r %d\n" % (m.nx, m.ny, m.x_lo, m.y_lo, m.res, len(n_tasks), s["max_tasks"],
                                                      s["mode"] if mode is None else mode, s["safe_dis"], s["margin"], asg is not None))
        f.write(" ".join("%.17g" % v for v in m.dist.reshape(-1)) + "\n")
        for k in range(len(n_tasks)):
            f.write("%d %s\n" % (n_tasks[k], " ".join(repr(float(v)) for v in pts[k].reshape(-1))))
            if asg is not None:
                f.write(" ".join(str(int(v)) for v in asg[k]) + "\n")
    r = subprocess.run([exe, path, tiles, str(max_cells)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    out = []
    for k in range(len(n_tasks)):
        status, n_order, t_a, t_b, fields, sweeps = (int(v) for v in lines[7 * k].split())
        dbl = lambda line: np.array([float(v) for v in line.split()]).reshape(cases.MAX_LEGS, 2)
        out.append({"status": status, "n_order": n_order, "total": np.array([t_a, t_b], np.int32), "fields": fields, "sweeps": sweeps,
                    "matrix": ints(lines[7 * k + 1]).reshape(cases.P_MAX, cases.P_MAX, 2), "order": ints(lines[7 * k + 2]),
                    "leg_start_xy": dbl(lines[7 * k + 3]), "leg_goal_xy": dbl(lines[7 * k + 4]), "assignment": ints(lines[7 * k + 5]),
                    "assign_total": ints(lines[7 * k + 6])})
    return out


def want_arrays(r):
    """the expected rows of a Result of any of the three oracles"""
    if hasattr(r, "assignment"):
        return cases.expected_arrays(r)
    out = tc.expected_arrays(r)
    out["assignment"], out["assign_total"] = np.full(cases.MAX_TASKS, cases.FILL_I, np.int32), np.full(2, cases.FILL_I, np.int32)
    return out


def same_as_oracle(got, want, where):
    w = want_arrays(want)
    assert got["status"] == w["status"] and got["n_order"] == w["n_order"] and got["fields"] == w["fields"], \
        (where, got["status"], got["n_order"], got["fields"], w["status"], w["n_order"], w["fields"])
    for k in KEYS:
        if w[k] is not None:                                               # the matrix of an E_RANGE mission is unspecified
            assert np.array_equal(got[k], w[k]), (where, k, got[k], w[k])
    assert (got["sweeps"] == cases.FILL_I) if want.fields is None else got["sweeps"] >= 1, (where, got["sweeps"])


_CACHE = {}


def window_expected():
    """the scene `window` of task_plan_cases under a cap that admits its 361 x 361 window"""
    if "window" not in _CACHE:
        s = tc.scene("window")
        _CACHE["window"] = tuple(cases.plan_wide(s["map"], ms["n"], s["max_tasks"], ms["pts"], None, s["mode"], s["safe_dis"], s["margin"], WINDOW_CAP)
                                 for ms in s["missions"])
    return _CACHE["window"]


@pytest.mark.parametrize("build", list(FLAGS))
@pytest.mark.parametrize("tiles", TILES)
def test_tiled_fields_equal_the_untouched_oracles_on_their_own_scenes(exes, build, tiles, tmp_path):
    multi = 0
    for mod, name in NARROW:
        s = mod.get_scene(name)
        want = window_expected() if name == "window" else mod.expected(name)
        got = run(exes[build], s, str(tmp_path / "missions.txt"), tiles, WINDOW_CAP if name == "window" else cases.RESERVED, inputs=mod.arrays(s))
        for k, (g, w) in enumerate(zip(got, want)):
            same_as_oracle(g, w, (name, k, tiles))
            multi += g["sweeps"] > 1
    assert tiles == "126x126" or multi >= 100                              # small tiles: most missions had a field of several visits
    far, near = window_expected()
    assert tc.expected("window")[0].status == tc.E_WINDOW and far.status == near.status == 0
    assert cases.window_cells(far) == 361 * 361 and far.order == [0, 0] and far.fields == 2


@pytest.mark.parametrize("build", list(FLAGS))
@pytest.mark.parametrize("tiles", TILES)
@pytest.mark.parametrize("name", cases.WIDE_SCENES)
def test_tiled_fields_equal_plan_wide_on_the_wide_scenes(exes, build, tiles, name, tmp_path):
    s = cases.scene(name)
    got = run(exes[build], s, str(tmp_path / "missions.txt"), tiles, s["reserved"])
    for k, (g, w) in enumerate(zip(got, cases.expected(name))):
        if w.status != cases.MASKED:                                       # the harness knows no mask
            same_as_oracle(g, w, (name, k, tiles))


@pytest.mark.parametrize("mode", cases.MODES, ids=cases.MODE_IDS)
@pytest.mark.parametrize("name", cases.WIDE_SCENES)
def test_every_mode_on_the_wide_scenes(exes, name, mode, tmp_path):
    s = cases.scene(name)
    got = run(exes["plain"], s, str(tmp_path / "missions.txt"), "126x126", s["reserved"], mode)
    for k, (g, w) in enumerate(zip(got, cases.expected(name, mode))):
        if w.status != cases.MASKED:
            same_as_oracle(g, w, (name, k, mode))


def test_a_window_beyond_the_cap_is_refused_and_the_order_of_the_checks_holds(exes, tmp_path):
    s = cases.scene("mixed")
    got = run(exes["plain"], s, str(tmp_path / "missions.txt"), "8x8", 50000)
    want = cases.expected("mixed", None, 50000)
    assert [w.status for w in want] == [cases.E_WINDOW, cases.MASKED, cases.E_TASKS, 0, cases.E_ENDPOINT, 0, cases.E_WINDOW]
    for k, (g, w) in enumerate(zip(got, want)):
        if w.status != cases.MASKED:
            same_as_oracle(g, w, ("mixed at 50000", k))
    m, nan = s["map"], float("nan")
    far = [(-12.0, -9.0), (12.0, 9.0), (nan, 0.0)]
    # tasks before end point before window
    assert cases.plan_wide(m, 0, 1, far, max_cells=40000).status == cases.E_TASKS
    assert cases.plan_wide(m, 1, 1, far, max_cells=40000).status == cases.E_ENDPOINT
    assert cases.plan_wide(m, 1, 1, far[:2] + [(0.0, 0.0)], max_cells=40000).status == cases.E_WINDOW
    assert cases.plan_wide(m, 6, 10, far, mode=cases.JOINT).status == cases.E_TASKS


def test_plan_wide_is_plan_below_the_cap():
    """the oracle against the modules it was put together from, on every scene they have: the fields rooted the other way round
    give the same matrix, and everything behind the matrix is those modules' own"""
    for mod, name in NARROW:
        s = mod.get_scene(name)
        for ms, w in zip(s["missions"], mod.expected(name)):
            r = cases.plan_wide(s["map"], ms["n"], s["max_tasks"], ms["pts"], ms["assign"], s["mode"], s["safe_dis"], s["margin"], tc.ps.MAX_CELLS)
            assert (r.status, r.matrix, r.order, r.total, r.legs, r.fields) == (w.status, w.matrix, w.order, w.total, w.legs, w.fields), name
            assert (r.assignment, r.assign_total) == (getattr(w, "assignment", None), getattr(w, "assign_total", None)), name


def test_the_scenes_hold_what_they_should():
    ex = cases.expected
    one, three, narrow, walls = ex("boxes")
    assert [r.status for r in ex("boxes")] == [0] * 4 and [cases.window_cells(r) for r in ex("boxes")] == [52000, 52000, 5566, 43680]
    assert (one.fields, three.fields, walls.fields) == (2, 6, 3)           # near walls: two fields from source 0 on one slab in a row
    assert three.order[1::2] == [[1, 2, 0][i] for i in three.order[0::2]] and len(three.order) == 6
    assert cases.less(ex("boxes", cases.ASSIGNED)[1].total, three.total) and ex("boxes", cases.ASSIGNED)[1].assignment == [1, 0, 2]
    open_, = ex("open")
    assert (open_.status, open_.fields, cases.window_cells(open_), len(open_.order)) == (0, 20, 52000, 20)
    assert open_.assignment != list(range(10)) and ex("open", cases.JOINT)[0].status == cases.E_TASKS
    comb, = ex("comb")
    assert comb.status == 0 and cases.window_cells(comb) == 52000 and comb.matrix[0, 1] == (896, 220)   # the wide search's comb
    g, = ex("closed")
    assert (g.status, len(g.order), cases.window_cells(g)) == (0, 1, 43296) and g.order == [0]          # greedy stops after an item
    assert sum(v == cases.INF for v in g.matrix.values()) == 12                                          # 2 inside, 3 outside
    for mode in (cases.OPTIMAL, cases.ASSIGNED, cases.JOINT):
        r, = ex("closed", mode)
        assert r.status == cases.E_NO_ORDER and r.matrix == g.matrix and r.assignment is None
    lds, first_wide = ex("edge")
    assert (lds.status, cases.window_cells(lds), first_wide.status, cases.window_cells(first_wide)) == (0, 32768, 0, 32896)
    for mode in cases.MODES:
        r, = ex("serpentine_range", mode)
        assert r.status == cases.E_RANGE and cases.window_cells(r) == 72000 and r.fields == 2
        assert r.matrix[0, 1] != cases.INF and max(r.matrix[0, 1]) > 35000                               # a route exists
    assert [r.status for r in ex("mixed")] == [0, cases.MASKED, cases.E_TASKS, 0, cases.E_ENDPOINT, 0, 0]
    # without the reservation, or with a smaller one, the same missions are E_WINDOW
    assert [r.status for r in ex("boxes", None, tc.ps.MAX_CELLS)] == [cases.E_WINDOW, cases.E_WINDOW, 0, cases.E_WINDOW]
    assert [r.status for r in ex("boxes", None, 50000)] == [cases.E_WINDOW, cases.E_WINDOW, 0, 0]
    assert [r.status for r in ex("edge", None, tc.ps.MAX_CELLS)] == [0, cases.E_WINDOW]
    # the Dijkstra budget: the fields of all wide scenes (`mixed` has the missions of `boxes` again), of at most 72 000 cells each
    assert sum(r.fields for name in cases.WIDE_SCENES if name != "mixed" for r in ex(name)) == 45


# ---- the build side ---------------------------------------------------------------------------------------------------------
def test_reservation_calls_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alore_backend.h")).read(), flags=re.S)
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    from alore_legged_manipulator_amd import _lib, backend
    lib = _lib.load()
    backend._bind(lib)
    for name in ("alore_backend_task_reserve", "alore_backend_task_reserved"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert re.search(r"\sT\s+" + name + r"$", syms, re.M), name
        assert getattr(lib, name).argtypes is not None, name
    for method in ("task_reserve", "task_reserved"):
        assert hasattr(backend.BatchedMSPlanner, method), method
    assert re.search(r"#define\s+ALORE_BE_TASK_E_RANGE\s+\(-8\)", hdr)
    assert backend.TASK_E_RANGE == -8 == cases.E_RANGE and backend.TASK_E_TASKS == -6 == backend.SEARCH_E_RANGE
    src = open(os.path.join(CSRC, "task_plan.h")).read()
    assert re.search(r"constexpr int E_RANGE = -8;", src)


def test_the_wide_kernel_is_in_the_gfx950_code_object():
    blob = open(LIB, "rb").read()
    assert b"task_costs_wide_kernel" in blob and b"gfx950" in blob
