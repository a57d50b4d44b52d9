"""csrc/path_search_wide.h (the grid search on windows beyond LDS: tiles, halo, dirty flags, the range rule) on the CPU against
its oracles, and the build side of the feature.

tests/harness/path_search_wide_check.cpp runs psearch::search_one_wide, which searches EVERY window by the tiled iteration, at
tile sizes 8 x 8, 5 x 7 and 126 x 126, compiled with g++ plain and as a stand-alone program with the address and undefined-
behaviour sanitizers.
  * every scene of tests/path_search_cases.py (windows of a few thousand cells, dozens of tiles at the small sizes) must equal
    that module's expected(): an oracle nobody touched pins the tile, halo and dirty-flag arithmetic.  The one exception is the
    first problem of `window` (40 000 cells, E_WINDOW there): forced onto the tiled route it is searched, and is compared with
    search_wide;
  * the wide scenes of tests/path_search_wide_cases.py must equal search_wide.
Every comparison is ==: status, cost pair, point count, coordinates, and sentinels beyond the path."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import path_search_cases as cases
from tests import path_search_wide_cases as wide

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "harness", "path_search_wide_check.cpp")
LIB = os.path.join(ROOT, "alore_legged_manipulator_amd", "libalore_nmpc.so")
FLAGS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
TILES = ("8x8", "5x7", "126x126")
NARROW = list(cases.SCENES) + [("random", k) for k in range(cases.RANDOM_FIELDS)]


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("path_search_wide_check")
    out = {}
    for name, flags in FLAGS.items():
        out[name] = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC, SRC, "-o", out[name]])
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the problems file of a scene, written once"""
    d, made = tmp_path_factory.mktemp("path_search_wide_problems"), {}

    def get(key, s):
        if key not in made:
            m, path = s["map"], str(d / ("%d.txt" % len(made)))
            with open(path, "w") as f:
                f.write("%d %d %r %r %r %d\n" % (m.nx, m.ny, m.x_lo, m.y_lo, m.res, len(s["problems"])))
                f.write(" ".join("%.17g" % v for v in m.dist.reshape(-1)) + "\n")
                for a, b in s["problems"]:
                    f.write("%r %r %r %r %r %r\n" % (float(a[0]), float(a[1]), float(b[0]), float(b[1]), s["safe_dis"], s["margin"]))
            made[key] = path
        return made[key]
    return get


def run(exe, tiles, max_cells, path, n):
    r = subprocess.run([exe, path, tiles, str(max_cells)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    out = []
    for k in range(n):
        status, npts, a, b, visits = (int(v) for v in lines[2 * k].split())
        xy = np.array([float(v) for v in lines[2 * k + 1].split()]).reshape(cases.K, 2)
        out.append((status, npts, (a, b), visits, xy))
    return out


def same_as_oracle(got, want, where):
    status, n, cost, _, xy = got
    assert status == want.status and n == want.n_points, (where, status, n, want.status, want.n_points)
    if want.status == cases.OK:
        assert cost == want.cost, (where, cost, want.cost)
        assert xy[:n].tolist() == [list(p) for p in want.xy], where
    assert (xy[n:] == cases.SENTINEL).all(), where                      # nothing written beyond the path, nothing at all on failure


def narrow_expected(name):
    """cases.expected, but the 40 000-cell problem of `window` by search_wide: the harness searches it"""
    want = list(cases.expected(name))
    if name == "window":
        s = cases.scene("window")
        assert want[0].status == cases.E_WINDOW
        want[0] = _window_0(s)
    return want


_CACHE = {}


def _window_0(s):
    if "w0" not in _CACHE:
        a, b = s["problems"][0]
        _CACHE["w0"] = wide.search_wide(s["map"], a, b, s["safe_dis"], s["margin"], wide.RESERVED)
    return _CACHE["w0"]


@pytest.mark.parametrize("build", list(FLAGS))
@pytest.mark.parametrize("tiles", TILES)
def test_tiled_search_equals_the_untouched_oracle_on_its_own_scenes(exes, files, build, tiles):
    multi = 0
    for name in NARROW:
        s = cases.get_scene(name)
        got = run(exes[build], tiles, wide.RESERVED, files(("narrow", name), s), len(s["problems"]))
        for k, (g, w) in enumerate(zip(got, narrow_expected(name))):
            same_as_oracle(g, w, (name, k, tiles))
            multi += g[3] > 1
    assert tiles == "126x126" or multi >= 100                           # small tiles: most problems needed several visits
    s = cases.scene("window")
    w0 = _window_0(s)
    assert w0.status == 0 and w0.cost == (340, 40) and wide.window_cells(w0) == 40000


@pytest.mark.parametrize("build", list(FLAGS))
@pytest.mark.parametrize("tiles", TILES)
@pytest.mark.parametrize("name", wide.WIDE_SCENES)
def test_tiled_search_equals_search_wide_on_the_wide_scenes(exes, files, build, tiles, name):
    s = wide.wide_scene(name)
    got = run(exes[build], tiles, wide.RESERVED, files(("wide", name), s), len(s["problems"]))
    for k, (g, w) in enumerate(zip(got, wide.wide_expected(name))):
        same_as_oracle(g, w, (name, k, tiles))


def test_a_window_beyond_the_cap_is_refused_and_the_order_of_the_statuses_holds(exes, files):
    s = wide.wide_scene("boxes")
    got = run(exes["plain"], "8x8", 50000, files(("wide", "boxes"), s), len(s["problems"]))
    want = wide.wide_expected("boxes", 50000)
    assert [w.status for w in want] == [cases.E_WINDOW] * 4 + [0, 0, 0]
    for k, (g, w) in enumerate(zip(got, want)):
        same_as_oracle(g, w, ("boxes at 50000", k))
    m = s["map"]
    nan = float("nan")
    # end point before same cell before window, as in setup
    assert wide.search_wide(m, (nan, 0.0), (1.0, 1.0), max_cells=40000).status == cases.E_ENDPOINT
    assert wide.search_wide(m, (1.0, 1.0), (1.01, 1.01), max_cells=40000).status == cases.E_SAME_CELL


def test_search_wide_is_search_below_the_cap():
    """the restated walk and pruning against the module they were restated from, on every scene it has"""
    for name in NARROW:
        s = cases.get_scene(name)
        for (a, b), w in zip(s["problems"], cases.expected(name)):
            r = wide.search_wide(s["map"], a, b, s["safe_dis"], s["margin"], cases.MAX_CELLS)
            assert (r.status, r.n_points, r.xy, r.cost, r.raw) == (w.status, w.n_points, w.xy, w.cost, w.raw), name


def test_paths_of_the_wide_scenes_are_connected_free_and_cost_what_the_field_says():
    for name in wide.WIDE_SCENES:
        s = wide.wide_scene(name)
        for (a, b), r in zip(s["problems"], wide.wide_expected(name)):
            if r.status != wide.E_RANGE:
                cases.check_result(s["map"], a, b, r)


def test_the_scenes_hold_what_they_should():
    ex = wide.wide_expected
    boxes = ex("boxes")
    assert [r.status for r in boxes] == [0] * 7
    assert [wide.window_cells(r) for r in boxes[:5]] == [52000] * 4 + [46200]              # 3 x 2 tiles of 126, ragged edges 8 and 74
    assert all(wide.window_cells(r) <= cases.MAX_CELLS for r in boxes[5:])                 # the LDS route in the same call
    assert all(3 <= r.n_points <= 6 for r in boxes[:5]) and boxes[0].cost == (60, 193)
    comb, = ex("comb")
    assert (comb.status, comb.n_points, comb.cost, wide.window_cells(comb)) == (0, 26, (896, 220), 52000)
    tight, = ex("comb_tight")
    assert (tight.status, wide.window_cells(tight)) == (cases.E_NO_PATH, 15860)            # ... which a 3 m margin cannot find
    closed, = ex("closed")
    assert (closed.status, wide.window_cells(closed), len(closed.field)) == (cases.E_NO_PATH, 48216, 841)
    lds, first_wide = ex("edge")
    assert (lds.status, lds.n_points, lds.cost, wide.window_cells(lds)) == (0, 2, (128, 67), 32768)
    assert (first_wide.status, first_wide.n_points, first_wide.cost, wide.window_cells(first_wide)) == (0, 2, (129, 67), 32896)
    rng, = ex("serpentine_range")
    assert rng.status == wide.E_RANGE and wide.window_cells(rng) == 72000 and len(rng.field) == 36389
    assert max(max(p) for p in rng.field.values()) > 35000
    s = wide.wide_scene("serpentine_range")
    start = s["map"].cell(*s["problems"][0][0])
    assert start in rng.field                                                               # the walk would find a path
    # without the reservation, or with a smaller one, the same problems are E_WINDOW
    assert [r.status for r in ex("boxes", cases.MAX_CELLS)] == [cases.E_WINDOW] * 5 + [0, 0]
    assert [r.status for r in ex("edge", 40000)] == [0, 0] and [r.status for r in ex("boxes", 40000)][:5] == [cases.E_WINDOW] * 5


# ---- the build side ---------------------------------------------------------------------------------------------------------
def test_reservation_calls_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alore_backend.h")).read(), flags=re.S)
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    from alore_legged_manipulator_amd import _lib, backend
    lib = _lib.load()
    backend._bind(lib)
    for name in ("alore_backend_search_reserve", "alore_backend_search_reserved", "alore_backend_search_wide_ticks"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert re.search(r"\sT\s+" + name + r"$", syms, re.M), name
        assert getattr(lib, name).argtypes is not None, name
    for method in ("search_reserve", "search_reserved", "search_wide_ticks"):
        assert hasattr(backend.BatchedMSPlanner, method), method
    assert re.search(r"#define\s+ALORE_BE_SEARCH_E_RANGE\s+\(-6\)", hdr)
    assert backend.SEARCH_E_RANGE == -6 == wide.E_RANGE
    src = open(os.path.join(CSRC, "path_search_wide.h")).read()
    assert re.search(r"constexpr int E_RANGE = -6;", src) and re.search(r"RANGE_LIMIT = 32767u;", src)
    assert re.search(r"WIDE_MAX_CELLS = 1 << 22;", src) and wide.WIDE_MAX_CELLS == 1 << 22 and wide.RANGE_LIMIT == 32767


def test_the_wide_kernel_is_in_the_gfx950_code_object():
    blob = open(LIB, "rb").read()
    assert b"search_paths_wide_kernel" in blob and b"gfx950" in blob
