"""csrc/path_search.h (way-point paths by grid search) on the CPU against its oracle, tests/path_search_cases.py, and the build
side of the feature: the alore_backend_search_* calls are declared, exported and bound, the kernel is in the gfx950 code object.

tests/harness/path_search_check.cpp includes the header, is compiled with g++ (once more as a stand-alone program with the address
and undefined-behaviour sanitizers) and runs the scenes through psearch::search_one: the header's own sweeps, walk and pruning.
Status, cost pair, point count and coordinates are compared with the oracle's Dijkstra for EQUALITY: the field is exact integer
pairs, every coordinate a correctly rounded double operation, contraction off on both sides."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import path_search_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "harness", "path_search_check.cpp")
LIB = os.path.join(ROOT, "alore_legged_manipulator_amd", "libalore_nmpc.so")
FLAGS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
SEARCH_CALLS = ("alore_backend_search_default_params", "alore_backend_search_paths", "alore_backend_device_paths",
                "alore_backend_device_search_status", "alore_backend_search_status", "alore_backend_get_paths", "alore_backend_search_sweeps")
ALL = list(cases.SCENES) + [("random", k) for k in range(cases.RANDOM_FIELDS)]


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("path_search_check")
    out = {}
    for name, flags in FLAGS.items():
        out[name] = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC, SRC, "-o", out[name]])
    return out


def run(exe, s, path):
    m = s["map"]
    with open(path, "w") as f:
        f.write("%d %d %r %r %r %d\n" % (m.nx, m.ny, m.x_lo, m.y_lo, m.res, len(s["problems"])))
        f.write(" ".join("%.17g" % v for v in m.dist.reshape(-1)) + "\n")
        for a, b in s["problems"]:
            f.write("%r %r %r %r %r %r\n" % (float(a[0]), float(a[1]), float(b[0]), float(b[1]), s["safe_dis"], s["margin"]))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    out = []
    for k in range(len(s["problems"])):
        status, n, a, b, sweeps = (int(v) for v in lines[2 * k].split())
        xy = np.array([float(v) for v in lines[2 * k + 1].split()]).reshape(cases.K, 2)
        out.append((status, n, (a, b), sweeps, xy))
    return out


def same_as_oracle(got, want, where):
    status, n, cost, _, xy = got
    assert status == want.status and n == want.n_points, (where, status, n, want.status, want.n_points)
    if want.status == cases.OK:
        assert cost == want.cost, (where, cost, want.cost)
        assert xy[:n].tolist() == [list(p) for p in want.xy], where
    assert (xy[n:] == cases.SENTINEL).all(), where                      # nothing written beyond the path, nothing at all on failure


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
@pytest.mark.parametrize("name", ALL, ids=str)
def test_header_equals_the_oracle(exes, build, name, tmp_path):
    s = cases.get_scene(name)
    got = run(exes[build], s, str(tmp_path / "problems.txt"))
    for k, (g, w) in enumerate(zip(got, cases.expected(name))):
        same_as_oracle(g, w, (name, k))


@pytest.mark.parametrize("name", ALL, ids=str)
def test_paths_are_connected_free_and_cost_what_the_field_says(name):
    s = cases.get_scene(name)
    for (a, b), r in zip(s["problems"], cases.expected(name)):
        cases.check_result(s["map"], a, b, r)


def test_the_scenes_hold_what_they_should():
    st = {name: [r.status for r in cases.expected(name)] for name in cases.SCENES}
    ex = cases.expected
    assert st["open"] == [0, 0, 0] and all(len(r.raw) <= 3 for r in ex("open"))                 # at most one turn
    assert ex("open")[1].n_points == 2 and ex("open")[1].cost == (41, 0)
    assert st["wall_gap"] == [0, 0] and all(r.n_points >= 3 for r in ex("wall_gap"))
    diag = np.hypot(cases.NX, cases.NY)
    assert st["spiral"] == [0, 0] and all(cases.key(r.cost) > 3.5 * diag for r in ex("spiral")) # several times the window's diagonal
    assert ex("spiral")[0].n_points == cases.K                                                  # ... and exactly as many way-points as fit
    assert st["box"] == [cases.E_NO_PATH] and len(ex("box")[0].field) > 20                      # the goal's side was searched
    for r, (cx, cy) in zip(ex("corner"), ((0, 0), (cases.NX - 1, cases.NY - 1))):
        x0, y0, x1, y1 = r.window
        assert r.status == 0 and (cx in (x0, x1)) and (cy in (y0, y1)) and x1 - x0 < cases.NX - 1 and y1 - y0 < cases.NY - 1
    assert st["detour"] == [0] and st["detour_tight"] == [cases.E_NO_PATH]
    assert ex("detour")[0].window != ex("detour_tight")[0].window
    for r in ex("safe_rule"):
        assert r.status == 0 and 0 < r.safe < cases.SAFE_DIS
    m = cases.scene("safe_rule")["map"]
    assert any((m.dist[c] < cases.SAFE_DIS) for r in ex("safe_rule") for c in r.raw)            # ... and the path uses what the cap freed
    assert st["bad"] == [cases.E_SAME_CELL] + [cases.E_ENDPOINT] * 5 + [0]
    assert st["serpentine"] == [cases.E_POINTS, 0] and len(ex("serpentine")[0].raw) > cases.K
    assert ex("serpentine")[1].n_points > 8
    assert st["window"] == [cases.E_WINDOW, 0]


def test_at_most_a_quarter_of_the_random_problems_have_no_path():
    share, res = cases.random_no_path_share()
    assert len(res) == 200 and share <= 0.25, share
    assert sum(r.status == 0 for r in res) >= 140
    assert len({r.n_points for r in res}) >= 4


# ---- the build side ---------------------------------------------------------------------------------------------------------
def test_search_calls_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alore_backend.h")).read(), flags=re.S)
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    from alore_legged_manipulator_amd import _lib, backend
    lib = _lib.load()
    backend._bind(lib)
    for name in SEARCH_CALLS:
        assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", hdr), name
        assert re.search(r"\sT\s+" + name + r"$", syms, re.M), name
        assert getattr(lib, name).argtypes is not None, name
    for method in ("search_paths", "search_paths_device", "device_paths", "search_status", "paths", "search_sweeps"):
        assert hasattr(backend.BatchedMSPlanner, method), method
    for k, v in (("OK", 0), ("MASKED", 1), ("E_ENDPOINT", -1), ("E_SAME_CELL", -2), ("E_WINDOW", -3), ("E_NO_PATH", -4), ("E_POINTS", -5)):
        assert re.search(r"#define\s+ALORE_BE_SEARCH_%s\s+\(?%d\)?" % (k, v), hdr), k
        assert getattr(backend, "SEARCH_" + k) == v == getattr(cases, k)
    assert re.search(r"#define\s+ALORE_BE_SEARCH_MAX_CELLS\s+32768", hdr)


def test_struct_mirrors_have_the_c_layout(tmp_path):
    from alore_legged_manipulator_amd import backend
    code = ('#include <stdio.h>\n#include "alore_backend.h"\nint main(){printf("%zu %zu", sizeof(alore_backend_search_params), '
            'sizeof(alore_backend_paths));}')
    (tmp_path / "s.c").write_text(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    sizes = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert sizes == [C.sizeof(backend.SearchParamsC), C.sizeof(backend.PathsC)]


def test_default_search_params_need_no_gpu():
    from alore_legged_manipulator_amd import backend
    p = backend.default_search_params()
    assert (p.safe_dis, p.window_margin) == (0.3, 3.0)


def test_the_kernel_is_in_the_gfx950_code_object():
    blob = open(LIB, "rb").read()
    assert b"search_paths_kernel" in blob and b"gfx950" in blob
