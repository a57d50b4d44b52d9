"""csrc/task_plan.h (the visit order of a rearrangement mission from path costs) on the CPU against its oracle,
tests/task_plan_cases.py, and the build side of the feature: the alore_backend_task_* calls are declared, exported and bound, the
kernels are in the gfx950 code object.

tests/harness/task_plan_check.cpp includes the header, is compiled with g++ (once more as a stand-alone program with the address
and undefined-behaviour sanitizers) and runs the scenes through tplan::plan_one: the header's own fields by sweeps, its greedy order
and its dynamic programme over subsets.  Every row of the result is pre-filled and compared with the oracle's for EQUALITY, what
must stay untouched included: costs are exact integer pairs, the orders follow written tie rules."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import task_plan_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "harness", "task_plan_check.cpp")
LIB = os.path.join(ROOT, "alore_legged_manipulator_amd", "libalore_nmpc.so")
FLAGS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
TASK_CALLS = ("alore_backend_task_default_params", "alore_backend_task_plan", "alore_backend_device_task", "alore_backend_get_task")
ALL = list(cases.SCENES) + [("random", cases.GREEDY), ("random", cases.OPTIMAL)]
KEYS = ("matrix", "order", "total", "leg_start_xy", "leg_goal_xy")


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("task_plan_check")
    out = {}
    for name, flags in FLAGS.items():
        out[name] = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC, SRC, "-o", out[name]])
    return out


def run(exe, s, path):
    m = s["map"]
    n_tasks, pts, asg = cases.arrays(s)
    with open(path, "w") as f:
        f.write("%d %d %r %r %r %d %d %d %r %r %d\n" % (m.nx, m.ny, m.x_lo, m.y_lo, m.res, len(n_tasks), s["max_tasks"], s["mode"],
                                                      s["safe_dis"], s["margin"], asg is not None))
        f.write(" ".join("%.17g" % v for v in m.dist.reshape(-1)) + "\n")
        for k in range(len(n_tasks)):
            f.write("%d %s\n" % (n_tasks[k], " ".join(repr(float(v)) for v in pts[k].reshape(-1))))
            if asg is not None:
                f.write(" ".join(str(int(v)) for v in asg[k]) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    out = []
    for k in range(len(n_tasks)):
        status, n_order, ta, tb, fields, sweeps = (int(v) for v in lines[5 * k].split())
        ints = lambda line: np.array([int(v) for v in line.split()], np.int32)
        dbl = lambda line: np.array([float(v) for v in line.split()]).reshape(cases.MAX_LEGS, 2)
        out.append({"status": status, "n_order": n_order, "total": np.array([ta, tb], np.int32), "fields": fields, "sweeps": sweeps,
                    "matrix": ints(lines[5 * k + 1]).reshape(cases.P_MAX, cases.P_MAX, 2), "order": ints(lines[5 * k + 2]),
                    "leg_start_xy": dbl(lines[5 * k + 3]), "leg_goal_xy": dbl(lines[5 * k + 4])})
    return out


def same_as_oracle(got, want, where):
    w = cases.expected_arrays(want)
    assert got["status"] == w["status"] and got["n_order"] == w["n_order"] and got["fields"] == w["fields"], \
        (where, got["status"], got["n_order"], got["fields"], w["status"], w["n_order"], w["fields"])
    for k in KEYS:
        assert np.array_equal(got[k], w[k]), (where, k, got[k], w[k])
    assert (got["sweeps"] == cases.FILL_I) if want.fields is None else got["sweeps"] >= 1, (where, got["sweeps"])


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
@pytest.mark.parametrize("name", ALL, ids=str)
def test_header_equals_the_oracle(exes, build, name, tmp_path):
    s = cases.get_scene(name)
    got = run(exes[build], s, str(tmp_path / "missions.txt"))
    for k, (g, w) in enumerate(zip(got, cases.expected(name))):
        same_as_oracle(g, w, (name, k))


def test_held_karp_equals_all_permutations():
    """the oracle's own optimal mode, wherever all permutations can be walked: n <= 7"""
    checked = 0
    for name in ALL:
        s = cases.get_scene(name)
        for ms, r in zip(s["missions"], cases.expected(name)):
            if r.matrix is None or r.n > 7:
                continue
            for asg in ([ms["assign"][:r.n]] if ms["assign"] is not None else []) + [list(range(r.n)), list(range(r.n))[::-1]]:
                assert cases.held_karp(r.matrix, r.n, list(asg)) == cases.brute_force(r.matrix, r.n, list(asg)), (name, asg)
                checked += 1
    assert checked > 100


def test_the_exact_order_of_sums():
    less = cases.less
    assert less((7, 0), (0, 5)) and not less((0, 5), (7, 0))             # 7 < 5 sqrt 2 = 7.07...
    assert less((0, 12), (17, 0)) and not less((17, 0), (0, 12))         # 12 sqrt 2 = 16.97... < 17
    assert less((0, 140), (99, 70)) and not less((99, 70), (0, 140))     # 70 sqrt 2 = 98.9949... < 99
    assert not less((3, 4), (3, 4)) and less((3, 4), cases.INF) and not less(cases.INF, (3, 4)) and not less(cases.INF, cases.INF)
    assert cases.add((1, 2), cases.INF) == cases.INF and cases.add((1, 2), (3, 4)) == (4, 6)


def test_the_scenes_hold_what_they_should():
    ex = cases.expected
    for n in cases.SIZES:
        P = 1 + 2 * n
        for kind in ("open", "wall_gap"):
            r = ex("%s:%d" % (kind, n))[0]
            assert r.status == 0 and r.fields == P - 1 and cases.INF not in r.matrix.values() and len(r.order) == 2 * n
        r = ex("clamp:%d" % n)[0]
        assert r.status == 0 and r.fields > P - 1 and cases.INF not in r.matrix.values()
        r = ex("box:%d" % n)[0]
        assert all((r.matrix[i, n + 1] == cases.INF) == (i != n + 1) and r.matrix[i, n + 1] == r.matrix[n + 1, i] for i in range(P))
        assert sum(d == cases.INF for d in r.matrix.values()) == 2 * (P - 1)
        r = ex("same_cell:%d" % n)[0]
        assert r.matrix[1, n + 1] == (0, 0) and all(r.matrix[i, j] != (0, 0) for i in range(P) for j in range(P) if i != j and {i, j} != {1, n + 1})
    assert ex("open:3")[0].fields == 6
    o, w = ex("open:10")[0], ex("wall_gap:10")[0]
    assert any(cases.less(o.matrix[k], w.matrix[k]) for k in o.matrix)       # the wall makes some pairs longer
    r = ex("whole_map")[0]
    assert r.window == (0, 0, 47, 47) and 0 < sum(d == cases.INF for d in r.matrix.values()) < 72
    r, sc = ex("leg_window")[0], cases.scene("leg_window")
    alone = cases.ps.search(sc["map"], sc["missions"][0]["pts"][0], sc["missions"][0]["pts"][1], sc["safe_dis"], sc["margin"])
    assert alone.status == 0 and cases.less(r.matrix[0, 1], alone.cost)      # the pair's own window makes the leg strictly longer
    g, b = ex("differ:greedy")[0], ex("differ:optimal")[0]
    assert g.order != b.order and len(g.order) == len(b.order) == 4 and cases.less(b.total, g.total)
    assert b.total[1] > 0 and g.total[1] > 0                                    # diagonal steps: the comparison is not one of integers
    r = ex("mirror:optimal")[0]
    assert r.order == [0, 0, 1, 1, 2, 2] and r.matrix[4, 2] == r.matrix[4, 3] and r.matrix[2, 5] == r.matrix[3, 6]
    assert cases.brute_force(r.matrix, 3, [0, 1, 2])[1] == r.total
    swapped = {(i, j): r.matrix[{2: 3, 3: 2, 5: 6, 6: 5}.get(i, i), {2: 3, 3: 2, 5: 6, 6: 5}.get(j, j)] for i, j in r.matrix}
    assert swapped == r.matrix                                                   # the mirror image has the same matrix: a true tie
    assert ex("mirror:greedy")[0].order[:3] == [0, 0, 1]
    a = ex("assign")
    assert a[0].order[1::2] == [[1, 0][i] for i in a[0].order[0::2]] and a[1].order[1::2] == [[1, 2, 0][i] for i in a[1].order[0::2]]
    assert a[0].total != ex("differ:optimal")[0].total
    g, b = ex("unreachable:greedy")[0], ex("unreachable:optimal")[0]
    assert g.status == 0 and len(g.order) == 3 and b.status == cases.E_NO_ORDER and b.matrix == g.matrix
    assert [r.status for r in ex("bad")] == [cases.E_TASKS] * 4 + [cases.E_ENDPOINT] * 2 + [cases.E_TASKS, 0, 0]
    assert [r.status for r in ex("window")] == [cases.E_WINDOW, 0]


def test_the_random_missions_are_mostly_plain():
    for mode in (cases.GREEDY, cases.OPTIMAL):
        res = cases.expected(("random", mode))
        assert len(res) == cases.RANDOM_MISSIONS and all(r.status in (0, cases.E_NO_ORDER) for r in res)
        assert sum(cases.INF in r.matrix.values() for r in res) < len(res) / 4
        assert sum(r.fields > r.P - 1 for r in res) < len(res) / 4
        assert sum(cases.INF in r.matrix.values() for r in res) >= 2 and sum(r.fields > r.P - 1 for r in res) >= 4
        assert len({r.n for r in res}) >= 6 and max(r.n for r in res) == 10


# ---- the build side ---------------------------------------------------------------------------------------------------------
def test_task_calls_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alore_backend.h")).read(), flags=re.S)
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    from alore_legged_manipulator_amd import _lib, backend
    lib = _lib.load()
    backend._bind(lib)
    for name in TASK_CALLS:
        assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", hdr), name
        assert re.search(r"\sT\s+" + name + r"$", syms, re.M), name
        assert getattr(lib, name).argtypes is not None, name
    for method in ("task_plan", "task_plan_device", "task_result", "device_task"):
        assert hasattr(backend.BatchedMSPlanner, method), method
    for k, v in (("OK", 0), ("MASKED", 1), ("E_ENDPOINT", -1), ("E_WINDOW", -3), ("E_TASKS", -6), ("E_NO_ORDER", -7), ("GREEDY", 0),
                 ("OPTIMAL", 1), ("MAX_TASKS", 10)):
        assert re.search(r"#define\s+ALORE_BE_TASK_%s\s+\(?%d\)?" % (k, v), hdr), k
        assert getattr(backend, "TASK_" + k) == v == getattr(cases, k)


def test_struct_mirrors_have_the_c_layout(tmp_path):
    from alore_legged_manipulator_amd import backend
    code = ('#include <stdio.h>\n#include "alore_backend.h"\nint main(){printf("%zu %zu", sizeof(alore_backend_task_params), '
            'sizeof(alore_backend_task_view));}')
    (tmp_path / "s.c").write_text(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    sizes = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert sizes == [C.sizeof(backend.TaskParamsC), C.sizeof(backend.TaskViewC)]


def test_default_task_params_need_no_gpu():
    from alore_legged_manipulator_amd import backend
    p = backend.default_task_params()
    assert (p.safe_dis, p.window_margin, p.mode) == (0.3, 3.0, backend.TASK_GREEDY)


def test_the_kernels_are_in_the_gfx950_code_object():
    blob = open(LIB, "rb").read()
    assert b"task_costs_kernel" in blob and b"task_order_kernel" in blob and b"gfx950" in blob
