"""The modes of csrc/task_plan.h that choose the item-to-target assignment (ASSIGNED, JOINT) on the CPU against their oracle,
tests/task_assign_cases.py, and the build side of the feature: the new calls are declared, exported and bound, the constants agree,
the struct layouts hold, the new kernels are in the gfx950 code object.

tests/harness/task_assign_check.cpp includes the header, is compiled with g++ (once more as a stand-alone program with the address
and undefined-behaviour sanitizers) and runs the scenes through tplan::plan_one_assigned.  Every row of the result is pre-filled
and compared with the oracle's for EQUALITY, what must stay untouched included."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import task_assign_cases as cases
from tests import task_plan_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "harness", "task_assign_check.cpp")
LIB = os.path.join(ROOT, "alore_legged_manipulator_amd", "libalore_nmpc.so")
FLAGS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
ASSIGN_CALLS = ("alore_backend_device_task_assign", "alore_backend_get_task_assign", "alore_backend_task_reorder")
RANDOM = [("random", cases.ASSIGNED), ("random", cases.JOINT)]
ALL = list(cases.SCENES) + RANDOM
KEYS = ("matrix", "order", "total", "leg_start_xy", "leg_goal_xy", "assignment", "assign_total")


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("task_assign_check")
    out = {}
    for name, flags in FLAGS.items():
        out[name] = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC, SRC, "-o", out[name]])
    return out


def ints(line):
    return np.array([int(v) for v in line.split()], np.int32)


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
        status, n_order, ta, tb, fields, sweeps = (int(v) for v in lines[7 * k].split())
        dbl = lambda line: np.array([float(v) for v in line.split()]).reshape(cases.MAX_LEGS, 2)
        out.append({"status": status, "n_order": n_order, "total": np.array([ta, tb], np.int32), "fields": fields, "sweeps": sweeps,
                    "matrix": ints(lines[7 * k + 1]).reshape(cases.P_MAX, cases.P_MAX, 2), "order": ints(lines[7 * k + 2]),
                    "leg_start_xy": dbl(lines[7 * k + 3]), "leg_goal_xy": dbl(lines[7 * k + 4]), "assignment": ints(lines[7 * k + 5]),
                    "assign_total": ints(lines[7 * k + 6])})
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


def _matrices():
    """every matrix the oracle has computed for the scenes of both features"""
    for name in list(tc.SCENES) + [("random", tc.GREEDY)]:
        for r in tc.expected(name):
            if r.matrix is not None:
                yield name, r
    for name in ALL:
        for r in cases.expected(name):
            if r.matrix is not None:
                yield name, r


def test_the_matching_equals_all_bijections():
    """the oracle's own matching, wherever all bijections can be walked: n <= 7"""
    checked = 0
    for name, r in _matrices():
        if r.n <= 7:
            assert cases.matching(r.matrix, r.n) == cases.matching_brute_force(r.matrix, r.n), name
            checked += 1
    assert checked > 50


def test_the_joint_programme_equals_all_routes():
    """the oracle's own joint programme, wherever all (order, bijection) pairs can be walked: n <= 4, 576 routes"""
    checked = 0
    for name, r in _matrices():
        if r.n <= 4:
            assert cases.joint(r.matrix, r.n) == cases.joint_brute_force(r.matrix, r.n), name
            checked += 1
    assert checked > 50


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_the_tie_rules_on_small_integer_matrices(exes, build, tmp_path):
    """matrices drawn from {1, 2, INF}: nearly every optimum is tied many times over, so the answer is the tie rule's.  Header,
    oracle and brute force agree; a hand-written matrix has a finite matching and no route (the rule of the assigned mode: both
    rows written, E_NO_ORDER)"""
    rng = np.random.default_rng(7)
    for mode, sizes in ((cases.ASSIGNED, (1, 2, 3, 5, 6)), (cases.JOINT, (1, 2, 3, 4))):
        mats = []
        for k in range(60):
            n = sizes[k % len(sizes)]
            P = 1 + 2 * n
            draw = rng.integers(0, 8, (P, P))
            mats.append((n, {(i, j): (0, 0) if i == j else cases.INF if draw[i, j] < 3 else (int(1 + draw[i, j] % 2), 0) for i in range(P) for j in range(P)}))
        if mode == cases.ASSIGNED:      # carry legs finite, nothing leaves the robot
            mats.append((2, {(i, j): (0, 0) if i == j else cases.INF if 0 in (i, j) else (1, 1) for i in range(5) for j in range(5)}))
        path = tmp_path / ("matrices_%d.txt" % mode)
        path.write_text("%d %d\n" % (mode, len(mats)) + "".join(
            "%d %s\n" % (n, " ".join("%d %d" % mat[i, j] for i in range(1 + 2 * n) for j in range(1 + 2 * n))) for n, mat in mats))
        r = subprocess.run([exes[build], "matrix", str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = r.stdout.split("\n")
        finite = 0
        for k, (n, mat) in enumerate(mats):
            (status, n_order, ta, tb), order, rows = ints(lines[3 * k]), ints(lines[3 * k + 1]), ints(lines[3 * k + 2])
            if mode == cases.ASSIGNED:
                asg, carry = cases.matching(mat, n)
                assert (asg, carry) == cases.matching_brute_force(mat, n)
                seq, total = tc.held_karp(mat, n, asg) if asg is not None else (None, cases.INF)
                want_order = None if seq is None else [v for i in seq for v in (i, asg[i])]
            else:
                want_order, total = cases.joint(mat, n)
                assert (want_order, total) == cases.joint_brute_force(mat, n)
                asg = None if want_order is None else [want_order[2 * want_order[0::2].index(i) + 1] for i in range(n)]
                carry = None if asg is None else cases.carry_sum(mat, n, asg)
            e_asg, e_order = np.full(cases.MAX_TASKS + 2, cases.FILL_I), np.full(cases.MAX_LEGS, cases.FILL_I)
            if asg is not None:
                e_asg[:n], e_asg[cases.MAX_TASKS:] = asg, carry
            if want_order is not None:
                e_order[:2 * n] = want_order
                finite += 1
                assert (status, n_order, ta, tb) == (0, 2 * n) + total, (mode, k)
            else:
                assert (status, n_order, ta, tb) == (cases.E_NO_ORDER, 0, cases.FILL_I, cases.FILL_I), (mode, k)
            assert np.array_equal(rows, e_asg) and np.array_equal(order, e_order), (mode, k, rows, e_asg, order, e_order)
        assert finite >= 15 and len(mats) - finite >= 5, finite
        if mode == cases.ASSIGNED:
            assert status == cases.E_NO_ORDER and rows[:2].tolist() == [0, 1] and rows[cases.MAX_TASKS:].tolist() == [2, 2]


def _identity_carry(r):
    return cases.carry_sum(r.matrix, r.n, list(range(r.n)))


def test_the_inequalities_between_the_modes():
    """on every mission of the random scenes that is OK: the matching is not above the identity's carry sum; JOINT <= ASSIGNED <=
    OPTIMAL of the same assignment (equal: it is that routing); JOINT is not above greedy where greedy completes"""
    less = cases.less
    for name in RANDOM:
        s, n_ok = cases.get_scene(name), 0
        for ms, r in zip(s["missions"], cases.expected(name)):
            if r.status != cases.OK:
                continue
            n_ok += 1
            a = r if s["mode"] == cases.ASSIGNED else cases.plan(s["map"], ms["n"], s["max_tasks"], ms["pts"], cases.ASSIGNED, s["safe_dis"], s["margin"])
            if a.assignment is not None:
                assert not less(_identity_carry(a), a.assign_total)
            if ms["n"] <= cases.JOINT_MAX_TASKS:
                j = r if s["mode"] == cases.JOINT else cases.plan(s["map"], ms["n"], s["max_tasks"], ms["pts"], cases.JOINT, s["safe_dis"], s["margin"])
                assert j.status == cases.OK                                  # ASSIGNED found a route, so there is one
                if a.status == cases.OK:
                    assert not less(a.total, j.total)
                g_order, g_total = tc.greedy(r.matrix, r.n)
                if len(g_order) == 2 * r.n:
                    assert not less(g_total, j.total)
                assert not less(j.assign_total, a.assign_total) if a.assignment is not None else True
            if a.status == cases.OK:
                seq, total = tc.held_karp(a.matrix, a.n, a.assignment)
                assert not less(total, a.total) and total == a.total
        assert n_ok >= 48


def test_the_random_missions_are_mostly_plain_and_some_fail():
    for name in RANDOM:
        res = cases.expected(name)
        assert len(res) == 64 and all(r.status in (cases.OK, cases.E_NO_ORDER) for r in res)
        assert sum(r.status == cases.OK for r in res) >= 48 and sum(r.status == cases.E_NO_ORDER for r in res) >= 1
    assert max(r.n for r in cases.expected(RANDOM[0])) == 10 and {r.n for r in cases.expected(RANDOM[1])} == {1, 2, 3, 4, 5}
    # two of the missions with up to ten tasks have a finite matching and no route for it: both rows written, E_NO_ORDER
    assert sum(r.status == cases.E_NO_ORDER and r.assignment is not None for r in cases.expected(RANDOM[0])) >= 1


def test_the_scenes_hold_what_they_should():
    ex, less = cases.expected, cases.less
    a, j = ex("crossed:assigned")[0], ex("crossed:joint")[0]
    ident = tc.plan(cases.scene("crossed:assigned")["map"], 2, 2, cases.scene("crossed:assigned")["missions"][0]["pts"], None, tc.OPTIMAL)
    assert a.assignment == [1, 0] and a.status == ident.status == 0 and less(a.total, ident.total) and less(a.assign_total, _identity_carry(a))
    assert not less(a.total, j.total)
    # the geometry of task_plan_cases "differ" as it stands has the identity as its matching: the targets are exchanged here
    d = tc.expected("differ:optimal")[0]
    assert cases.matching(d.matrix, 2)[0] == [0, 1] and cases.matching(a.matrix, 2)[1] == cases.matching(d.matrix, 2)[1]
    a = ex("mirror:assigned")[0]
    assert a.assignment == [0, 1, 2] and a.order == [0, 0, 1, 1, 2, 2] and a.total == tc.expected("mirror:optimal")[0].total
    assert ex("mirror:joint")[0].order == [0, 0, 1, 1, 2, 2]
    a, j = ex("tie:assigned")[0], ex("tie:joint")[0]
    optima = [list(p) for p in cases.itertools.permutations(range(3)) if cases.carry_sum(a.matrix, 3, p) == a.assign_total]
    assert optima == [[1, 0, 2], [1, 2, 0]] and a.assignment == [1, 0, 2]    # a true tie of matchings: the smaller vector
    assert a.assign_total[1] > 0 and j.total == a.total and j.order < a.order and j.assignment == [1, 2, 0]   # and a tie of routes
    a, j = ex("joint_beats_assigned:assigned")[0], ex("joint_beats_assigned:joint")[0]
    assert a.status == j.status == 0 and less(j.total, a.total) and less(a.assign_total, j.assign_total)
    assert cases.search_joint_beats_assigned() == cases.JOINT_BEATS_ASSIGNED
    for mode in ("assigned", "joint"):
        r = ex("box:" + mode)[0]
        assert r.status == cases.E_NO_ORDER and r.assignment is None and r.matrix == tc.expected("box:3")[0].matrix
    a, j = ex("unroutable:assigned")[0], ex("unroutable:joint")[0]
    assert a.status == j.status == cases.E_NO_ORDER and a.assignment == [0, 1] and a.assign_total != cases.INF and j.assignment is None
    assert all(a.matrix[0, k] == cases.INF for k in range(1, 5)) and all(a.matrix[1 + i, 3 + t] != cases.INF for i in range(2) for t in range(2))
    assert [r.status for r in ex("too_many:joint")] == [cases.E_TASKS, cases.E_TASKS, 0]
    assert [r.status for r in ex("too_many:assigned")] == [0, cases.E_ENDPOINT, 0]
    for mode in ("assigned", "joint"):
        s = cases.scene("ignored_assignment:" + mode)
        r = ex("ignored_assignment:" + mode)
        assert [ms["assign"] for ms in s["missions"]] == [[0, 0], [7, -1]] and cases.arrays(s)[2] is not None
        assert r[0].status == r[1].status == 0 and r[0].order == r[1].order and r[0].assignment == r[1].assignment
        opt = [tc.plan(s["map"], 2, 2, ms["pts"], ms["assign"], tc.OPTIMAL).status for ms in s["missions"]]
        assert opt == [cases.E_TASKS, cases.E_TASKS]


# ---- the build side ---------------------------------------------------------------------------------------------------------
def test_assign_calls_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alore_backend.h")).read(), flags=re.S)
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    from alore_legged_manipulator_amd import _lib, backend
    lib = _lib.load()
    backend._bind(lib)
    for name in ASSIGN_CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert re.search(r"\sT\s+" + name + r"$", syms, re.M), name
        assert getattr(lib, name).argtypes is not None, name
    for method in ("device_task_assign", "task_assignment", "task_reorder"):
        assert hasattr(backend.BatchedMSPlanner, method), method
    src = open(os.path.join(CSRC, "task_plan.h")).read()
    for k, v in (("ASSIGNED", 2), ("JOINT", 3), ("JOINT_MAX_TASKS", 5)):
        assert re.search(r"#define\s+ALORE_BE_TASK_%s\s+\(?%d\)?" % (k, v), hdr), k
        assert getattr(backend, "TASK_" + k) == v == getattr(cases, k)
        assert re.search(r"\b%s = %d\b" % (k, v), src), k


def test_struct_mirrors_have_the_c_layout(tmp_path):
    from alore_legged_manipulator_amd import backend
    code = ('#include <stdio.h>\n#include "alore_backend.h"\nint main(){printf("%zu %zu %zu", sizeof(alore_backend_task_params), '
            'sizeof(alore_backend_task_view), sizeof(alore_backend_task_assign_view));}')
    (tmp_path / "s.c").write_text(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    sizes = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert sizes == [C.sizeof(backend.TaskParamsC), C.sizeof(backend.TaskViewC), C.sizeof(backend.TaskAssignViewC)]
    assert sizes[0] == 24 and sizes[1] == 8 + 9 * C.sizeof(C.c_void_p) and sizes[2] == 2 * C.sizeof(C.c_void_p)   # the old two as they were


def test_the_kernels_are_in_the_gfx950_code_object():
    blob = open(LIB, "rb").read()
    assert b"task_assign_order_kernel" in blob and b"task_joint_kernel" in blob and b"gfx950" in blob
