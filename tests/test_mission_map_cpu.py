"""csrc/mission_map.h (the edits a mission makes to the occupancy map) on the CPU against its oracle, tests/mission_cases.py, and the
build side of the feature: mission_map.hip compiles for gfx950, the alore_backend_map_paint and alore_backend_mission_* calls are
declared, exported and bound.

tests/harness/mission_map_check.cpp includes the header, is compiled with g++ -ffp-contract=off (once more with the address and
undefined-behaviour sanitizers, as a stand-alone program) and drives the header's functions sequentially through the calls of
mission_cases.py.  Compared for EQUALITY after every call: the state grid, the edit list as bytes, status, phase and goal indices,
n_changed, the box and n_skipped.  Every operation that decides a cell or a rule is a correctly rounded double operation, one
narrowing to float or an integer operation, on both sides."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import mission_cases as cases
from tests import occupancy_cases as occ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "harness", "mission_map_check.cpp")
LIB = os.path.join(ROOT, "alore_legged_manipulator_amd", "libalore_nmpc.so")
FLAGS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
CALLS = ("alore_backend_map_paint", "alore_backend_device_paint_counters", "alore_backend_map_paint_counters",
         "alore_backend_mission_default_params", "alore_backend_mission_create", "alore_backend_mission_set", "alore_backend_mission_set_goals",
         "alore_backend_mission_step", "alore_backend_device_mission", "alore_backend_get_mission")


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("mission_map_check")
    out = {}
    for name, flags in FLAGS.items():
        out[name] = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC, SRC, "-o", out[name]])
    return out


def hx(v):
    return float(v).hex()


def header(slots):
    return "%d %d %s %s %s %d  %s\n" % (occ.NX, occ.NY, hx(occ.X_LO), hx(occ.Y_LO), hx(occ.RES), slots, " ".join(hx(v) for v in cases.PARAMS.values()))


def edits_text(call, edits):
    return "%s %d\n" % (call, len(edits)) + "".join("%s %s %s %s %d\n" % (hx(e[0]), hx(e[1]), hx(e[2]), hx(e[3]), int(e[4])) for e in edits)


def run(exe, text, tmp_path, slots):
    """the harness' output: a list of {"invalid": k} and of states as mission_cases.Missions.snapshot() gives them"""
    infile = tmp_path / "calls.txt"
    infile.write_text(text)
    r = subprocess.run([exe, str(infile)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-4000:])
    lines, at, out = r.stdout.split("\n"), 0, []
    while at < len(lines) and lines[at]:
        if lines[at].startswith("invalid"):
            out.append({"invalid": int(lines[at].split()[1])})
            at += 1
            continue
        c = [int(v) for v in lines[at].split()[1:]]
        n = int(lines[at + 1].split()[1])
        edits = [lines[at + 2 + k].split() for k in range(n)]
        at += 2 + n
        ints = [np.array(lines[at + a].split(), np.int32) for a in range(5)]
        grid = np.array([lines[at + 5 + x].split() for x in range(occ.NX)], np.uint8)
        at += 5 + occ.NX
        assert grid.shape == (occ.NX, occ.NY) and all(len(a) == slots for a in ints)
        out.append(dict(zip(("status", "phase", "goal_item", "goal_target", "goal_status"), ints), n_changed=c[0], box=tuple(c[1:5]), n_skipped=c[5],
                        edits=cases.as_array([[float.fromhex(v) for v in e[:4]] + [int(e[4])] for e in edits]), grid=grid))
    return out


def same(got, exp, what):
    for key in ("status", "phase", "goal_item", "goal_target", "goal_status", "grid"):
        assert np.array_equal(got[key], exp[key]), (what, key, np.argwhere(got[key] != exp[key])[:8])
    assert got["edits"].tobytes() == exp["edits"].tobytes(), (what, "edits", len(got["edits"]), len(exp["edits"]))
    assert (got["n_changed"], tuple(got["box"]), got["n_skipped"]) == (exp["n_changed"], tuple(exp["box"]), exp["n_skipped"]), what


def mission_text():
    text = header(cases.SLOTS)
    for name, args, _ in cases.mission_expected():
        if name == "set":
            n, pts, kinds, mask = args
            text += "S %d %d\n" % (len(n), cases.T)
            for b in range(len(n)):
                text += "%d %d %s %s\n" % (mask[b], n[b], " ".join(hx(v) for v in pts[b].reshape(-1)), " ".join(str(int(k)) for k in kinds[b]))
        elif name == "goals":
            goals, mask = args
            text += "G %d\n" % len(goals) + "".join("%d %s %s\n" % (mask[b], hx(goals[b, 0]), hx(goals[b, 1])) for b in range(len(goals)))
        else:
            poses, after = args
            text += "T %d\n" % len(poses) + "".join("%s %s %d\n" % (hx(poses[b, 0]), hx(poses[b, 1]), 0 if after is None else after[b])
                                                    for b in range(len(poses)))
    return text


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_paint_lists_equal_the_oracle(exes, build, tmp_path):
    text = header(1) + "".join(edits_text("P", e) for e in cases.paint_calls())
    got = run(exes[build], text, tmp_path, 1)
    exp = cases.paint_expected()
    assert len(got) == len(exp) == 4
    for k, (g, (grid, n, box, skipped)) in enumerate(zip(got, exp)):
        assert np.array_equal(g["grid"], grid), (k, np.argwhere(g["grid"] != grid)[:8])
        assert (g["n_changed"], g["box"], g["n_skipped"]) == (n, box, skipped), k


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_missions_equal_the_oracle(exes, build, tmp_path):
    got = run(exes[build], mission_text(), tmp_path, cases.SLOTS)
    exp = cases.mission_expected()
    assert len(got) == len(exp) == 5
    for k, (g, (name, _, snap)) in enumerate(zip(got, exp)):
        same(g, snap, (k, name))


def test_the_pinned_edits_hit_the_listed_cells(exes, tmp_path):
    """(0.82, 0.5) -> x cells 35 .. 44 and (-2.75, 0.25) -> 2, 4, 6, in the header and in the oracle; the oracle with a multiplied
    lattice, and without the narrowing to float, gives a different grid on them: the scenarios tell the implementations apart"""
    want = {cases.PIN_ACCUMULATED: list(range(35, 45)), cases.PIN_NARROWED: [2, 4, 6]}
    for pin, cells in want.items():
        got = run(exes["plain"], header(1) + edits_text("P", [pin]), tmp_path, 1)[0]
        assert sorted(set(np.argwhere(got["grid"] == 2)[:, 0].tolist())) == cells
        assert (got["grid"] == 2).sum() == len(cells) and got["n_changed"] == len(cells) and got["box"] == (cells[0], 24, cells[-1], 24)
        m = cases.new_map()
        cases.paint_list(m, [pin])
        assert np.array_equal(m.grid, got["grid"])
    def grid(pin, **how):
        m = cases.new_map()
        cases.paint_list(m, [pin], **how)
        return m.grid
    assert np.argwhere(grid(cases.PIN_ACCUMULATED, accumulated=False) == 2)[:, 0].tolist() == list(range(35, 46))
    assert np.argwhere(grid(cases.PIN_NARROWED, narrow=False) == 2)[:, 0].tolist() == [2, 3, 4, 5, 6]
    exp = cases.paint_expected()[0][0]
    both = [cases.PIN_ACCUMULATED, cases.PIN_NARROWED]
    for how in (dict(accumulated=False), dict(narrow=False)):
        m = cases.new_map()
        cases.paint_list(m, both, **how)
        assert not np.array_equal(m.grid, exp), how


def test_the_scenarios_cover_what_they_should():
    import itertools
    grids = set()
    # lock / free / lock: two locks next to each other commute, so the six orders are four classes (free first, free last, free
    # between the locks either way round), and every class gives another grid
    for order in itertools.permutations(cases.CHAIN):
        m = cases.new_map()
        cases.paint_list(m, order)
        grids.add(m.grid.tobytes())
    assert len(grids) == 4
    for k, e in enumerate(cases.border_edits()[:6]):       # four borders and the corner are clipped, the sixth edit is outside
        m = cases.new_map()
        n, box, _ = cases.paint_list(m, [e])
        full = (int(2 * e[2] / occ.RES) + 1) * (int(2 * e[3] / occ.RES) + 1)
        assert (0 < n < full) if k < 5 else n == 0, (k, n, full)
    m = cases.new_map()
    assert cases.paint_list(m, [cases.border_edits()[6]])[0] == 1                  # a zero half: one point
    assert len(cases.seeded_edits()) == 300
    calls = cases.mission_expected()
    st = calls[0][2]["status"]
    assert {cases.OK, cases.MASKED, cases.E_POINT, cases.E_TASKS} == set(st.tolist()) and (st[[3, 4, 8]] == cases.E_TASKS).all() and \
        (st[[5, 6]] == cases.E_POINT).all() and st[10] == cases.OK
    g = calls[1][2]
    ok = [b for b in range(20, 40) if st[b] == cases.OK and calls[1][1][1][b]]
    assert all(g["goal_item"][b] == 2 and g["phase"][b] == cases.PHASE_ITEM for b in ok if b < 30) and any(b < 30 for b in ok)
    assert all(g["goal_item"][b] == 1 and g["goal_target"][b] == 3 and g["phase"][b] == cases.PHASE_TARGET for b in ok if b >= 30)
    assert (g["goal_status"] == cases.GOAL_E_POINT).any() and {0, 1, 2} == set(g["phase"].tolist())
    for k in (2, 3, 4):
        e = calls[k][2]["edits"]
        assert len(e) > 40 and (e["make_obs"] == 0).any() and (e["make_obs"] == 1).any() and calls[k][2]["n_changed"] > 0
    halves = set(calls[4][2]["edits"]["hx"].tolist())
    assert halves == {0.5, 0.3, 0.2}                                               # all three rules fire in the last tick
    # exactly at the threshold: no edit; just inside: an edit (tick 0, by slot % 6)
    o = cases.Missions(cases.new_map(), 1)
    row = np.zeros((1, 21, 2))
    row[0, 1], row[0, 2] = (0.5, 0.25), (-1.0, 0.25)
    o.set([1], row)
    o.set_goals([(0.5, 0.25)])
    assert o.phase[0] == cases.PHASE_ITEM
    o.step([(2.5, 0.25)])
    assert len(o.edits) == 0
    o.step([(2.5 - cases.EPS, 0.25)])
    assert len(o.edits) == 1 and o.edits[0][4] == 0


def test_host_validation(exes, tmp_path):
    """NaN or infinite fields, negative halves and too many lattice points are refused; a zero half (one point) is accepted"""
    nan, inf = float("nan"), float("inf")
    good = [(0.0, 0.0, 0.0, 0.0, 1), (0.0, 0.0, 3.1, 0.5, 0), (1e6, -1e6, 0.5, 0.5, 1)]
    bad = [(nan, 0, 0.5, 0.5, 1), (0, inf, 0.5, 0.5, 1), (0, 0, nan, 0.5, 1), (0, 0, 0.5, -inf, 1), (0, 0, -0.1, 0.5, 1), (0, 0, 0.5, -1e-300, 1),
           (0, 0, 3.2, 0.5, 1), (0, 0, 0.5, 1e300, 1)]
    text = header(1) + edits_text("V", good) + "".join(edits_text("V", good + [b] + good) for b in bad)
    got = run(exes["plain"], text, tmp_path, 1)
    assert [g["invalid"] for g in got] == [-1] + [3] * len(bad)
    assert all(cases.edit_valid(e, occ.RES) for e in good) and not any(cases.edit_valid(e, occ.RES) for e in bad)
    assert int(2 * 3.1 / occ.RES) + 2 == 64 and int(2 * 3.2 / occ.RES) + 2 > 64


# ---- the build side ---------------------------------------------------------------------------------------------------------
def test_calls_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alore_backend.h")).read(), flags=re.S)
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    from alore_legged_manipulator_amd import _lib, backend
    lib = _lib.load()
    backend._bind(lib)
    for name in CALLS:
        assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", hdr), name
        assert re.search(r"\sT\s+" + name + r"$", syms, re.M), name
        assert getattr(lib, name).argtypes is not None, name
    for method in ("map_paint", "map_paint_device", "mission_create", "mission_set", "mission_set_goals", "mission_step", "mission_state"):
        assert hasattr(backend.BatchedMSPlanner, method), method


def test_struct_mirrors_have_the_c_layout(tmp_path):
    from alore_legged_manipulator_amd import backend
    code = ('#include <stdio.h>\n#include "alore_backend.h"\nint main(){printf("%zu %zu %zu", sizeof(alore_backend_map_edit), '
            'sizeof(alore_backend_mission_params), sizeof(alore_backend_mission_view));}')
    (tmp_path / "s.c").write_text(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    sizes = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert sizes == [C.sizeof(backend.MapEditC), C.sizeof(backend.MissionParamsC), C.sizeof(backend.MissionViewC)]
    assert sizes[0] == 40 == backend.EDIT_DTYPE.itemsize == cases.EDIT_DTYPE.itemsize


def test_default_mission_params_need_no_gpu():
    from alore_legged_manipulator_amd import backend
    p = backend.default_mission_params()
    assert {k: getattr(p, k) for k, _ in backend.MissionParamsC._fields_} == cases.PARAMS


def test_the_kernels_are_in_the_gfx950_code_object():
    """mission_map.hip is compiled for gfx950 and linked: its kernels are in the library's device code"""
    blob = open(LIB, "rb").read()
    for kernel in (b"mission_paint_begin_kernel", b"mission_paint_axes_kernel", b"mission_paint_cells_kernel", b"mission_set_kernel",
                   b"mission_goals_kernel", b"mission_edits_kernel"):
        assert kernel in blob, kernel
    assert b"gfx950" in blob
