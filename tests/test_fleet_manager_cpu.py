"""csrc/fleet_manager.h (plan_manager's state machine for one robot of a fleet) on the CPU against its oracle,
tests/fleet_manager_cases.py, and the build side of the feature: fleet_manager.hip compiles for gfx950, the alore_backend_manager_*
calls are declared, exported and bound.

tests/harness/fleet_manager_check.cpp includes the header, is compiled with g++ -ffp-contract=off (once more with the address and
undefined-behaviour sanitizers, as a stand-alone program) and runs the scenarios robot by robot.  Compared BIT FOR BIT after every
tick on every seed: the state words, the masks, every time and pose, the counters."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import fleet_manager_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "harness", "fleet_manager_check.cpp")
LIB = os.path.join(ROOT, "alore_legged_manipulator_amd", "libalore_nmpc.so")
FLAGS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
CALLS = ("alore_backend_manager_default_params", "alore_backend_manager_create", "alore_backend_manager_request", "alore_backend_manager_begin",
         "alore_backend_manager_starts", "alore_backend_manager_end", "alore_backend_manager_next_legs", "alore_backend_device_manager",
         "alore_backend_get_manager")


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("fleet_manager_check")
    out = {}
    for name, flags in FLAGS.items():
        out[name] = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC, SRC, "-o", out[name]])
    return out


def num(v):
    return repr(float(v))


def scenario_text(sc):
    B, p, d = sc["B"], sc["params"], sc["dist"]
    text = ["%d %d" % (B, cases.P), "%s %s %d %d %d" % (num(p["replan_time"]), num(p["max_replan_time"]), p["replan_on_collision_only"],
                                                         p["stop_inside_obstacle"], p["stop_on_no_path"]),
            "%d %d %s %s %s" % (cases.NX, cases.NY, num(cases.X_LO), num(cases.Y_LO), num(cases.RES)), " ".join(num(v) for v in d.reshape(-1))]
    zero = np.zeros((B, 3))
    for step in cases.steps_of(sc):
        if step[0] == "Q":
            _, starts, goals, mask = step
            text.append("Q %d %d" % (starts is not None, goals is not None))
            s, g = (zero if starts is None else starts), (zero if goals is None else goals)
            text += ["%d %s %s" % (mask[b], " ".join(num(v) for v in s[b][:3]), " ".join(num(v) for v in g[b][:3])) for b in range(B)]
        elif step[0] == "T":
            t = step[1]
            text.append("T %s" % num(t["now"]))
            text += ["%s %s %d %s %d %d %d %d %s" % (num(t["poses"][b, 0]), num(t["poses"][b, 1]), t["collision"][b], " ".join(num(v) for v in t["xytheta"][b]),
                                                    t["search"][b], t["build"][b], t["ok"][b], t["n_pieces"][b], " ".join(num(v) for v in t["T"][b]))
                     for b in range(B)]
        else:
            _, reset, poses = step
            task = sc["task"]
            text.append("L %d" % reset)
            text += ["%s %d %d %s %s" % (" ".join(num(v) for v in poses[b]), task["status"][b], task["n_order"][b],
                                         " ".join(num(v) for v in task["leg_goal_xy"][b].reshape(-1)), " ".join(num(v) for v in task["leg_yaw"][b]))
                     for b in range(B)]
    return "\n".join(text) + "\n"


def run(exe, sc, tmp_path):
    """the harness' output as the oracle's snapshots: a list of (ints [11][B], doubles [14][B], counters [8])"""
    infile = tmp_path / "scenario.txt"
    infile.write_text(scenario_text(sc))
    r = subprocess.run([exe, str(infile)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-4000:])
    lines, B, out = r.stdout.strip().split("\n"), sc["B"], []
    assert len(lines) % (B + 1) == 0
    for at in range(0, len(lines), B + 1):
        rows = [ln.split() for ln in lines[at:at + B]]
        ints = np.array([[int(v) for v in row[:11]] for row in rows], np.int32).T
        dbl = np.array([[float(v) for v in row[11:]] for row in rows], np.float64).T
        assert lines[at + B].startswith("C ")
        out.append((ints, dbl, np.array(lines[at + B].split()[1:], np.int32)))
    return out


same = cases.same


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
@pytest.mark.parametrize("seed", cases.SEEDS)
def test_the_header_equals_the_oracle(exes, build, seed, tmp_path):
    sc = cases.scenario(seed)
    got, (_, exp, _) = run(exes[build], sc, tmp_path), cases.run_oracle(sc)
    assert len(got) == len(exp) == sc["K"] == 12 and sc["B"] == 70
    for k, (g, e) in enumerate(zip(got, exp)):
        same(g, e, (seed, "tick", k))


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_next_legs_equal_the_oracle(exes, build, tmp_path):
    sc = cases.legs_scenario()
    got, (fleet, exp, _) = run(exes[build], sc, tmp_path), cases.run_oracle(sc)
    assert len(got) == len(exp)
    for k, (g, e) in enumerate(zip(got, exp)):
        same(g, e, ("legs", k))
    legs = exp[-2][0][3]
    assert legs.tolist() == [2, 6, 4, 0, 6, 0]                       # every mission through its legs; the failed one and the busy robot took none
    assert exp[-1][0][3].tolist() == [1, 1, 1, 0, 1, 0]              # reset_legs: the free robots start again


def test_the_seeds_reach_every_branch():
    """the committed seeds, between them, contain every case of the list; each seed alone is printed for whoever changes one"""
    events, per_seed = set(), {}
    for seed in cases.SEEDS:
        fleet, snaps, _ = cases.run_oracle(cases.scenario(seed))
        per_seed[seed] = fleet.events
        events |= fleet.events
        c = dict(zip(cases.COUNTERS, snaps[-1][2]))
        assert c["fresh"] > 0 and c["delivered"] > 0 and c["arrived"] > 0 and c["stopped"] > 0
    missing = [e for e in cases.COVERAGE if e not in events]
    assert not missing, (missing, per_seed)
    # two ticks differ from one: the tick that goes to GOINGTOGOAL does not run the finish rule, the next one does
    fleet = cases.Fleet(1, cases.SEED_PARAMS[1])
    fleet.request(np.zeros((1, 3)), np.full((1, 3), 9.0))
    tick = dict(search=[0], build=[0], ok=[0], T=[[1.0]], n_pieces=[1])
    states = []
    for k in range(3):
        fleet.begin(cases.tick_time(k), np.zeros((1, 3)))
        fleet.end(**tick)
        states.append(fleet.robots[0].state)
    assert states == [cases.PLANNING, cases.GOINGTOGOAL, cases.IDLE] and fleet.counters["arrived"] == 1


def test_the_oracle_pins_the_order_of_operations():
    """(dx dx + dy dy) + fmod(|dyaw|, 2 pi) 0.02 < 1.0, the first term from the POSE, the yaw from plan_start_xytheta; strict
    comparisons with replan_time; >= in the finish rule"""
    p = dict(replan_time=1.0, max_replan_time=0.5)
    def robot(pose, start_yaw, goal=(0.0, 0.0, 0.0), total=100.0):
        f = cases.Fleet(1, p)
        f.request(np.array([[5.0, 5.0, start_yaw]]), np.array([goal]))
        f.begin(100.0, [pose])
        f.end([0], [0], [1], [[total]], [1])
        f.begin(101.0, [pose])
        assert f.robots[0].action == cases.NONE and f.robots[0].state == cases.PLANNING      # exactly replan_time: no cycle
        f.end([0], [0], [1], [[total]], [1])
        f.begin(101.25, [pose])
        return f.robots[0]
    assert robot((0.6, 0.6, 0.0), 0.0).state == cases.GOINGTOGOAL                  # 0.72 < 1: the pose decides, the start is far away
    assert robot((0.8, 0.6, 0.0), 0.0).state == cases.REPLAN                       # 0.64 + 0.36 = 1.0 is not < 1.0
    assert robot((0.9, 0.4, 0.0), 3.0).state == cases.REPLAN                       # 0.97 + 0.06
    assert robot((0.9, 0.4, 0.0), 2.0 * np.pi + 0.5).state == cases.GOINGTOGOAL    # the fmod: 0.97 + 0.01
    r = robot((9.0, 9.0, 0.0), 0.0)
    assert r.state == cases.REPLAN and r.time == 101.25 + 0.5 - 100.0
    assert robot((9.0, 9.0, 0.0), 0.0, total=0.25).state == cases.IDLE             # arrived at 100.25 already: nothing starts


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
    for method in ("manager_create", "manager_request", "manager_begin", "manager_starts", "manager_end", "manager_next_legs", "manager_view",
                   "get_manager"):
        assert hasattr(backend.BatchedMSPlanner, method), method


def test_struct_mirrors_have_the_c_layout(tmp_path):
    from alore_legged_manipulator_amd import backend
    code = ('#include <stdio.h>\n#include "alore_backend.h"\nint main(){printf("%zu %zu", sizeof(alore_backend_manager_params), '
            'sizeof(alore_backend_manager_view));}')
    (tmp_path / "s.c").write_text(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    sizes = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert sizes == [C.sizeof(backend.ManagerParamsC), C.sizeof(backend.ManagerViewC)]


def test_default_manager_params_need_no_gpu():
    from alore_legged_manipulator_amd import backend
    p = backend.default_manager_params()
    assert {k: getattr(p, k) for k, _ in backend.ManagerParamsC._fields_ if k != "reserved"} == cases.DEFAULT_PARAMS


def test_the_kernels_are_in_the_gfx950_code_object():
    """fleet_manager.hip is compiled for gfx950 and linked: its kernels are in the library's device code"""
    blob = open(LIB, "rb").read()
    for kernel in (b"manager_request_kernel", b"manager_begin_kernel", b"manager_starts_kernel", b"manager_end_kernel", b"manager_next_legs_kernel"):
        assert kernel in blob, kernel
    assert b"gfx950" in blob
