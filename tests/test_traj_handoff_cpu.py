"""csrc/traj_handoff.h on the CPU: the promotion rule of a pending trajectory, the handle's list of outstanding start times and the
splitter that cuts a closed-loop run where a promotion has to go between two ticks, compiled with g++ alone (address and
undefined-behaviour sanitizers on) into a stand-alone program that is run as a child process (tests/harness/traj_handoff_check.cpp:
one request per line, one answer per line, doubles as hexadecimal floating point).  Every expected value is worked out here from the
rules: a pending entry is promoted when it is valid and now > start (strictly; mpc.cpp:177-182) or when a newer message forces it
(mpc.cpp:151-156); the tick that carries the promotion of a start time is the first whose time t0 + dt_tick * t exceeds it."""
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "harness", "traj_handoff_check.cpp")
HDR = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc", "traj_handoff.h")

T0, DT, N = 0.123, 0.01, 12


def tick(t, t0=T0, dt=DT):
    return t0 + dt * t


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("traj_handoff") / "traj_handoff_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    SRC, "-o", path], check=True, timeout=300)
    return path


def ask(exe, lines, path):
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rows = [ln.split() for ln in r.stdout.strip().split("\n")]
    assert len(rows) == len(lines)
    return rows


def test_header_is_plain_cpp():
    text = open(HDR).read()
    assert sorted(re.findall(r"#include\s+(\S+)", text)) == ["<cstddef>", "<vector>"]
    assert not re.search(r"getenv|\bhip[A-Z_]\w*|alore_nmpc_handle|alore_nmpc_solver", text)


def test_promotion_rule_is_strict(exe, tmp_path):
    start = 0.7
    cases = [((1, start, start, 0), 0),                              # now == start: the old trajectory is still tracked
             ((1, start, math.nextafter(start, math.inf), 0), 1),    # the next representable now: promoted
             ((1, start, math.nextafter(start, -math.inf), 0), 0),
             ((0, start, start + 1.0, 0), 0),                        # nothing pending
             ((1, start, start - 5.0, 1), 1),                        # forced by a newer message, whatever the start time
             ((0, start, start + 1.0, 1), 0),                        # ... but only a valid entry
             ((1, -0.0, 0.0, 0), 0), ((1, 1e300, math.inf, 0), 1), ((1, 0.0, math.nan, 0), 0)]
    rows = ask(exe, ["P %d %s %s %d" % (v, float(s).hex(), float(n).hex(), f) for (v, s, n, f), _ in cases], str(tmp_path / "p.txt"))
    assert [int(r[0]) for r in rows] == [want for _, want in cases]


def expected_segments(t0, dt, n, starts):
    cuts = set()
    for s in starts:
        first = next((t for t in range(n) if tick(t, t0, dt) > s), None)
        if first is not None:
            cuts.add(first)
    bounds = sorted(cuts | {0}) + [n]
    return [(a, b - a, 1 if a in cuts else 0) for a, b in zip(bounds[:-1], bounds[1:])] if n > 0 else []


SPLITS = {
    "none outstanding": [],
    "before t0: promoted in front of tick 0, no cut": [T0 - 1.0],
    "after the last tick: nothing": [tick(N - 1)],                     # equal to the last tick's time: not exceeded by any tick
    "two starts inside one tick: one cut": [tick(4) + 0.002, tick(4) + 0.007],
    "tick 1 and tick n - 1: parts shorter than three ticks": [tick(0), tick(N - 2)],
    "a start equal to a tick's time is exceeded by the next tick": [tick(5)],
    "every kind at once": [T0 - 1.0, tick(0), tick(5), tick(5) + 0.001, tick(N - 2) + 0.003, tick(N - 1) + 1.0],
}


def test_run_splitter(exe, tmp_path):
    names = list(SPLITS)
    lines = ["S %s %s %d %d %s" % (T0.hex(), DT.hex(), N, len(SPLITS[k]), " ".join(float(s).hex() for s in SPLITS[k])) for k in names]
    lines.append("S %s %s 0 1 %s" % (T0.hex(), DT.hex(), T0.hex()))     # an empty run has no segment
    rows = ask(exe, lines, str(tmp_path / "s.txt"))
    assert rows[-1] == ["0"]
    got = {}
    for name, row in zip(names, rows[:-1]):
        segs, at = [], 1
        for _ in range(int(row[0])):
            first, count, promote = (int(x) for x in row[at:at + 3])
            times = [float.fromhex(x) for x in row[at + 3:at + 3 + count]]
            at += 3 + count
            segs.append((first, count, promote))
            # the time of every tick of every segment is t0 + dt_tick * t with the GLOBAL t, bit for bit
            assert [x.hex() for x in times] == [tick(first + j).hex() for j in range(count)], name
        assert at == len(row), name
        assert segs == expected_segments(T0, DT, N, SPLITS[name]), name
        assert [t for f, c, _ in segs for t in range(f, f + c)] == list(range(N)), name
        got[name] = segs
    assert got["before t0: promoted in front of tick 0, no cut"] == [(0, N, 1)]
    assert got["after the last tick: nothing"] == [(0, N, 0)] and got["none outstanding"] == [(0, N, 0)]
    assert got["two starts inside one tick: one cut"] == [(0, 5, 0), (5, N - 5, 1)]
    assert got["tick 1 and tick n - 1: parts shorter than three ticks"] == [(0, 1, 0), (1, N - 2, 1), (N - 1, 1, 1)]
    assert got["a start equal to a tick's time is exceeded by the next tick"] == [(0, 6, 0), (6, N - 6, 1)]
    # this t0 and dt_tick do tell a shifted t0 from the global index: a segment issued as a public run from t0' = t0 + dt_tick * k
    # would have sampled at other times
    differ = [(k, j) for k, _, _ in got["every kind at once"] if k > 0 for j in range(N - k) if (T0 + DT * k) + DT * j != T0 + DT * (k + j)]
    assert differ, "choose a t0 / dt_tick for which the two ways of summing differ"


def test_outstanding_start_times(exe, tmp_path):
    starts = [1.0, 2.0, 2.0, 3.0]                                      # the same start time twice is kept once
    lines = ["T %s %d %s" % (float(now).hex(), len(starts), " ".join(s.hex() for s in starts)) for now in (0.5, 2.0, 4.0)]
    rows = ask(exe, lines, str(tmp_path / "t.txt"))
    parsed = [(int(r[0]), [float.fromhex(x) for x in r[1:-1]], int(r[-1])) for r in rows]
    assert parsed[0] == (0, [1.0, 2.0, 3.0], 1)                        # nothing due: no promotion is enqueued, the list stays
    assert parsed[1] == (1, [2.0, 3.0], 1)                             # strict: the entry AT now stays outstanding
    assert parsed[2] == (1, [], 0)
