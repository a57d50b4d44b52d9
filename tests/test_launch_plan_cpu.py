"""csrc/nmpc_launch_plan.h on the CPU: the stagger, two-phase and XCD plans, the launch geometry and the choice of the kernel build,
compiled with g++ alone (address and undefined-behaviour sanitizers on) into a stand-alone program that is run as a child process.
Every expected value is worked out here from the rules the launch path has always followed."""
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "harness", "launch_plan_harness.cpp")
HDR = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc", "nmpc_launch_plan.h")
MAPPINGS = [(4, 5), (8, 3), (16, 2), (16, 4), (32, 1)]


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    SRC, "-o", exe], check=True, timeout=300)
    text = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    rows = {}
    for line in text.splitlines():
        key, _, val = line.partition(" = ")
        key = key.rstrip(" =")
        tag, _, args = key.partition(" ")
        rows.setdefault(tag, []).append((args.split(), val.split()))
    return rows


def one(rows, tag, name=None):
    hits = [v for a, v in rows[tag] if name is None or (a and a[0] == name)]
    assert len(hits) == 1, (tag, name, hits)
    return hits[0]


def test_header_is_plain_cpp():
    text = open(HDR).read()
    assert sorted(re.findall(r"#include\s+(\S+)", text)) == ["<cmath>", "<cstddef>"]
    assert not re.search(r"getenv|\bhip[A-Z_]\w*|alore_nmpc_handle|alore_nmpc_solver", text)


def test_stagger(out):
    got = {tuple(a): [int(x) for x in v] for a, v in out["stagger"]}
    # 4 * 256 = 1024 resident blocks of 4 * (51 * 20 + 28) * 16 = 67072 B: 1024 * 67072 / 7.5e3 = 9157.6 ns over 1024 blocks in ticks of 10 ns, x 1024
    assert 4 * (51 * 20 + 28) * 16 == 67072
    assert int(1024 * 67072 / 7.5e3 / 10.0 / 1024 * 1024.0 + 0.5) == 916
    assert got[("256", "20", "16", "256", "20", "0", "0")] == [1024, 916]
    assert got[("256", "20", "16", "256", "7", "0", "0")] == [0, 0]      # 256 * 7 < 2048: less than two residencies
    assert got[("256", "20", "16", "256", "8", "0", "0")] == [1024, 916]  # exactly two
    assert got[("256", "20", "16", "256", "20", "1", "0")] == [0, 0]     # override 0 ns: off
    assert got[("256", "20", "16", "256", "20", "1", "5000")] == [1024, int(5000.0 / 10.0 / 1024 * 1024.0 + 0.5)]


def test_two_phase(out):
    def tp(name):
        return [int(x) for x in one(out, "two_phase", name)]
    off = [0, 0, 0, 0, 0, 0]
    # tail = ceil(0.30 * 1.08 * 256) + 3 = 86, unit = 342, lag = ceil((1024 + 128) / 342) = 4, count2 = 20 - 4
    assert math.ceil(0.30 * 1.08 * 256) + 3 == 86 and (1024 + 128 + 341) // 342 == 4
    assert tp("default") == [1, 86, 4, 16, 16 * 4 * (16 + 256 * 17), 20 * 342]
    assert tp("count4") == off      # lag 4 leaves no two-phase batch
    lag1 = (1024 + 128 + 256) // 257
    assert tp("tail1") == [1, 1, lag1, 20 - lag1, (20 - lag1) * 4 * (16 + 256 * 17), 20 * 257]
    assert tp("tail0")[1] == 1       # tail clamps to [1, grid]
    lag_full = (1024 + 128 + 511) // 512
    assert tp("tail_huge") == [1, 256, lag_full, 20 - lag_full, (20 - lag_full) * 4 * (16 + 256 * 17), 20 * 512]
    assert tp("lag0") == [1, 86, 1, 19, 19 * 4 * (16 + 256 * 17), 20 * 342]  # lag clamps to at least 1; single follows lag
    assert tp("lag_neg") == tp("lag0")
    assert tp("single_neg") == [1, 86, 4, 20, 20 * 4 * (16 + 256 * 17), 24 * 342]  # single clamps to at least 0: the tails of the last batches need 4 more units
    assert tp("single2") == [1, 86, 4, 18, 18 * 4 * (16 + 256 * 17), 22 * 342]
    assert tp("single_all") == off
    for name in ("conv", "persistent", "unsupported", "unwanted", "one_residency"):
        assert tp(name) == off, name
    assert tp("lag_past_end") == off  # 256 * 3 blocks: below two residencies
    assert [int(x) for x in one(out, "two_phase_blocks")] == [20 * 342, 8 * 342]
    # the (4, 5) grid build at N = 20, one iteration, no stamps, at most 64 * 16 blocks per batch, stage-block kernel
    assert [int(x) for x in one(out, "two_phase_supported")] == [1, 0, 0, 0, 0, 0]


def test_xcd_apportionment(out):
    eq = [int(x) for x in one(out, "xcd_plan", "equal")]
    shares = [1537, 1537] + [1536] * 6
    assert eq == [1] + shares + [sum(shares[:i]) for i in range(8)]
    # at least max(12, 2) * 4 * 256 = 12288 blocks and fewer than 2^28
    assert [int(x) for x in one(out, "xcd_eligible")] == [1, 1, 0, 0, 1, 0]
    draws = [(a, v) for a, v in out["xcd_plan"] if a[0] == "draw"]
    assert len(draws) == 300
    for a, v in draws:
        total, speed = int(a[1]), [float(x) for x in a[2:10]]
        assert all(0.85 <= s <= 1.15 for s in speed)
        on, share, base = int(v[0]), [int(x) for x in v[1:9]], [int(x) for x in v[9:17]]
        assert on == 1 and sum(share) == total and min(share) >= 0, (a, v)
        assert base == [sum(share[:i]) for i in range(8)]
        for s, sp in zip(share, speed):  # largest remainder: within one block of the exact proportion
            assert abs(s - total * sp / sum(speed)) < 1.0 + 1e-9


def test_xcd_speed_update(out):
    def upd(name):
        v = one(out, "xcd_update", name)
        return int(v[0]), [float(x) for x in v[1:]]
    used, sp = upd("equal")
    assert used == 1 and sp == [1.0] * 8
    used, sp = upd("late")  # XCD 3 finished 10 % late
    assert used == 1
    for x in range(8):
        if x != 3:
            assert abs(sp[x] / sp[3] - 1.1 ** 0.7) <= 1e-12
    assert abs(sum(sp) / 8 - 1.0) <= 1e-12
    for name, rounds in (("very_late", 1), ("very_late_x20", 20)):
        used, sp = upd(name)
        assert used == rounds and all(0.85 <= s <= 1.15 for s in sp) and sp[3] == 0.85, (name, sp)
    skew = [0.85, 1.15, 1.0, 1.1, 0.9, 1.0, 1.05, 0.95]
    for name in ("no_start", "end_not_after_start", "too_short"):
        assert upd(name) == (0, skew), name


def test_geometry(out):
    got = {tuple(int(x) for x in a): [int(x) for x in v] for a, v in out["geometry"]}
    lds = lambda N, L: 4 * ((((64 // L) * 25 * N + 255) & ~255) + (((64 // L) * 5 * N + 255) & ~255))
    assert got[(4096, 20, 256, 81920)] == [1, 4, 5, 16, 256, lds(20, 4)]
    assert got[(4096, 50, 256, 81920)] == [1, 16, 4, 4, 1024, lds(50, 16)]
    assert got[(1, 20, 256, 0)] == [1, 32, 1, 2, 1, lds(20, 32)]
    assert got[(1, 65, 256, 0)][0] == 0
    assert got[(4096, 24, 256, 81920)][:3] == [1, 8, 3]   # the packed mapping holds 20 stages: N = 24 widens to 8 lanes
    assert got[(4096, 20, 256, 0)][:3] == [1, 16, 2]      # on its own 4096 problems spread: 1024 wavefronts of 4
    assert got[(300, 20, 256, 0)][:3] == [1, 32, 1]       # 150 wavefronts: every one a CU to itself
    assert [int(x) for x in one(out, "lds_floats")] == [lds(20, 4) // 4, lds(50, 16) // 4, lds(20, 32) // 4]


def expected_build(L, S, N, n_sqp, diag_in, stamp, conv, persist, twoph, trace, xcd):
    """The rules of the launcher as they stood before the table: a cascade in which later matches replace earlier ones, None where
    it answered hipErrorInvalidValue.  (L, S, DIAG, STAMP, ONCE, FULLN, TRACE, PERSIST, TWOPH, CONV)"""
    diag = stamp or diag_in
    if conv and (stamp or persist or twoph or trace):
        return None
    once = n_sqp == 1 and not conv
    fn = None
    if (L, S) in MAPPINGS:
        fn = (L, S, 1, 1, 0, 0, 0, 0, 0, 0) if stamp else (L, S, int(diag), 0, int(once), 0, 0, 0, 0, 0)
    if conv:
        fn = (L, S, 1, 0, 0, 0, 0, 0, 0, 1) if (L, S) in MAPPINGS else None
    fills = L == 4 and S == 5 and N == 20
    if fills and once and not stamp:
        fn = (4, 5, int(diag), 0, 1, 1, 0, 0, 0, 0)
    if fills and not once and not stamp:
        fn = (4, 5, 1, 0, 0, 1, 0, 0, 0, 1) if conv else (4, 5, int(diag), 0, 0, 1, 0, 0, 0, 0)
    if persist:
        if not (fills and once and not stamp):
            return None
        fn = (4, 5, int(diag), 0, 1, 1, 0, 1, 0, 0)
    if twoph:
        if not (fills and once and not stamp) or persist or trace or xcd:
            return None
        fn = (4, 5, int(diag), 0, 1, 1, 0, 0, 1, 0)
    if trace:
        if not (fills and once and not stamp and diag):
            return None
        fn = (4, 5, 1, 0, 1, 1, 1, int(persist), 0, 0)
    return fn


def test_build_selection(out):
    assert [int(x) for x in one(out, "builds")] == [41, 6]
    table = {int(a[0]): tuple(int(x) for x in v) for a, v in out["build"]}
    assert sorted(table) == list(range(41)) and len(set(table.values())) == 41
    seen, n = set(), 0
    for a, v in out["select"]:
        L, S, N, n_sqp, f = (int(x) for x in a)
        flags = [bool(f & (1 << k)) for k in range(7)]  # diag, stamp, conv, persist, two-phase, trace, XCD shares
        want = expected_build(L, S, N, n_sqp, *flags)
        if want is None:
            assert v == ["none"], (a, v)
        else:
            assert v != ["none"], (a, want)
            got = tuple(int(x) for x in v)
            assert got[1:] == want and table[got[0]] == want, (a, got, want)
            seen.add(want)
        n += 1
    assert n == 5 * 3 * 2 * 128
    assert seen == set(table.values())  # every build of the table is reachable, and nothing outside it is ever chosen
    assert one(out, "select_unknown_mapping") == ["-1"]
    plain = {b for b in table.values() if not any(b[5:])}
    assert len(plain) == 25                                              # five mappings x (diag, once) + stamps
    assert len({b for b in table.values() if b[9]}) == 6                 # converged solves: five mappings + the one that fills (4, 5)
    assert expected_build(4, 5, 20, 1, True, False, False, False, False, False, False) == (4, 5, 1, 0, 1, 1, 0, 0, 0, 0)
    assert expected_build(4, 5, 20, 15, False, False, False, False, False, False, False) == (4, 5, 0, 0, 0, 1, 0, 0, 0, 0)


def test_sampler_selection(out):
    table = {int(a[0]): tuple(int(x) for x in v) for a, v in out["sampler_build"]}
    assert sorted(table) == list(range(6)) and len(set(table.values())) == 6
    assert set(table.values()) == {(L, S, d) for (L, S) in ((16, 2), (32, 1), (8, 3)) for d in (0, 1)}
    for a, v in out["sampler"]:
        L, S, N, n_sqp, f = (int(x) for x in a)
        stamp, diag, wave = bool(f & 1), bool(f & 2), bool(f & 4)
        kind = 0
        if not wave and n_sqp == 1 and not stamp and N + 1 <= 32:
            kind = 2 if (L, S) in ((16, 2), (32, 1)) else (1 if (L, S) == (8, 3) else 0)
        got_kind, got_build = int(v[0]), int(v[1])
        assert got_kind == kind, (a, v)
        if kind == 0:
            assert got_build == -1, (a, v)
        else:
            assert table[got_build] == (L, S, int(diag)), (a, v)
