"""csrc/laser_scan.h (laser scans of a world cloud) on the CPU against its oracle, tests/laser_scan_cases.py, and the build side of
the feature: the alore_backend_laser_* calls are declared, exported and bound, the kernels are in the gfx950 code object.

tests/harness/laser_scan_check.cpp includes the header, is compiled with g++ (once more as a stand-alone program with the address
and undefined-behaviour sanitizers) and runs the scenes through laser::scan_one.  The range image, hit count, compact order,
laser-frame and world-frame floats, status, and the perspective sets sorted by index are compared with the oracle for EQUALITY: both
sides call the same libm, every other step is a correctly rounded operation with contraction off, and the image is a minimum over
doubles, which does not depend on the order of the points."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import laser_scan_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "harness", "laser_scan_check.cpp")
LIB = os.path.join(ROOT, "alore_legged_manipulator_amd", "libalore_nmpc.so")
FLAGS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
LASER_CALLS = ("alore_backend_laser_default_params", "alore_backend_laser_create", "alore_backend_laser_set_cloud",
               "alore_backend_laser_scan", "alore_backend_device_laser", "alore_backend_get_laser")
ALL = list(cases.SCENES)


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("laser_scan_check")
    out = {}
    for name, flags in FLAGS.items():
        out[name] = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC, SRC, "-o", out[name]])
    return out


def run(exe, s, path):
    p = s["params"]
    with open(path, "w") as f:
        f.write(" ".join(repr(p[k]) for k in cases.FIELDS) + " %d %d %d\n" % (len(s["cloud"]), len(s["poses"]), s["capacity"]))
        for pt in s["cloud"]:
            f.write("%r %r %r\n" % tuple(float(v) for v in pt))
        for pose in s["poses"]:
            f.write("%r %r %r\n" % tuple(float(v) for v in pose))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    S, out = s["sensor"], []
    slots = s["capacity"] if S.perspective else S.hrz * S.vtc
    for k in range(len(s["poses"])):
        status, count = (int(v) for v in lines[6 * k].split())
        arr = [np.array([float(v) for v in lines[6 * k + j].split()]) for j in range(1, 6)]
        out.append(dict(status=status, count=count, image=None if S.perspective else arr[0].reshape(S.hrz, S.vtc),
                        laser=arr[1].astype(np.float32).reshape(slots, 3), world=arr[2].astype(np.float32).reshape(slots, 3),
                        index=arr[3].astype(np.int32), compact=None if S.perspective else arr[4].astype(np.float32).reshape(slots, 3)))
    return out


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def same_as_oracle(S, got, want, where):
    assert got["status"] == want.status and got["count"] == want.count, (where, got["status"], got["count"], want.status, want.count)
    if S.perspective:
        if want.status == cases.E_CAPACITY:
            return                                                       # the slots are unspecified
        m = want.count
        order = np.argsort(got["index"][:m], kind="stable")
        assert same(got["index"][:m][order], want.index[:m]), where      # the oracle's set is in index order
        assert same(got["laser"][:m][order], want.laser[:m]) and same(got["world"][:m][order], want.world[:m]), where
        assert np.isnan(got["laser"][m:]).all() and np.isnan(got["world"][m:]).all() and (got["index"][m:] == -1).all(), where
        return
    assert (got["image"] == want.image).all(), where
    assert same(got["laser"], want.laser) and same(got["world"], want.world), where
    assert same(got["index"], want.index) and same(got["compact"], want.compact), where


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
@pytest.mark.parametrize("name", ALL)
def test_header_equals_the_oracle(exes, build, name, tmp_path):
    s = cases.scene(name)
    got = run(exes[build], s, str(tmp_path / "scene.txt"))
    for k, (g, w) in enumerate(zip(got, cases.expected(name))):
        same_as_oracle(s["sensor"], g, w, (name, k))


@pytest.mark.parametrize("name", ALL)
def test_the_guard_holds_on_every_scene(name):
    looked = cases.guard(name)
    assert looked > 0 or len(cases.scene(name)["cloud"]) == 0


@pytest.mark.parametrize("name", cases.RANGE_SCENES)
def test_hit_bins_hold_the_nearest_point_that_falls_into_them(name):
    s = cases.scene(name)
    S = s["sensor"]
    for r in cases.expected(name):
        if r.status != cases.OK:
            assert r.count == 0 and (r.image == cases.EMPTY).all() and np.isnan(r.laser).all() and np.isnan(r.world).all()
            continue
        distances = {dis for _, dis, idx in r.in_range if idx is not None}
        hit = r.image < cases.EMPTY
        assert int(hit.sum()) == r.count and all(float(v) in distances for v in r.image[hit])
        for _, dis, idx in r.in_range:
            if idx is not None:
                assert r.image[idx] <= dis
        assert np.isnan(r.laser[~hit.reshape(-1)]).all() and np.isfinite(r.laser[hit.reshape(-1)]).all()
        assert (r.index[:r.count] == np.flatnonzero(hit.reshape(-1))).all() and (r.index[r.count:] == -1).all()
        if not S.filter:                                                 # without the spread a bin is hit only by a point that falls into it
            assert {idx for _, _, idx in r.in_range if idx is not None} == {(int(b) // S.vtc, int(b) % S.vtc) for b in r.index[:r.count]}


def test_the_scenes_hold_what_they_should():
    ex = cases.expected
    assert all(r.count == 0 and r.status == 0 for r in ex("empty") + ex("perspective_empty"))
    assert [r.count for r in ex("one")] == [1] * len(cases.POSES)
    room = cases.cloud("room")
    assert len(cases.cloud("n257")) == 257 and 1000 < len(room) < 4000
    assert np.isnan(room).any() and np.isinf(room).any()
    for name in ("room16", "room2f", "tiny", "limited"):
        s = cases.scene(name)
        for r in ex(name):
            seen = [i for i, _, _ in r.in_range]
            assert len(seen) < np.isfinite(room).all(1).sum()                            # some points lie beyond the horizon
            assert any(idx is None for _, _, idx in r.in_range)                          # ... some outside the field of view
            assert 0 < r.count < s["sensor"].hrz * s["sensor"].vtc or s["sensor"].filter  # (the closest points fill the ring)
    # occlusion: a pillar hides the wall behind it -- fewer wall points are nearest in their bin than fall into one
    r = ex("room16")[0]
    falls = {}
    for i, dis, idx in r.in_range:
        if idx is not None:
            falls.setdefault(idx, []).append(dis)
    assert any(len(v) > 1 and min(v) < 0.7 * max(v) for v in falls.values())
    assert any(sorted(v)[0] == sorted(v)[1] for v in falls.values() if len(v) > 1)      # ties on the distance in one bin
    # the seam: bin 0 takes points from both sides of +-pi (an index of hrz becomes 0)
    S = cases.scene("room16")["sensor"]
    for pose, r in zip(cases.POSES, ex("room16")):
        c, sn = math.cos(pose[2]), math.sin(pose[2])
        at_seam = [cases.seen(S, room[i], pose, c, sn)[6] for i, _, idx in r.in_range if idx is not None and idx[0] == 0]
        assert any(a > 3.14 for a in at_seam) and any(a < -3.14 for a in at_seam), pose
        raw = [math.floor((a + (math.pi + S.hrz_res / 2.0)) / S.hrz_res) for a in at_seam]
        assert S.hrz in raw and 0 in raw
    # the filter's spread covers the whole ring for the closest points, and a horizontal limit empties the image's back
    assert all((r.image[:, 0] < 0.04).all() for r in ex("room2f"))
    assert all((r.image < cases.EMPTY).all() for r in ex("tiny"))
    for r in ex("limited"):
        assert (r.image[:134] == cases.EMPTY).all() and (r.image[227:] == cases.EMPTY).all() and (r.image[136:225] < cases.EMPTY).any()
    # the point at the sensor is skipped in range mode and seen in perspective mode
    for r, p in zip(ex("at_sensor"), ex("perspective_at_sensor")):
        assert any(dis == 0.0 and idx is None for _, dis, idx in r.in_range) and r.image.min() > 0.0
        assert (p.laser[:p.count] == 0.0).all(1).sum() == 1
    assert [r.status for r in ex("bad_pose")] == [0, cases.E_POSE, 0, cases.E_POSE, cases.E_POSE, 0]
    assert [r.status for r in ex("perspective_bad_pose")] == [0, cases.E_POSE, 0, cases.E_POSE, cases.E_POSE, 0]
    assert all(r.status == 0 and cases.PERSPECTIVE_OVERFLOWS < r.count <= cases.PERSPECTIVE_FITS for r in ex("perspective_fits"))
    assert all(r.status == cases.E_CAPACITY and r.count > cases.PERSPECTIVE_OVERFLOWS for r in ex("perspective_overflows"))
    assert [r.count for r in ex("perspective_overflows")] == [r.count for r in ex("perspective_fits")]


# ---- the build side ---------------------------------------------------------------------------------------------------------
def test_laser_calls_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alore_backend.h")).read(), flags=re.S)
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    from alore_legged_manipulator_amd import _lib, backend
    lib = _lib.load()
    backend._bind(lib)
    for name in LASER_CALLS:
        assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", hdr), name
        assert re.search(r"\sT\s+" + name + r"$", syms, re.M), name
        assert getattr(lib, name).argtypes is not None, name
    for method in ("laser_create", "laser_set_cloud", "laser_scan", "laser_results", "laser_device_view"):
        assert hasattr(backend.BatchedMSPlanner, method), method
    for k, v in (("OK", 0), ("E_POSE", -1), ("E_CAPACITY", -2)):
        assert re.search(r"#define\s+ALORE_BE_LASER_%s\s+\(?%d\)?" % (k, v), hdr), k
        assert getattr(backend, "LASER_" + k) == v == getattr(cases, k)
    assert re.search(r"#define\s+ALORE_BE_LASER_MAX_BINS\s+8192", hdr) and backend.LASER_MAX_BINS == 8192


def test_struct_mirrors_have_the_c_layout(tmp_path):
    from alore_legged_manipulator_amd import backend
    code = ('#include <stdio.h>\n#include "alore_backend.h"\nint main(){printf("%zu %zu", sizeof(alore_backend_laser_params), '
            'sizeof(alore_backend_laser_view));}')
    (tmp_path / "s.c").write_text(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    sizes = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert sizes == [C.sizeof(backend.LaserParamsC), C.sizeof(backend.LaserViewC)]
    assert [n for n, _ in backend.LaserParamsC._fields_] == list(cases.FIELDS)


def test_default_laser_params_need_no_gpu():
    from alore_legged_manipulator_amd import backend
    p = backend.default_laser_params()
    assert {k: getattr(p, k) for k in cases.FIELDS} == cases.DEFAULTS


def test_the_kernels_are_in_the_gfx950_code_object():
    blob = open(LIB, "rb").read()
    assert b"laser_range_kernel" in blob and b"laser_perspective_kernel" in blob and b"gfx950" in blob
