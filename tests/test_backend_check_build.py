"""alore_backend_check_plans / alore_backend_device_check (the stored plans against the map of now), CPU side: the two calls are
declared, exported and bound with argument types, and the ctypes / numpy mirrors of alore_backend_check have the C layout."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "alore_legged_manipulator_amd", "libalore_nmpc.so")
NAMES = ("alore_backend_check_plans", "alore_backend_device_check")


def test_check_calls_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "alore_backend.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert re.search(r"\sT\s+" + name + r"$", syms, re.M), name
    assert re.search(r"typedef\s+struct\s+alore_backend_check\s*\{", hdr)


def test_record_is_48_bytes_on_both_sides():
    from alore_legged_manipulator_amd import backend
    assert C.sizeof(backend.CheckC) == 48 and backend.CHECK_DTYPE.itemsize == 48
    fields = ("collision", "first_panel", "n_checked", "pad", "first_time", "first_xy", "min_dist")
    assert tuple(n for n, _ in backend.CheckC._fields_) == fields == backend.CHECK_DTYPE.names
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "alore_backend.h"\nint main(){printf("%zu", sizeof(alore_backend_check));'
            + "".join('printf(" %%zu", offsetof(alore_backend_check, %s));' % f for f in fields) + "}")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(code)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got[0] == 48
    assert got[1:] == [getattr(backend.CheckC, f).offset for f in fields] == [backend.CHECK_DTYPE.fields[f][1] for f in fields]


def test_binding_sets_argtypes():
    from alore_legged_manipulator_amd import _lib, backend
    lib = _lib.load()
    backend._bind(lib)
    assert lib.alore_backend_check_plans.argtypes == [C.c_void_p, C.c_int, backend.DP, backend.DP, C.c_double, C.c_int,
                                                      C.POINTER(backend.CheckC), C.c_void_p]
    assert lib.alore_backend_device_check.argtypes == [C.c_void_p, C.POINTER(C.c_void_p)]
    assert callable(getattr(backend.BatchedMSPlanner, "check_plans"))
