"""Object classes of the back_end (alore_backend_set_classes and its companions, the per-slot xv hand-over of the trajectory store),
CPU side: the calls are declared, exported and bound with argument types, and the ctypes / numpy mirrors of
alore_backend_class_view and alore_backend_class_stat have the C layout."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "alore_legged_manipulator_amd", "libalore_nmpc.so")
BACKEND = ("alore_backend_set_classes", "alore_backend_set_problem_classes", "alore_backend_device_classes", "alore_backend_class_stats")
NMPC = ("alore_nmpc_refs_set_from_backend_xv", "alore_nmpc_refs_set_pending_from_backend_xv")
STAT_FIELDS = ("n", "n_ok", "n_collision", "sum_attempts", "sum_evals", "max_evals", "pad", "min_dist", "max_duration")
VIEW_FIELDS = ("n_classes", "pad", "class_of", "xv", "clamped", "classes", "stats")


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_calls_are_declared_and_exported():
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for hdr, names in ((header("alore_backend.h"), BACKEND), (header("alore_nmpc.h"), NMPC)):
        for name in names:
            assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
            assert re.search(r"\sT\s+" + name + r"$", syms, re.M), name
    hdr = header("alore_backend.h")
    assert re.search(r"typedef\s+struct\s+alore_backend_class_stat\s*\{", hdr)
    assert re.search(r"typedef\s+struct\s+alore_backend_class_view\s*\{", hdr)
    assert re.search(r"#define\s+ALORE_BE_MAX_CLASSES\s+256\b", hdr)


def c_layout(struct, fields):
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "alore_backend.h"\nint main(){printf("%%zu", sizeof(%s));' % struct
            + "".join('printf(" %%zu", offsetof(%s, %s));' % (struct, f) for f in fields) + "}")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(code)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        return [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]


def test_records_have_the_c_layout_on_every_side():
    from alore_legged_manipulator_amd import backend
    got = c_layout("alore_backend_class_stat", STAT_FIELDS)
    assert got[0] == 48 == C.sizeof(backend.ClassStatC) == backend.CLASS_STAT_DTYPE.itemsize
    assert tuple(n for n, _ in backend.ClassStatC._fields_) == STAT_FIELDS == backend.CLASS_STAT_DTYPE.names
    assert got[1:] == [getattr(backend.ClassStatC, f).offset for f in STAT_FIELDS] == [backend.CLASS_STAT_DTYPE.fields[f][1] for f in STAT_FIELDS]
    assert backend.CLASS_STAT_DTYPE["sum_evals"].itemsize == 8 == C.sizeof(C.c_longlong)
    got = c_layout("alore_backend_class_view", VIEW_FIELDS)
    assert got[0] == 48 == C.sizeof(backend.ClassViewC)
    assert tuple(n for n, _ in backend.ClassViewC._fields_) == VIEW_FIELDS
    assert got[1:] == [getattr(backend.ClassViewC, f).offset for f in VIEW_FIELDS]
    assert backend.MAX_CLASSES == 256


def test_binding_sets_argtypes():
    from alore_legged_manipulator_amd import _lib, backend, nmpc
    lib = _lib.load()
    backend._bind(lib)
    assert lib.alore_backend_set_classes.argtypes == [C.c_void_p, C.c_int, C.POINTER(backend.BackendConfig), C.POINTER(backend.FrontEndParamsC)]
    assert lib.alore_backend_set_problem_classes.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    assert lib.alore_backend_device_classes.argtypes == [C.c_void_p, C.POINTER(backend.ClassViewC)]
    assert lib.alore_backend_class_stats.argtypes == [C.c_void_p, C.c_int, C.POINTER(backend.ClassStatC), C.c_void_p]
    assert lib.alore_nmpc_refs_set_from_backend_xv.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_double, C.c_int,
                                                                C.c_void_p]
    assert lib.alore_nmpc_refs_set_pending_from_backend_xv.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double,
                                                                        C.c_void_p, C.c_double, C.c_int, C.c_void_p]
    for name in ("set_classes", "set_problem_classes", "class_view", "class_xv", "class_stats"):
        assert callable(getattr(backend.BatchedMSPlanner, name)), name
    assert callable(nmpc.BatchedNmpc.refs_set_from_backend)
