"""csrc/backend_classes.h (object classes of the back_end: the validation of a class against the handle's config, the effective xv
of a config, the per-class reduction of status records) on the CPU.

tests/harness/backend_classes_check.cpp includes the header, is compiled with g++ -ffp-contract=off (once more with the address and
undefined-behaviour sanitizers, as a stand-alone program) and is compared with NumPy: the reduction uses integer sums, minima and
maxima only, so the comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import backend_classes_cases as cases  # noqa: E402

CSRC = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "harness", "backend_classes_check.cpp")
FLAGS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("backend_classes_check")
    out = {}
    for name, flags in FLAGS.items():
        out[name] = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC, SRC, "-o", out[name]])
    return out


def run(exe, mode, payload: bytes, tmp_path) -> bytes:
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(src, "wb").write(payload)
    subprocess.check_call([exe, mode, src, dst])
    return open(dst, "rb").read()


def classes_report(exe, handle, configs, tmp_path):
    payload = np.int32(len(configs)).tobytes() + bytes(handle) + b"".join(bytes(c) for c in configs)
    rows = [ln.split() for ln in run(exe, "classes", payload, tmp_path).decode().splitlines()]
    assert [int(r[0]) for r in rows] == list(range(len(configs)))
    return [(r[1], float(r[2])) for r in rows]


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_validation_and_effective_xv(exes, build, tmp_path):
    from alore_legged_manipulator_amd.backend import default_config
    handle = default_config()
    good = cases.class_configs()
    rep = classes_report(exes[build], handle, good, tmp_path)
    assert [r[0] for r in rep] == ["ok"] * 4                      # the four classes of the scene are accepted
    assert [r[1] for r in rep] == [0.0, 0.2, 0.3, 0.1]            # 0 for standard_diff, else icr_xv
    assert [r[1] for r in rep] == [cases.effective_xv(c) for c in good]
    bad = cases.class_configs()
    bad[1].sparse_res = 4
    bad[2].n_check = 9
    bad[3].final_check_num = 65
    rep = classes_report(exes[build], handle, bad, tmp_path)
    assert [r[0] for r in rep] == ["ok", "sparse_res", "n_check", "final_check_num"]   # the field is named
    # a standard_diff class with a non-zero icr_xv integrates with 0
    sd = default_config()
    sd.icr_xv, sd.standard_diff = 0.7, 1
    assert classes_report(exes[build], handle, [sd], tmp_path) == [("ok", 0.0)]


def random_records(rng, count, n_classes, P, empty):
    from alore_legged_manipulator_amd.backend import StatusC
    dt = np.dtype([(n, np.int32) for n in ("ok", "attempts", "alm_rounds", "evals", "lbfgs_ret", "path_ret", "collision", "n_pieces")] +
                  [("cost", np.float64), ("xy_err", np.float64, 2), ("min_dist", np.float64), ("tail_s", np.float64)])
    assert dt.itemsize == C.sizeof(StatusC) == 72
    st = np.zeros(count, dt)
    st["ok"] = rng.integers(0, 2, count)
    st["collision"] = 1 - st["ok"]
    st["attempts"] = rng.integers(1, 4, count)
    st["evals"] = rng.integers(50, 2_000_000_000, count)          # the 64-bit sum is needed
    st["n_pieces"] = rng.integers(1, P + 1, count)
    st["min_dist"] = rng.uniform(0.1, 3.0, count)
    class_of = rng.integers(0, n_classes, count).astype(np.int32)
    class_of[class_of == empty] = (empty + 1) % n_classes
    T = rng.uniform(0.2, 2.0, (count, P))
    return class_of, st, T


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_reduction_equals_numpy(exes, build, tmp_path):
    from alore_legged_manipulator_amd.backend import CLASS_STAT_DTYPE
    rng = np.random.default_rng(20)
    count, n_classes, P, empty = 200, 5, 16, 3
    class_of, st, T = random_records(rng, count, n_classes, P, empty)
    st["ok"][class_of == 1] = 0                                   # a class without a successful plan: DBL_MAX and 0
    payload = np.array([count, n_classes, P, 1], np.int32).tobytes() + class_of.tobytes() + st.tobytes() + T.tobytes()
    got = np.frombuffer(run(exes[build], "reduce", payload, tmp_path), CLASS_STAT_DTYPE)
    ref = cases.stats_numpy(class_of, st, T, n_classes)
    assert got.tobytes() == ref.tobytes()
    assert got["n"][empty] == 0 and got["min_dist"][empty] == np.finfo(np.float64).max and got["max_duration"][empty] == 0.0
    assert got["n"][1] > 0 and got["n_ok"][1] == 0 and got["min_dist"][1] == np.finfo(np.float64).max
    assert got["n"].sum() == count and got["sum_evals"].max() > 2**31
    # without indices every slot is class 0
    payload = np.array([count, 1, P, 0], np.int32).tobytes() + class_of.tobytes() + st.tobytes() + T.tobytes()
    one = np.frombuffer(run(exes[build], "reduce", payload, tmp_path), CLASS_STAT_DTYPE)
    assert one.tobytes() == cases.stats_numpy(np.zeros(count, np.int32), st, T, 1).tobytes()
