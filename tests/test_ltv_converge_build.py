"""LTV-MPC with the reference's stopping rule (alore_ltv_get_cmd_converge / _tick_converge / _relin_info), CPU side: the three calls
are declared, exported and bound, and both converged (CONV) builds of the lanes kernel exist in the assembly next to their plain twins,
with no more scratch and no more spilled VGPRs than those.  CPU-only: hipcc cross-compiles without a GPU."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc")
LIB = os.path.join(ROOT, "alore_legged_manipulator_amd", "libalore_nmpc.so")
NAMES = ("alore_ltv_get_cmd_converge", "alore_ltv_tick_converge", "alore_ltv_relin_info")


def test_converge_calls_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "alore_ltv_mpc.h")).read()
    from alore_legged_manipulator_amd import _lib
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in bound, name
    # the header states the rule with the reference's lines, and what a wavefront's time follows
    assert "mpc.cpp:581-583" in hdr and "mpc.cpp:584" in hdr and "slowest" in hdr


@pytest.mark.skipif(not os.path.exists(LIB), reason="libalore_nmpc.so not built")
def test_converge_calls_are_exported():
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\sT\s+" + name + r"$", syms, re.M), name


def _ltv_assembly(td):
    """ltv_mpc.hip to gfx950 assembly with the flags of the csrc Makefile (the common FLAGS and the file's own additions)"""
    flags, extra = None, None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("FLAGS"):
            flags = line.split(":=", 1)[1].split()
        if line.startswith("build/ltv_mpc.o: FLAGS +="):
            extra = line.split("+=", 1)[1].split()
    assert flags and extra, "flags of ltv_mpc.hip not found in the csrc Makefile"
    flags = [f.replace("$(ARCH)", "gfx950") for f in flags + extra if f != "-fPIC"]
    out = os.path.join(td, "ltv.s")
    subprocess.run([HIPCC] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, "ltv_mpc.hip"), "-o", out], check=True, capture_output=True, timeout=600)
    return out


def _resources(path):
    """{(S, CONV): (scratch bytes, spilled VGPRs)} of every get_cmd_lanes_kernel in the .amdgpu_metadata block"""
    recs, cur = [], {}
    for line in open(path):
        m = re.match(r"\s+(?:- )?\.(name|agpr_count|private_segment_fixed_size|vgpr_spill_count):\s+(\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "agpr_count" and "agpr_count" in cur:
            recs.append(cur)
            cur = {}
        cur[k] = v
    recs.append(cur)
    out = {}
    for r in recs:
        mm = re.match(r"_ZN3ltv20get_cmd_lanes_kernelILi(\d+)ELb([01])EEE", r.get("name", ""))
        if mm and not r["name"].endswith(".kd"):
            out[(int(mm.group(1)), int(mm.group(2)))] = (int(r["private_segment_fixed_size"]), int(r["vgpr_spill_count"]))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_both_conv_builds_exist_and_spill_no_more_than_their_twins():
    with tempfile.TemporaryDirectory() as td:
        res = _resources(_ltv_assembly(td))
    assert sorted(res) == [(2, 0), (2, 1), (4, 0), (4, 1)], sorted(res)
    for S in (2, 4):
        assert res[(S, 1)][0] <= res[(S, 0)][0] and res[(S, 1)][1] <= res[(S, 0)][1], (S, res)
