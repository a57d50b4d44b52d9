"""Converged solves to a KKT tolerance (alore_nmpc_rti_converge / alore_nmpc_rti_many_converge), CPU side: the two calls are declared,
exported and bound, and every converged-solve (CONV) build of the stage-block kernel exists in the assembly with the registers of its
plain twin.  CPU-only: hipcc cross-compiles without a GPU."""
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
LIB = os.path.join(ROOT, "alore_legged_manipulator_amd", "libalore_nmpc.so")
NAMES = ("alore_nmpc_rti_converge", "alore_nmpc_rti_many_converge")


def test_converge_calls_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "alore_nmpc.h")).read()
    from alore_legged_manipulator_amd import _lib
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in bound, name


@pytest.mark.skipif(not os.path.exists(LIB), reason="libalore_nmpc.so not built")
def test_converge_calls_are_exported():
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\sT\s+" + name + r"$", syms, re.M), name


def _resources(path):
    """{(template arguments): (scratch bytes, spilled VGPRs)} of every rti_block_kernel of the assembly (records of the
    .amdgpu_metadata block, as tools/kernel_resources.py reads them)"""
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
        mm = re.match(r"_ZN4nmpc16rti_block_kernelI((?:L[ib]\d+E)+)E", r.get("name", ""))
        if mm and not r["name"].endswith(".kd"):
            args = tuple(int(a) for a in re.findall(r"L[ib](\d+)E", mm.group(1)))
            out[args] = (int(r["private_segment_fixed_size"]), int(r["vgpr_spill_count"]))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_every_conv_build_exists_and_keeps_the_registers_of_its_twin():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_masked_regions import block_kernel_assembly
    with tempfile.TemporaryDirectory() as td:
        res = _resources(block_kernel_assembly(td))
    # (L, S, DIAG, STAMP, ONCE, FULLN, TRACE, PERSIST, TWOPH, CONV): the five mappings and the FULLN (4, 5) build, DIAG, several iterations
    twins = [(4, 5, 0), (8, 3, 0), (16, 2, 0), (16, 4, 0), (32, 1, 0), (4, 5, 1)]
    # The two (4, 5) builds sit at the register limit and spill already; the frozen results and the `done` flag of a converged solve
    # cost them a little more (measured: scratch 560 / 548 and 336 / 292 bytes, spills 171 / 162 and 140 / 135).  Every other build
    # must not use more scratch or spill more than its twin.
    slack = {(4, 5, 0): (1.05, 1.10), (4, 5, 1): (1.20, 1.10)}
    for L, S, full in twins:
        plain = res.get((L, S, 1, 0, 0, full, 0, 0, 0, 0))
        conv = res.get((L, S, 1, 0, 0, full, 0, 0, 0, 1))
        assert plain is not None and conv is not None, (L, S, full, sorted(res))
        fs, fp = slack.get((L, S, full), (1.0, 1.0))
        assert conv[0] <= plain[0] * fs, ((L, S, full), conv, plain)
        assert conv[1] <= plain[1] * fp, ((L, S, full), conv, plain)
