"""csrc/nmpc_group_ops.h on the device: tests/harness/group_ops_check.hip (a program of its own, one wavefront) compares the quad-native
L = 4 forms with the generic text bit for bit, and the L = 8 / 16 scans with serial sums.  Needs a real MI355X."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alore_legged_manipulator_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.gpu
def test_quad_forms_equal_the_generic_ones_bit_for_bit():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "group_ops_check")
        # the flags of csrc/Makefile that bear on the code of the header
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-I" + CSRC,
                               os.path.join(ROOT, "tests", "harness", "group_ops_check.hip"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout, r.stdout
