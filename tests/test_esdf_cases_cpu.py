"""The ESDF construction of the oracle (oracle/backend_oracle.c: be_update_esdf2d, the reference the GPU is held to in
tests/test_esdf_cases_gpu.py) against the plain brute-force reference of tests/esdf_cases.py, on the 15 geometries x 14 contents
stated there: thin, clipped, tiny and rounded-up windows with seeds (or none) on the window's rim.  Everything under the final
square root is an exact integer or DBL_MAX, so the comparison is np.array_equal on the whole [nx][ny] field.

The oracle reads a cell past the end of the grid as unknown (0) and touches no memory there; a stand-alone program built from
oracle/backend_oracle.c and tests/harness/esdf_oracle_check.c with the address and undefined-behaviour sanitizers runs every
geometry on grids allocated at exactly nx ny bytes."""
import os
import subprocess

import numpy as np
import pytest

from tests import esdf_cases as cases
from tests.test_esdf_window_cpu import geometry_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = cases.DBL_MAX


def oracle(grid, geom, start=None):
    from oracle.backend_driver import EsdfGrid
    nx, ny, res, x_lo, y_lo, odom, rng = geom
    return EsdfGrid.from_occupancy(grid, x_lo, y_lo, res, odom=odom, detection_range=rng, start=start).dist


@pytest.fixture(scope="module")
def fields():
    """{(geometry, content): (oracle, plain reference, exact transform)}, computed once"""
    out = {}
    for name, key, g in cases.cases():
        geom, win = cases.geometry(name), cases.window(name)
        out[name, key] = (oracle(g, geom), cases.plain(g, geom, win), cases.plain(g, geom, win, alias=False))
    return out


def test_the_oracle_equals_the_plain_reference(fields):
    assert len(fields) == 210
    for (name, key), (orc, ref, _) in fields.items():
        assert orc.shape == cases.geometry(name)[:2]
        assert np.array_equal(orc, ref), (name, key, np.argwhere(orc != ref)[:8])
        min_x, min_y, max_x, max_y = cases.window(name)
        outside = np.ones(orc.shape, bool)
        outside[min_x:max_x, min_y:max_y] = False
        assert (orc[outside] == DBL_MAX).all(), (name, key)
        assert np.isfinite(orc).all() and (orc[~outside] < DBL_MAX).all(), (name, key)


def test_the_alias_moves_column_0_of_the_window_and_nothing_else(fields):
    """Without the alias rule the reference is the exact Euclidean transform.  It differs from the oracle only in column 0 of the
    window, rows >= 1 -- and there it does differ, e.g. on tall_whole with its first row or its first corner occupied: a
    construction that drops the rule (or a `keep` rule of the kernels that lets the wrong thread write) does not pass as exact."""
    differ = set()
    for (name, key), (orc, _, exact) in fields.items():
        min_x, min_y, max_x, max_y = cases.window(name)
        bad = np.argwhere(orc != exact)
        if len(bad):
            differ.add((name, key))
            assert (bad[:, 1] == min_y).all() and (bad[:, 0] >= min_x + 1).all() and (bad[:, 0] < max_x).all(), (name, key, bad[:8])
    assert ("tall_whole", "row_first") in differ and ("tall_whole", "corner_00") in differ
    # interior seeds alone never show it: what the suite held before these cases could not tell the two apart
    assert not any(key == "hole" and name.endswith("_whole") for name, key in differ)


def test_two_updates_in_place():
    """corner_ur's map: the random grid on the whole map, then the checkerboard in tiny_mid's window: the second update changes its
    X x Y cells and keeps every other value of the first"""
    nx, ny, res, x_lo, y_lo = cases.geometry("corner_ur")[:5]
    whole = (nx, ny, res, x_lo, y_lo, (0.0, 0.0), 1e3)
    tiny = cases.geometry("tiny_mid")
    assert tiny[:5] == whole[:5]
    g = cases.contents(nx, ny)
    first = oracle(g["random"], whole)
    second = oracle(g["checker"], tiny, start=first)
    win_whole, win_tiny = (0, 0, nx - 1, ny), cases.window("tiny_mid")   # ny = 48 rounds up, nx = 64 does not
    ref1 = cases.plain(g["random"], whole, win_whole)
    ref2 = cases.plain(g["checker"], tiny, win_tiny, dist=ref1)
    assert np.array_equal(first, ref1) and np.array_equal(second, ref2)
    changed = np.argwhere(second != first)
    assert len(changed) and (changed >= (31, 23)).all() and (changed < (33, 25)).all()


def test_the_oracle_reads_nothing_past_the_grid(tmp_path):
    exe = str(tmp_path / "esdf_oracle_check")
    subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "harness", "esdf_oracle_check.c"), os.path.join(ROOT, "oracle", "backend_oracle.c"),
                    "-o", exe, "-lm"], check=True, timeout=300)
    r = subprocess.run([exe, geometry_file(str(tmp_path / "geometries.txt"))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")[:-1]
    assert [ln.split()[:3] for ln in lines] == [[name, str(state), "0"] for name in cases.NAMES for state in (1, 2)]
    for ln in lines:   # every cell of the window's X x Y is written, with a value below DBL_MAX, and no other
        name, _, _, written = ln.split()
        min_x, min_y, max_x, max_y = cases.window(name)
        assert int(written) == (max_x - min_x) * (max_y - min_y), ln
