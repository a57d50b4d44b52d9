"""The ESDF construction on the GPU (csrc/esdf_build.hip) against the oracle (oracle/backend_oracle.c: be_update_esdf2d) on the
cases of tests/esdf_cases.py: thin, clipped, tiny and rounded-up windows, each with 14 contents that put seeds (or none) on the
window's rim, where the reference's aliased scratch, the read of g[Y] and the lines without a seed show.  tests/test_esdf_cases_cpu.py
holds the oracle to a plain brute-force reference on the same cases.

Both routes are compared: alore_backend_build_esdf (buffers of its own, sized for the window) and the resident map
(map_create / map_set_grid / map_update_esdf: one workspace per handle, sized for the map's detection range).  All values are sums of
squared integers or DBL_MAX until the final square root, so the fields are compared with np.array_equal on the whole [nx][ny] array.
Where the window ends past the map the cells past the grid are unknown (0) on every route; the last test runs such windows after
calls that leave other contents in freed device memory and in the workspace."""
import numpy as np
import pytest

from tests import esdf_cases as cases

pytestmark = pytest.mark.gpu


def planner():
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    return BatchedMSPlanner(1, 16)


def oracle(grid, geom, start=None):
    from oracle.backend_driver import EsdfGrid
    nx, ny, res, x_lo, y_lo, odom, rng = geom
    return EsdfGrid.from_occupancy(grid, x_lo, y_lo, res, odom=odom, detection_range=rng, start=start).dist


def build(pl, grid, geom):
    nx, ny, res, x_lo, y_lo, odom, rng = geom
    return pl.build_esdf(grid, x_lo, y_lo, res, odom=odom, detection_range=rng)


def same(dev, ref, what):
    assert dev.shape == ref.shape and np.array_equal(dev, ref), (what, np.argwhere(dev != ref)[:8])


@pytest.mark.parametrize("name", cases.NAMES)
def test_build_esdf_is_bit_identical_to_the_oracle(name):
    geom = cases.geometry(name)
    for key, g in cases.contents(*geom[:2]).items():
        pl = planner()   # no map yet: the build starts from DBL_MAX everywhere
        same(build(pl, g, geom), oracle(g, geom), (name, key))
        pl.close()


@pytest.mark.parametrize("name", cases.NAMES)
def test_resident_esdf_is_bit_identical_to_the_oracle(name):
    geom = cases.geometry(name)
    nx, ny, res, x_lo, y_lo, odom, rng = geom
    for key, g in cases.contents(nx, ny).items():
        pl = planner()
        pl.map_create(nx, ny, x_lo, y_lo, res, detection_range=rng)
        pl.map_set_grid(g)
        pl.map_update_esdf(odom, rng)
        st = pl.map_state()
        assert np.array_equal(st["grid"], g)
        same(st["dist"], oracle(g, geom), (name, key))
        pl.close()


def test_the_field_does_not_depend_on_what_ran_before():
    from alore_legged_manipulator_amd.backend import BackendError
    # build_esdf of a larger map full of occupied cells, then of a map whose window ends a row past it, all free: the row past
    # the grid reads as unknown, not as what the freed buffers held
    pl = planner()
    big = (150, 150, 0.1, -7.5, -7.5, (0.0, 0.0), 1e3)
    g_big = np.full((150, 150), 2, np.uint8)
    same(build(pl, g_big, big), oracle(g_big, big), "150 x 150 occupied")
    geom = cases.geometry("roundup_x")
    g = cases.contents(*geom[:2])["free"]
    same(build(pl, g, geom), oracle(g, geom), "roundup_x free after 150 x 150 occupied")
    pl.close()

    # a row and a column past the map, then another map and a window of 1 x 2 cells at its corner
    pl = planner()
    geom = cases.geometry("roundup_xy")
    g = cases.contents(*geom[:2])["random"]
    same(build(pl, g, geom), oracle(g, geom), "roundup_xy random")
    geom = cases.geometry("tiny_edge")
    for key in ("random", "occupied"):
        g = cases.contents(*geom[:2])[key]
        same(build(pl, g, geom), oracle(g, geom), ("tiny_edge after roundup_xy", key))
    pl.close()

    # the resident map: one workspace sized for the whole map, used by the whole map and then by a window of 2 x 2 cells
    pl = planner()
    tiny = cases.geometry("tiny_mid")
    nx, ny, res, x_lo, y_lo = tiny[:5]
    whole = (nx, ny, res, x_lo, y_lo, (0.0, 0.0), 1e3)
    c = cases.contents(nx, ny)
    pl.map_create(nx, ny, x_lo, y_lo, res, detection_range=1e3)
    pl.map_set_grid(c["random"])
    pl.map_update_esdf(whole[5], whole[6])
    first = oracle(c["random"], whole)
    same(pl.map_state()["dist"], first, "resident, whole map")
    pl.map_set_grid(c["checker"])
    pl.map_update_esdf(tiny[5], tiny[6])
    second = oracle(c["checker"], tiny, start=first)
    assert not np.array_equal(first, second)
    same(pl.map_state()["dist"], second, "resident, tiny_mid's window in the whole map's workspace")
    pl.close()

    # a window above the map's detection range is refused and the field stays as it is
    pl = planner()
    geom = cases.geometry("corner_ll")
    nx, ny, res, x_lo, y_lo, odom, rng = geom
    g = cases.contents(nx, ny)["random"]
    pl.map_create(nx, ny, x_lo, y_lo, res, detection_range=rng)
    pl.map_set_grid(g)
    pl.map_update_esdf(odom, rng)
    ref = oracle(g, geom)
    same(pl.map_state()["dist"], ref, "resident, corner_ll")
    with pytest.raises(BackendError):
        pl.map_update_esdf((0.0, 0.0), 2.5 * rng)
    same(pl.map_state()["dist"], ref, "resident, after the refused window")
    pl.close()
