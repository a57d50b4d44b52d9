"""Laser scans of a resident world cloud on the GPU (alore_backend_laser_*) against the sequential oracle of
tests/laser_scan_cases.py.

Range image, hit count, status, the compact order of the hit bins and the laser-frame points are compared bit for bit: the image is
a minimum over correctly rounded distances, the bin of every point is fixed by the input guard of the cases module (asserted on the
CPU), and the points come from tables computed on the host.  World-frame points may differ by one float: their double value differs
from the oracle's only through sin / cos of the yaw, bounded by OpenCL at 4 units in the last place of a double -- about 3e-14 m at
30 m, far below a float's spacing -- so the rounded float is the same or the adjacent one: the bound is max(one unit in the last
place of the float, 1e-12).  The same bound holds for the laser-frame points of perspective mode."""
import numpy as np
import pytest

from tests import laser_scan_cases as cases
from tests import occupancy_cases as occ

pytestmark = pytest.mark.gpu


def planner():
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    return BatchedMSPlanner(1, 16)


def sensor(s, max_scans=None, pl=None):
    pl = pl or planner()
    pl.laser_create(max_scans or len(s["poses"]), s["capacity"], **s["params"])
    return pl


def scan_scene(name):
    s = cases.scene(name)
    pl = sensor(s)
    pl.laser_set_cloud(s["cloud"])
    pl.laser_scan(np.array(s["poses"]))
    return pl.laser_results(), s


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def within_one_float(got, want, where):
    assert (np.isnan(got) == np.isnan(want)).all(), where
    ok = ~np.isnan(want)
    bound = np.maximum(np.spacing(np.abs(want[ok])).astype(np.float64), 1e-12)
    err = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64))
    assert (err <= bound).all(), (where, float(err.max()))


def by_index(got, k, m):
    order = np.argsort(got["index"][k, :m], kind="stable")
    return got["index"][k, :m][order], got["laser_points"][k, :m][order], got["world_points"][k, :m][order]


def range_equals_oracle(got, k, want, where):
    assert got["status"][k] == want.status and got["n_points"][k] == want.count, (where, got["status"][k], got["n_points"][k], want.count)
    assert (got["range_image"][k] == want.image).all(), where
    assert same(got["index"][k], want.index) and same(got["compact_points"][k], want.compact), where
    assert same(got["laser_points"][k], want.laser), where
    within_one_float(got["world_points"][k], want.world, where)


def perspective_equals_oracle(got, k, want, s, where):
    assert got["status"][k] == want.status and got["n_points"][k] == want.count, (where, got["status"][k], got["n_points"][k], want.count)
    if want.status == cases.E_CAPACITY:
        return
    m = want.count
    index, laser, world = by_index(got, k, m)
    assert same(index, want.index[:m]), where
    assert same(world, s["cloud"][index]), where                          # the source points verbatim
    within_one_float(laser, want.laser[:m], where)
    assert np.isnan(got["laser_points"][k, m:]).all() and np.isnan(got["world_points"][k, m:]).all() and (got["index"][k, m:] == -1).all(), where


@pytest.mark.parametrize("name", cases.RANGE_SCENES)
def test_range_scenes_equal_the_oracle(name):
    got, s = scan_scene(name)
    for k, want in enumerate(cases.expected(name)):
        range_equals_oracle(got, k, want, (name, k))


@pytest.mark.parametrize("name", cases.PERSPECTIVE_SCENES)
def test_perspective_scenes_equal_the_oracle(name):
    got, s = scan_scene(name)
    assert got["range_image"] is None
    for k, want in enumerate(cases.expected(name)):
        perspective_equals_oracle(got, k, want, s, (name, k))
    if name == "perspective_overflows":
        assert (got["status"] == cases.E_CAPACITY).all() and (got["n_points"] > cases.PERSPECTIVE_OVERFLOWS).all()


def scan_bits(got, k, perspective):
    """what a scan left, as comparable bytes (perspective mode: in index order)"""
    m = int(got["n_points"][k])
    if perspective:
        return tuple(a.tobytes() for a in by_index(got, k, m)) + (m, int(got["status"][k]))
    return tuple(got[n][k].tobytes() for n in ("range_image", "laser_points", "world_points", "index", "compact_points")) + (m, int(got["status"][k]))


@pytest.mark.parametrize("name", ["room16", "room2f", "perspective_fits"])
def test_a_scan_does_not_depend_on_its_batch_mates_or_on_the_route(name):
    import torch
    s = cases.scene(name)
    per = s["sensor"].perspective
    poses = np.array(s["poses"])
    pl = sensor(s, max_scans=70)
    pl.laser_set_cloud(s["cloud"])
    pl.laser_scan(poses)
    got = pl.laser_results()
    ref = [scan_bits(got, k, per) for k in range(len(poses))]
    for k, want in enumerate(cases.expected(name)):                       # the reference of this test is itself the oracle's
        assert got["n_points"][k] == want.count
    # permuted
    perm = np.random.default_rng(1).permutation(len(poses))
    pl.laser_scan(poses[perm])
    got = pl.laser_results()
    assert [scan_bits(got, j, per) for j in range(len(poses))] == [ref[k] for k in perm]
    # 1, 3 and 70 scans per call
    for n in (1, 3, 70):
        which = np.arange(n) % len(poses) if n > 1 else np.array([4])
        pl.laser_scan(poses[which])
        got = pl.laser_results(n)
        assert [scan_bits(got, j, per) for j in range(n)] == [ref[k] for k in which], n
    # device poses at strides 24 and 32, on a stream
    st = torch.cuda.Stream()
    for width in (3, 4):
        d = torch.zeros((len(poses), width), dtype=torch.float64, device="cuda")
        d[:, :3] = torch.from_numpy(poses).cuda()
        torch.cuda.synchronize()
        pl.laser_scan(d, stream=st)
        got = pl.laser_results()
        assert [scan_bits(got, k, per) for k in range(len(poses))] == ref, width
    # point strides 12 and 16, host and device
    four = np.concatenate([s["cloud"], np.full((len(s["cloud"]), 1), 7.0, np.float32)], 1)
    for cloud in (four, torch.from_numpy(four).cuda(), torch.from_numpy(np.array(s["cloud"])).cuda()):
        torch.cuda.synchronize()
        pl.laser_set_cloud(cloud, stream=st)
        pl.laser_scan(d, stream=st)
        got = pl.laser_results()
        assert [scan_bits(got, k, per) for k in range(len(poses))] == ref


@pytest.mark.parametrize("perspective", [0, 1])
def test_scan_then_map_integrate_in_stream_order(perspective):
    """pose -> scan -> map on one stream without a host wait; then the map equals tests/occupancy_cases.py run on the fetched
    world slab with its NaN rows dropped, bit for bit: stream order and the NaN convention against the existing oracle"""
    import torch
    s = cases.scene("room16")
    poses = np.array([cases.POSES[0], cases.POSES[5]])
    pl = sensor(s, max_scans=2)
    nx, ny, lo_x, lo_y, res, rng = 100, 80, -5.0, -4.0, 0.1, 3.0
    pl.map_create(nx, ny, lo_x, lo_y, res, detection_range=rng, perspective=perspective)
    st = torch.cuda.Stream()
    d_cloud, d_poses = torch.from_numpy(np.array(s["cloud"])).cuda(), torch.from_numpy(poses).cuda()
    view = pl.laser_device_view()
    slots = view["world_points"].shape[1]
    assert slots == 360 * 16 and view["world_points"].stride(0) == slots * 3
    torch.cuda.synchronize()
    pl.laser_set_cloud(d_cloud, stream=st)
    pl.laser_scan(d_poses, stream=st)
    pl.map_integrate([(view["world_points"][k], tuple(poses[k])) for k in range(2)], update_esdf=True, stream=st)
    got = pl.laser_results(2)                                             # waits
    state = pl.map_state()
    for k, want in enumerate(cases.expected("room16")[i] for i in (0, 5)):
        range_equals_oracle(got, k, want, ("chain", k))
    m = occ.OracleMap(nx, ny, lo_x, lo_y, res, pl.map_logodds, rng, bool(perspective))
    for k in range(2):
        rows = got["world_points"][k]
        rows = rows[~np.isnan(rows).any(1)]
        assert 0 < len(rows) == got["n_points"][k] < slots
        m.integrate(rows, tuple(poses[k]))
    assert (state["grid"] == m.grid).all() and (state["grid"] == occ.OCCUPIED).sum() > 20
    assert (state["log_odds"] == m.log_odds).all()


BAD_PARAMS = [dict(vtc_laser_line_num=1), dict(hrz_laser_line_num=0), dict(hrz_laser_line_num=513, vtc_laser_line_num=16),
              dict(sensing_horizon=0.0), dict(sensing_horizon=-1.0), dict(sensing_horizon=float("nan")), dict(pc_resolution=0.0),
              dict(vtc_laser_range_dgr=0.0), dict(vtc_laser_range_dgr=180.0)]


def test_refused_parameters_and_calls_out_of_order():
    from alore_legged_manipulator_amd.backend import BackendError
    pl = planner()
    pose = np.array([cases.POSES[0]])
    with pytest.raises(BackendError, match="error -1"):
        pl.laser_set_cloud(cases.cloud("one"))                            # before laser_create
    with pytest.raises(BackendError, match="error -1"):
        pl.laser_scan(pose)
    for bad in BAD_PARAMS:
        with pytest.raises(BackendError, match="error -1"):
            pl.laser_create(2, 16, **bad)
    with pytest.raises(BackendError, match="error -1"):
        pl.laser_create(0, 16)
    with pytest.raises(BackendError, match="error -1"):
        pl.laser_create(2, 0)                                             # perspective mode needs a capacity
    with pytest.raises(BackendError, match="error -1"):
        pl.laser_scan(pose)                                               # none of them left a sensor behind
    pl.laser_create(2, 16, hrz_laser_line_num=512, vtc_laser_line_num=16, if_perspective=0)   # 8192 bins: the largest image
    with pytest.raises(BackendError, match="error -1"):
        pl.laser_scan(pose)                                               # before laser_set_cloud
    pl.laser_set_cloud(cases.cloud("one"))
    with pytest.raises(BackendError, match="error -1"):
        pl.laser_scan(np.array([cases.POSES[0]] * 3))                     # count > max_scans
    with pytest.raises(BackendError, match="error -1"):
        pl.laser_scan(0x1000, count=1, pose_stride_bytes=20)              # a stride that is no multiple of 8
    pl.laser_scan(np.array(cases.POSES[:2]))
    got = pl.laser_results()
    assert got["range_image"].shape == (2, 512, 16) and (got["status"] == 0).all() and (got["n_points"] == 1).all()
    assert ((got["range_image"] < cases.EMPTY).sum((1, 2)) == 1).all()
