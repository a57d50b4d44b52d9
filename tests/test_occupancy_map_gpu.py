"""The resident occupancy map on the GPU (alore_backend_map_*): point clouds in, log-odds, cell states and the ESDF updated in
place on the device, against the sequential oracle of tests/occupancy_cases.py.

State grid and log-odds are compared for EQUALITY after every scan: every operation that decides a cell is a correctly rounded
double operation or an integer operation, contraction is off in csrc/occupancy_update.h, and the oracle takes the five log-odds
from the library (map_logodds), so no second `log` is involved.  The counts are read from the device view and must be zero
between scans.  The distance field is compared, bit for bit, with what build_esdf gives for the fetched state grid.

Shapes: a 64 x 48 map (an x / y stride swap shows) at 0.1 m from (-3.2, -2.4), range 2.0; scans of about 300 points (more than one
workgroup of 256); one scan of 5000 points on 160 x 160 at range 6.0 (20 workgroups, a few thousand cells with counts); one scan
of 40004 points on the small map that sends more than 32767 rays through eight cells (where a short count would wrap)."""
import ctypes as C

import numpy as np
import pytest

from tests import occupancy_cases as cases

pytestmark = pytest.mark.gpu


def planner(n=1):
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    return BatchedMSPlanner(n, 16)


def create(pl, s):
    pl.map_create(s["nx"], s["ny"], s["x_lo"], s["y_lo"], s["res"], detection_range=s["range"], perspective=int(s["perspective"]))
    if s["seed"] is not None:
        pl.map_set_grid(s["seed"])
    return pl.map_logodds


def _hip_runtime():
    """the HIP runtime this process already runs on (the one torch loaded)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def counts(pl):
    import torch  # noqa: F401  (loads the HIP runtime)
    hip = _hip_runtime()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    v = pl.map_device()
    out = []
    for ptr in (v.count_hit, v.count_all):
        a = np.full((v.nx, v.ny), -1, np.int32)
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemcpy(a.ctypes.data, ptr, a.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        out.append(a)
    return out


def same(st, exp, what):
    g, lo = exp
    assert np.array_equal(st["grid"], g), (what, "grid", np.argwhere(st["grid"] != g)[:8])
    assert np.array_equal(st["log_odds"], lo), (what, "log_odds", np.argwhere(st["log_odds"] != lo)[:8])


def run_scenario(name, device=False, stride_floats=2):
    """the states after every scan of the scenario, one map_integrate per scan"""
    import torch
    s = cases.scenario(name)
    pl = planner()
    L5 = create(pl, s)
    states = []
    for pts, pose in s["scans"]:
        q = np.full((len(pts), stride_floats), np.nan, np.float32)   # the padding is never read
        q[:, :2] = pts
        pl.map_integrate([(torch.from_numpy(q).cuda() if device else q, pose)], update_esdf=False)
        states.append(pl.map_state())
    return pl, L5, states


# ---- 1, 8 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["raycast", "large"])
def test_raycast_scans_equal_the_oracle(name):
    s = cases.scenario(name)
    pl = planner()
    L5 = create(pl, s)
    exp = cases.expected(name, L5)
    for k, (pts, pose) in enumerate(s["scans"]):
        pl.map_integrate([(pts, pose)], update_esdf=False)
        same(pl.map_state(), exp[k], (name, k))
        hit, total = counts(pl)
        assert not hit.any() and not total.any(), (name, k)
    assert (exp[-1][0] == 2).any() and (exp[-1][0] == 1).sum() > 100


def test_counts_do_not_wrap_where_a_short_would():
    """the deviation "int counts": 40003 valid points in one scan.  The sensor's cell and the first cells of the fan see more than
    32767 rays; the reference's short totals wrap negative there and make each a hit (tests/test_occupancy_cpu.py shows that on
    the rule).  With exact counts each is a miss: clamp_min, Unoccupied, and the whole map equals the int oracle.  The
    wave-aggregated atomics add up to 40003 here, far beyond the 200 of the other scans."""
    s = cases.scenario("crowded")
    pl = planner()
    L5 = create(pl, s)
    pts, pose = s["scans"][0]
    pl.map_integrate([(pts, pose)], update_esdf=False)
    st = pl.map_state()
    same(st, cases.expected("crowded", L5)[0], "crowded")
    hit, total = counts(pl)
    assert not hit.any() and not total.any()
    seen = cases.totals("crowded", L5)[0]
    crowded = [tuple(c) for c in np.argwhere(seen > 32767)]
    sensor = cases.new_oracle(s, L5).index(*pose[:2])
    assert seen[sensor] == 40003 and sensor in crowded and len(crowded) >= 4
    for c in crowded:
        assert cases.as_short(seen[c]) < 0
        assert st["log_odds"][c] == L5[2] and st["grid"][c] == 1, c           # a hit would give clamp_max and Occupied
    assert (st["log_odds"] == L5[3]).any() and (st["grid"] == 2).any()        # the wall itself is hit


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
def test_state_rule():
    pl, L5, st = run_scenario("state_rule", stride_floats=3)
    exp = cases.expected("state_rule", L5)
    for k in range(4):
        same(st[k], exp[k], k)
    s = cases.scenario("state_rule")
    m = cases.new_oracle(s, L5)
    cell = m.index(*[float(v) for v in s["scans"][0][0][0]])
    free = m.line(m.index(*s["scans"][0][1][:2]), cell)[1]
    assert st[0]["grid"][cell] == 2 and st[0]["log_odds"][cell] == L5[3]
    assert st[1]["log_odds"][cell] == L5[3]                                   # a hit at clamp_max changes nothing
    assert st[0]["log_odds"][free] == L5[2] and st[1]["log_odds"][free] == L5[2]   # a miss at or below clamp_min: clamp_min exactly
    assert st[3]["log_odds"][cell] < L5[4] and st[3]["grid"][cell] == 2       # misses only: below the p_occ logit, still Occupied


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
def test_remove_outliers_on_a_seeded_grid():
    pl, L5, st = run_scenario("outliers")
    exp = cases.expected("outliers", L5)
    for k in range(4):
        same(st[k], exp[k], k)
    after_skip, after_centre, after_near, after_in = (s["grid"] for s in st)
    # the lattice of SKIP_POSE by repeated addition never enters column 8 (start + i * res does: pinned on the CPU in
    # test_occupancy_cpu.py::test_remove_outliers_properties); the control hole two columns on is filled
    assert after_skip[cases.SKIP_HOLE] == 0 and after_skip[cases.CONTROL_HOLE] == 1
    assert after_centre[cases.SINGLE_HOLE] == 1 and all(after_centre[c] == 0 for c in cases.PAIR_HOLES)
    assert after_near[cases.RING_CELL] == 0 and (after_near[0:3, 23:26] == 1).all() and (after_centre[0:3, 23:26] == 0).all()
    assert (after_in[0:2, 33:36] == 1).all() and (after_near[0:2, 33:36] == 0).all()


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
def test_perspective_mode():
    pl, L5, st = run_scenario("perspective", stride_floats=4)
    exp = cases.expected("perspective", L5)
    s = cases.scenario("perspective")
    m = cases.new_oracle(s, L5)
    for k, (pts, pose) in enumerate(s["scans"]):
        same(st[k], exp[k], k)
        far = pts[20]
        assert np.hypot(far[0] - pose[0], far[1] - pose[1]) > m.range and m.in_map(float(far[0]), float(far[1]))
        assert st[k]["grid"][m.index(float(far[0]), float(far[1]))] == 2          # beyond the range, inside the map
        mn, mx = m.window(pose[:2])
        box = st[k]["grid"][mn[0]:mx[0] + 1, mn[1]:mx[1] + 1]
        assert (box != 0).all() and (box == 1).sum() > 1000
    assert (st[-1]["grid"] == 2).sum() == (exp[-1][0] == 2).sum() >= 10


# ---- 5 ----------------------------------------------------------------------------------------------------------------------
def test_resident_esdf_is_build_esdf_of_the_fetched_grid():
    s = cases.scenario("raycast")
    pl, ref = planner(), planner()
    create(pl, s)
    (p0, o0), (p1, o1) = s["scans"][0], s["scans"][1]
    pl.map_integrate([(p0, o0)], update_esdf=True)
    st0 = pl.map_state()
    d0 = ref.build_esdf(st0["grid"], s["x_lo"], s["y_lo"], s["res"], o0[:2], s["range"])
    assert np.array_equal(st0["dist"], d0)
    finite0 = d0 < 1e300
    assert finite0.any() and not finite0.all()
    pl.map_integrate([(p1, o1)], update_esdf=True)
    st1 = pl.map_state()
    d1 = ref.build_esdf(st1["grid"], s["x_lo"], s["y_lo"], s["res"], o1[:2], s["range"])
    assert np.array_equal(st1["dist"], d1)
    changed = st1["dist"] != d0
    kept = finite0 & ~changed
    assert changed.any() and kept.any()                         # cells outside the second window keep the first scan's values
    # the ESDF alone, in a window of the caller's choice
    pl.map_update_esdf(o0[:2], 1.0)
    d2 = ref.build_esdf(st1["grid"], s["x_lo"], s["y_lo"], s["res"], o0[:2], 1.0)
    assert np.array_equal(pl.map_state()["dist"], d2)


def test_update_esdf_on_another_stream_follows_the_integrate():
    """map_integrate and map_update_esdf share one ESDF workspace: a map_update_esdf issued on a second stream right after a
    map_integrate of several scans on a first one waits for it on the device and gives the field of the two run one after the other"""
    import torch
    s = cases.scenario("raycast")
    (p0, o0), (p1, o1) = s["scans"][0], s["scans"][1]
    pl, ref = planner(), planner()
    create(pl, s)
    create(ref, s)
    d0, d1 = torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda()
    st1, st2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    pl.map_integrate([(d0, o0), (d1, o1), (d0, o0), (d1, o1)], update_esdf=True, stream=st1)
    pl.map_update_esdf(o0[:2], 1.0, stream=st2)
    pl.map_integrate([(d1, o1)], update_esdf=True, stream=st1)                # ... and waits for the ESDF on st2 in turn
    got = pl.map_state()                                                      # waits for the device
    for sc in ((p0, o0), (p1, o1), (p0, o0), (p1, o1)):
        ref.map_integrate([sc], update_esdf=True)
    ref.map_update_esdf(o0[:2], 1.0)
    ref.map_integrate([(p1, o1)], update_esdf=True)
    exp = ref.map_state()
    assert all(np.array_equal(got[k], exp[k]) for k in exp)


# ---- 6 ----------------------------------------------------------------------------------------------------------------------
def test_device_points_give_the_bits_of_the_host_route():
    _, L5, host = run_scenario("raycast")
    _, _, dev = run_scenario("raycast", device=True, stride_floats=4)
    for k, (a, b) in enumerate(zip(host, dev)):
        for key in ("grid", "log_odds"):
            assert np.array_equal(a[key], b[key]), (k, key)


def test_integrate_then_check_plans_on_one_stream():
    """a small planned batch, then an obstacle integrated across the plans: map_integrate and check_plans(fetch=False) on one
    non-default stream, fetched afterwards, against the same sequence with host arrays and fetch=True on a second planner"""
    import torch
    from alore_legged_manipulator_amd.backend import CHECK_DTYPE
    from alore_legged_manipulator_amd.flat_traj import straight_goal
    s = cases.scenario("raycast")
    fts = [straight_goal((-1.5, y, 0.0), (1.5, y, 0.0)) for y in (-1.0, -0.3, 0.4, 1.1)]
    pose = cases.POSES[0]
    pts = np.full((40, 4), np.nan, np.float32)                              # a padded xyzw layout: 16 bytes per point
    pts[:, :2] = cases.wall((0.5, -0.6), (0.5, 0.7), 40)
    keys = ("collision", "first_panel", "n_checked", "first_time", "first_xy", "min_dist")
    got = []
    for device in (True, False):
        pl = planner(len(fts))
        pl.set_free_map(6.0)
        pl.minco_plan(fts)
        create(pl, s)
        if device:
            st = torch.cuda.Stream()
            d_pts = torch.from_numpy(pts).cuda()
            torch.cuda.synchronize()
            pl.map_integrate([(d_pts, pose)], update_esdf=True, stream=st)
            assert pl.check_plans(min_safe_dis=0.2, stream=st, fetch=False) is None
            st.synchronize()
            hip = _hip_runtime()
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            slab = np.zeros(len(fts), CHECK_DTYPE)
            assert hip.hipMemcpy(slab.ctypes.data, pl.device_check(), slab.nbytes, 2) == 0
            got.append({k: slab[k].copy() for k in keys})
        else:
            pl.map_integrate([(pts, pose)], update_esdf=True)
            got.append(pl.check_plans(min_safe_dis=0.2))
        got[-1]["dist"] = pl.map_state()["dist"]
    for k in keys + ("dist",):
        assert np.array_equal(got[0][k], got[1][k]), k
    assert list(got[1]["collision"]) == [0, 1, 1, 0]                        # the wall crosses the two middle lanes


# ---- 7 ----------------------------------------------------------------------------------------------------------------------
def test_contract():
    from alore_legged_manipulator_amd.backend import BackendError
    s = cases.scenario("raycast")
    pl = planner()
    L5 = create(pl, s)
    pts, pose = s["scans"][0]
    pl.map_integrate([(pts, pose)], update_esdf=False)
    before = pl.map_state()
    for bad in ((9.0, 0.0, 0.0), (s["x_lo"], 0.0, 0.0), (float("nan"), 0.0, 0.0)):
        with pytest.raises(BackendError, match="inside the map"):
            pl.map_integrate([(pts, cases.POSES[1]), (pts, bad)], update_esdf=True)   # refused before anything is enqueued
    after = pl.map_state()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    # n_points = 0: a cycle with no rays; RemoveOutliers and the window still run
    m = cases.new_oracle(s, L5)
    m.integrate(pts, pose)
    m.integrate(np.zeros((0, 2), np.float32), cases.POSES[1])
    pl.map_integrate([(np.zeros((0, 2), np.float32), cases.POSES[1])], update_esdf=False)
    same(pl.map_state(), (m.grid, m.log_odds), "no points")
    assert not np.array_equal(m.grid, before["grid"])
    with pytest.raises(BackendError, match="stride"):
        pl.map_integrate([((pl.map_device().grid, 4), pose)], point_stride_bytes=6)
    # set_map ends the resident map
    pl.set_map(np.full((s["nx"], s["ny"]), 100.0), s["x_lo"], s["y_lo"], s["res"])
    with pytest.raises(BackendError, match="no resident map"):
        pl.map_integrate([(pts, pose)])
    with pytest.raises(BackendError, match="no resident map"):
        pl.map_state()
    create(pl, s)                                                            # ... until the next map_create
    pl.map_integrate([(pts, pose)], update_esdf=False)
    same(pl.map_state(), cases.expected("raycast", L5)[0], "created again")
    pl.build_esdf(before["grid"], s["x_lo"], s["y_lo"], s["res"], pose[:2], s["range"])
    with pytest.raises(BackendError, match="no resident map"):
        pl.map_logodds
    with pytest.raises(BackendError, match="no resident map"):
        planner().map_integrate([(pts, pose)])
    with pytest.raises(BackendError, match="map_create"):
        planner().map_create(64, 48, 0.0, 0.0, 0.1, p_hit=1.0)


def test_several_scans_in_one_call_are_the_scans_one_by_one():
    """more scans than one upload of argument blocks holds (8): the chunks follow each other in stream order"""
    s = cases.scenario("raycast")
    scans = [s["scans"][k % 2] for k in range(11)]
    one, many = planner(), planner()
    create(one, s)
    create(many, s)
    for sc in scans:
        one.map_integrate([sc], update_esdf=True)
    many.map_integrate(scans, update_esdf=True)
    a, b = one.map_state(), many.map_state()
    assert all(np.array_equal(a[k], b[k]) for k in a)
