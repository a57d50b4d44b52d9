"""Oracle, scenes and input guard of the laser-scan tests (test_laser_scan_cpu.py, test_laser_scan_gpu.py).

The oracle restates, in plain Python floats (IEEE double, no fused multiply-add) and in the reference's own shape, what the laser
simulator publishes at a sensing tick (planning_ddr_opt/utils/laser_simulator/src/laser_sim_node.cpp): pt2LaserIdx (:113-142) for the
yaw-only pose of rcvOdometryCallbck, renderSensedPoints (:423-533) as a loop over points into a dis_map array with the spread of the
resolution filter written as the reference's two loops (up to three turns round the ring, no clamp), idx2Pt (:152-160),
perspectivePoints (:343-421), and the transform of the published floats into the world frame (sdf_map.cpp:12-30).  It is sequential
and scalar: the kernel's shape (atomic minima on bit patterns, ballots, a prefix sum) is not restated here.  math.atan2 / sin / cos /
sqrt / floor call the same libm as the g++ harness; float32 points are widened to double exactly as csrc/laser_scan.h does it.  The
deviations of that header are the oracle's too: in range on the double sum, non-finite points skipped, a point at the sensor skipped
in range mode, the filter's counts clamped before the cast.  The oracle is unpinned (the node needs ROS, PCL and TF to build).

guard() is a condition on the INPUTS, not a tolerance: a device atan2 / sin / cos a few units in the last place off glibc's moves an
angle by about 1e-15, i.e. about 1e-13 of a bin at a resolution of 0.0175 rad; the guard keeps every angle 1e-9 of a bin from a bin
edge and 1e-9 rad from a cut-off, four orders of margin, so the bin of every point is the same on both sides."""
import math

import numpy as np

OK, E_POSE, E_CAPACITY = 0, -1, -2
EMPTY = 9999.0
GUARD = 1e-9

DEFAULTS = dict(sensing_horizon=27.0, pc_resolution=0.1, hrz_laser_line_num=360, vtc_laser_line_num=16, vtc_laser_range_dgr=30.0,
                hrz_limited=0, hrz_laser_range_dgr=90.0, use_resolution_filter=0, if_perspective=1)
FIELDS = tuple(DEFAULTS)


class Sensor:
    """the node's parameters and the quantities main() derives from them (:554-564)"""

    def __init__(self, **kw):
        p = dict(DEFAULTS, **kw)
        self.p = p
        self.horizon, self.pc_resolution = float(p["sensing_horizon"]), float(p["pc_resolution"])
        self.hrz, self.vtc = int(p["hrz_laser_line_num"]), int(p["vtc_laser_line_num"])
        self.hrz_limited, self.filter, self.perspective = bool(p["hrz_limited"]), bool(p["use_resolution_filter"]), bool(p["if_perspective"])
        self.vtc_range_rad = p["vtc_laser_range_dgr"] / 180.0 * math.pi
        self.vtc_res = self.vtc_range_rad / float(self.vtc - 1)
        self.half_vtc = (self.vtc_range_rad + self.vtc_res) / 2.0
        self.half_hrz = p["hrz_laser_range_dgr"] / 180.0 * math.pi / 2.0
        self.hrz_res = 2 * math.pi / float(self.hrz)


def seen(S, pt, pose, c, s):
    """the offsets of a float32 point from the sensor: (in range, dx, dy, dz, dis, vtc_rad, hrz_rad); angles only in range"""
    px, py, pz = float(pt[0]), float(pt[1]), float(pt[2])
    if not (math.isfinite(px) and math.isfinite(py) and math.isfinite(pz)):
        return False, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
    dx, dy, dz = px - pose[0], py - pose[1], pz
    d2 = dx * dx + dy * dy + dz * dz
    if not d2 <= S.horizon * S.horizon:
        return False, dx, dy, dz, 0.0, 0.0, 0.0
    dis = math.sqrt(d2)
    vtc_rad = math.atan2(dz, math.sqrt(dx * dx + dy * dy))
    hrz_rad = math.atan2(-dx * s + dy * c, dx * c + dy * s)
    return True, dx, dy, dz, dis, vtc_rad, hrz_rad


def pt2laser_idx(S, vtc_rad, hrz_rad):
    if abs(vtc_rad) >= S.half_vtc:
        return None
    if S.hrz_limited and abs(hrz_rad) >= S.half_hrz:
        return None
    vtc_rad += S.half_vtc
    vtc_idx = math.floor(vtc_rad / S.vtc_res)
    if vtc_idx >= S.vtc:
        vtc_idx = 0
    hrz_rad += math.pi + S.hrz_res / 2.0
    hrz_idx = math.floor(hrz_rad / S.hrz_res)
    if hrz_idx >= S.hrz:
        hrz_idx = 0
    return hrz_idx, vtc_idx


def idx2pt(S, x, y, dis):
    vtc_rad = y * S.vtc_res - S.vtc_range_rad / 2.0
    hrz_rad = x * S.hrz_res - math.pi
    z = math.sin(vtc_rad) * dis
    xy = math.cos(vtc_rad) * dis
    return math.cos(hrz_rad) * xy, math.sin(hrz_rad) * xy, z


def occ_grid_num(S, mesh_len, line_num):
    q = S.pc_resolution / mesh_len if mesh_len != 0.0 else math.inf
    return int(math.floor(q)) if q < line_num else line_num       # min(floor(q), line_num), taken in double before the cast


class Result:
    pass


def nan3(n):
    return np.full((n, 3), np.nan, np.float32)


def render(S, cloud, pose, capacity=0):
    """one scan of the sensor S at pose (x, y, yaw) over the float32 cloud [n][3]: what csrc/laser_scan.h calls the outputs"""
    r = Result()
    bins = S.hrz * S.vtc
    slots = capacity if S.perspective else bins
    r.status, r.count = OK, 0
    r.image = None if S.perspective else np.full((S.hrz, S.vtc), EMPTY)
    r.laser, r.world, r.index = nan3(slots), nan3(slots), np.full(slots, -1, np.int32)
    r.compact = r.laser if S.perspective else nan3(slots)
    r.in_range = []                                                 # (point index, dis, bin or None) of the points in range
    if not all(math.isfinite(v) for v in pose[:3]):
        r.status = E_POSE
        return r
    c, s = math.cos(pose[2]), math.sin(pose[2])
    if S.perspective:
        laser, world, index = [], [], []
        for i, pt in enumerate(cloud):
            ok, dx, dy, dz, dis, _, _ = seen(S, pt, pose, c, s)
            if not ok:
                continue
            r.in_range.append((i, dis, None))
            laser.append((dx * c + dy * s, -dx * s + dy * c, dz))   # rot^T (pt - t)
            world.append(pt)
            index.append(i)
        r.count = len(index)
        r.all_laser, r.all_world = np.array(laser, np.float64).astype(np.float32).reshape(-1, 3), np.array(world, np.float32).reshape(-1, 3)
        r.all_index = np.array(index, np.int32)
        if r.count > capacity:
            r.status = E_CAPACITY
        else:
            r.laser[:r.count], r.world[:r.count], r.index[:r.count] = r.all_laser, r.all_world, r.all_index
        return r
    dis_map = r.image
    idx_map = np.full((S.hrz, S.vtc), -1, np.int64)
    for i, pt in enumerate(cloud):
        ok, dx, dy, dz, dis, vtc_rad, hrz_rad = seen(S, pt, pose, c, s)
        if not ok:
            continue
        if not dis > 0.0:
            r.in_range.append((i, dis, None))
            continue
        idx = pt2laser_idx(S, vtc_rad, hrz_rad)
        r.in_range.append((i, dis, idx))
        if idx is None:
            continue
        if S.filter:
            line_rad = idx[1] * S.vtc_res - S.vtc_range_rad / 2.0
            dis_to_z_axis = dis * math.cos(line_rad)
            tmp1 = occ_grid_num(S, dis_to_z_axis * S.hrz_res, S.hrz)
            tmp2 = occ_grid_num(S, dis_to_z_axis * S.vtc_res, S.vtc)
            for d_hrz in range(-tmp1, tmp1 + 1):
                for d_vtc in range(-tmp2, tmp2 + 1):
                    hrz_idx = (idx[0] + d_hrz + S.hrz) % S.hrz
                    vtc_idx = idx[1] + d_vtc
                    if vtc_idx >= S.vtc or vtc_idx < 0:
                        continue
                    if dis < dis_map[hrz_idx, vtc_idx]:
                        idx_map[hrz_idx, vtc_idx] = i
                        dis_map[hrz_idx, vtc_idx] = dis
        elif dis < dis_map[idx]:
            idx_map[idx] = i
            dis_map[idx] = dis
    k = 0
    for x in range(S.hrz):
        for y in range(S.vtc):
            if idx_map[x, y] == -1:
                continue
            p = idx2pt(S, x, y, float(dis_map[x, y]))
            b = x * S.vtc + y
            r.laser[b] = p                                          # the floats of the published cloud
            fx, fy = float(r.laser[b, 0]), float(r.laser[b, 1])
            r.world[b] = (pose[0] + c * fx - s * fy, pose[1] + s * fx + c * fy, float(r.laser[b, 2]))
            r.compact[k], r.index[k] = r.laser[b], b
            k += 1
    r.count = k
    return r


# ---- the scenes ------------------------------------------------------------------------------------------------------------------
HORIZON = 6.0
R16 = dict(sensing_horizon=HORIZON, if_perspective=0)                                                     # 360 x 16, no filter
R2F = dict(sensing_horizon=HORIZON, if_perspective=0, vtc_laser_line_num=2, vtc_laser_range_dgr=10.0, use_resolution_filter=1)
TINY = dict(sensing_horizon=HORIZON, if_perspective=0, hrz_laser_line_num=8, vtc_laser_line_num=2, vtc_laser_range_dgr=40.0,
            use_resolution_filter=1, pc_resolution=2.0)                                                   # every spread wraps
LIMITED = dict(R16, hrz_limited=1)
LIMITED2F = dict(R2F, hrz_limited=1, hrz_laser_range_dgr=200.0)
PERSPECTIVE = dict(sensing_horizon=HORIZON)

# positions are float32-exact, so that a cloud point can sit exactly at a sensor; yaws: 0, +-pi, near +-pi/2, and one more
POSES = [(0.5, -0.25, 0.0), (0.5, -0.25, math.pi), (-1.25, 0.75, -math.pi), (1.0, 0.5, 1.5707), (-1.25, 0.75, -1.5709), (1.0, 0.5, 0.7)]
# a point at z = 0 is in the sensor's plane: with an even number of vertical lines that is a bin edge, which the guard forbids for
# every point it can see, so the point at the sensor comes with poses at its own position only
AT_SENSOR_POSES = [(0.5, -0.25, 0.0), (0.5, -0.25, math.pi), (0.5, -0.25, 0.7)]
BAD_POSES = [POSES[0], (0.5, float("nan"), 0.0), POSES[5], (float("inf"), 0.0, 0.3), (1.0, 0.5, float("nan")), POSES[3]]


def column(x, y, heights):
    return [(x, y, z) for z in heights]


def room(seed):
    """walls of a room of about 8 m x 6 m as columns of four heights, three pillars of six heights near the middle (they occlude
    the walls behind them), every position jittered by the seed; some columns twice (equal distances in one bin)"""
    rng = np.random.default_rng(seed)
    pts = []
    wall_z, pillar_z = (0.05, 0.35, 0.65, 1.15), (0.03, 0.13, 0.23, 0.33, 0.43, 0.53)
    xs, ys = np.arange(-4.0, 4.0001, 0.1), np.arange(-3.0, 3.0001, 0.1)
    for x in xs:
        for y in (-3.0, 3.0):
            pts += column(x + rng.uniform(-0.02, 0.02), y + rng.uniform(-0.02, 0.02), wall_z)
    for y in ys[1:-1]:
        for x in (-4.0, 4.0):
            pts += column(x + rng.uniform(-0.02, 0.02), y + rng.uniform(-0.02, 0.02), wall_z)
    for cx, cy in ((1.9, 0.3), (-0.4, -1.6), (-2.3, 1.4)):
        for a in np.linspace(0.0, 2 * math.pi, 8, endpoint=False):
            pts += column(cx + 0.15 * math.cos(a) + rng.uniform(-0.01, 0.01), cy + 0.15 * math.sin(a) + rng.uniform(-0.01, 0.01), pillar_z)
    pts += pts[40:60] + pts[-30:-20]                                 # ties
    return pts


def specials(seed):
    """what the contract treats specially, for every pose: points beyond the horizon, non-finite coordinates, points just either side of the +-pi seam of every yaw, points above and below the vertical range, and points
    so close that the filter's spread covers the whole ring"""
    rng = np.random.default_rng(seed)
    pts = [(float("nan"), 0.5, 0.1), (0.3, float("nan"), 0.1), (0.2, 0.1, float("nan")), (float("inf"), 0.0, 0.1), (0.1, float("-inf"), 0.2)]
    for a in rng.uniform(-math.pi, math.pi, 24):
        r = rng.uniform(6.6, 9.5)
        pts.append((r * math.cos(a), r * math.sin(a), rng.uniform(0.02, 0.5)))
    for x, y, yaw in POSES:
        for da in (-0.0011, 0.0013):                                 # behind the sensor, either side of the seam
            a = yaw + math.pi + da
            pts.append((x + 2.1 * math.cos(a), y + 2.1 * math.sin(a), 0.07))
        a = yaw + rng.uniform(0.2, 0.9)
        pts.append((x + 1.0 * math.cos(a), y + 1.0 * math.sin(a), 1.23))     # above every vertical range used here
        pts.append((x + 1.1 * math.cos(a), y + 1.1 * math.sin(a), -1.37))    # below
        pts.append((x + 1.2 * math.cos(a), y + 1.2 * math.sin(a), -0.05))    # below the plane, in range
        a = yaw + rng.uniform(-2.0, 2.0)
        pts.append((x + 0.031 * math.cos(a), y + 0.031 * math.sin(a), 0.0021))  # the spread goes round the ring
    return pts


def shell(n, seed):
    rng = np.random.default_rng(seed)
    a, r = rng.uniform(-math.pi, math.pi, n), rng.uniform(0.5, 7.0, n)
    return np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-0.6, 0.9, n)], 1)


SEED = 5
_clouds = {}


def cloud(name):
    if name not in _clouds:
        if name == "empty":
            c = np.zeros((0, 3), np.float32)
        elif name == "one":
            c = np.array([[2.3, 0.9, 0.21]], np.float32)
        elif name == "n257":
            c = shell(257, SEED).astype(np.float32)                  # one more than a workgroup is wide
        elif name == "at_sensor":                                    # dis == 0 for the poses of AT_SENSOR_POSES
            c = np.concatenate([shell(257, SEED), np.array([[0.5, -0.25, 0.0]])]).astype(np.float32)
        elif name == "room":
            rng = np.random.default_rng(SEED + 1)
            c = np.array(room(SEED + 2) + specials(SEED + 3), np.float32)
            c = c[rng.permutation(len(c))]
        else:
            raise KeyError(name)
        c.setflags(write=False)
        _clouds[name] = c
    return _clouds[name]


PERSPECTIVE_FITS, PERSPECTIVE_OVERFLOWS = 2048, 96
# name: (parameters, cloud, poses, capacity of a perspective scan)
SCENES = {
    "empty": (R16, "empty", POSES[:2], 0),
    "one": (R16, "one", POSES, 0),
    "n257": (R16, "n257", POSES, 0),
    "room16": (R16, "room", POSES, 0),
    "room2f": (R2F, "room", POSES, 0),
    "tiny": (TINY, "room", POSES, 0),
    "limited": (LIMITED, "room", POSES, 0),
    "limited2f": (LIMITED2F, "room", POSES, 0),
    "n257_filter": (R2F, "n257", POSES, 0),
    "at_sensor": (R16, "at_sensor", AT_SENSOR_POSES, 0),
    "at_sensor_filter": (R2F, "at_sensor", AT_SENSOR_POSES, 0),
    "bad_pose": (R16, "n257", BAD_POSES, 0),
    "perspective_empty": (PERSPECTIVE, "empty", POSES[:2], 16),
    "perspective_fits": (PERSPECTIVE, "room", POSES, PERSPECTIVE_FITS),
    "perspective_overflows": (PERSPECTIVE, "room", POSES, PERSPECTIVE_OVERFLOWS),
    "perspective_at_sensor": (PERSPECTIVE, "at_sensor", AT_SENSOR_POSES, 300),
    "perspective_bad_pose": (PERSPECTIVE, "n257", BAD_POSES, 300),
}
RANGE_SCENES = tuple(n for n, s in SCENES.items() if not Sensor(**s[0]).perspective)
PERSPECTIVE_SCENES = tuple(n for n in SCENES if n not in RANGE_SCENES)
_expected = {}


def scene(name):
    prm, cl, poses, cap = SCENES[name]
    return dict(params=dict(DEFAULTS, **prm), sensor=Sensor(**prm), cloud=cloud(cl), poses=list(poses), capacity=cap)


def expected(name):
    """[Result] per pose of the scene, computed once and shared; the arrays are read-only"""
    if name not in _expected:
        s = scene(name)
        out = []
        for pose in s["poses"]:
            r = render(s["sensor"], s["cloud"], pose, s["capacity"])
            for a in (r.image, r.laser, r.world, r.index, r.compact):
                if a is not None:
                    a.setflags(write=False)
            out.append(r)
        _expected[name] = out
    return _expected[name]


def away_from_integer(v):
    return abs(v - round(v))


def guard(name):
    """asserts, for every point in range of every pose of the scene, that no decision of the contract is within reach of a
    rounding difference in atan2, sin or cos; returns the number of points it looked at"""
    s = scene(name)
    S, looked = s["sensor"], 0
    for pose in s["poses"]:
        if not all(math.isfinite(v) for v in pose):
            continue
        c, sn = math.cos(pose[2]), math.sin(pose[2])
        for i, pt in enumerate(s["cloud"]):
            px, py, pz = float(pt[0]), float(pt[1]), float(pt[2])
            if not (math.isfinite(px) and math.isfinite(py) and math.isfinite(pz)):
                continue
            dx, dy = px - pose[0], py - pose[1]
            d2, h2 = dx * dx + dy * dy + pz * pz, S.horizon * S.horizon
            assert abs(d2 - h2) > GUARD * h2, (name, pose, i, "horizon")
            ok, _, _, _, dis, vtc_rad, hrz_rad = seen(S, pt, pose, c, sn)
            if not ok or not dis > 0.0:
                continue
            looked += 1
            assert away_from_integer((vtc_rad + S.half_vtc) / S.vtc_res) >= GUARD, (name, pose, i, "vtc bin")
            assert away_from_integer((hrz_rad + (math.pi + S.hrz_res / 2.0)) / S.hrz_res) >= GUARD, (name, pose, i, "hrz bin")
            assert abs(abs(vtc_rad) - S.half_vtc) >= GUARD, (name, pose, i, "vtc cut-off")
            if S.hrz_limited:
                assert abs(abs(hrz_rad) - S.half_hrz) >= GUARD, (name, pose, i, "hrz cut-off")
    return looked
