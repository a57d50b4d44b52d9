"""Oracle and scan generators of the occupancy-map tests (test_occupancy_cpu.py, test_occupancy_map_gpu.py).

OracleMap restates, in plain Python floats (IEEE double, no fused multiply-add) and in the reference's own shape, the half of
plan_env::SDFmap that runs before updateESDF2d (planning_ddr_opt/utils/plan_env/src/sdf_map.cpp): updateOccupancyCallback
(:35-130), raycastProcess (:132-175) with setCacheOccupancy and the queue of touched cells, updateOccupancyMap (:281-314),
RemoveOutliers (:316-350) as an in-place scan over the lattice points, getGridsBetweenPoints2D (:387-414), coord2gridIndex
(:467-472), isInGloMap and closetPointInMap (:591-614).  It is sequential and scalar: the kernels' shape (counts by atomics, marks
of visited columns and rows, passes over a box) is not restated here.  The five log-odds are an input: the library's own values.
The oracle is unpinned (plan_env needs ROS, PCL and Eigen to build).  The deviations of csrc/occupancy_update.h are the oracle's
too: the counts are int32 (they do not wrap at 32768 as the reference's shorts do), non-finite points are skipped, a sensor
outside the map is refused, and the outermost ring of the map is not filled."""
import math

import numpy as np

UNKNOWN, UNOCCUPIED, OCCUPIED = 0, 1, 2
UNKNOWN_FLAG = 0.01


class OracleMap:
    def __init__(self, nx, ny, x_lo, y_lo, res, log_odds5, detection_range, perspective=False):
        self.nx, self.ny, self.x_lo, self.y_lo, self.res = int(nx), int(ny), float(x_lo), float(y_lo), float(res)
        self.x_hi, self.y_hi = self.x_lo + self.nx * self.res, self.y_lo + self.ny * self.res
        self.inv = 1 / self.res
        self.l_hit, self.l_miss, self.l_min, self.l_max, self.l_occ = (float(v) for v in log_odds5)
        self.range = float(detection_range)
        self.perspective = bool(perspective)
        self.grid = np.zeros((self.nx, self.ny), np.uint8)
        self.log_odds = np.full((self.nx, self.ny), self.l_min - UNKNOWN_FLAG)
        self.count_hit = np.zeros((self.nx, self.ny), np.int32)
        self.count_all = np.zeros((self.nx, self.ny), np.int32)
        self.queue = []
        self.last_total = np.zeros((self.nx, self.ny), np.int64)   # count_all of the last raycast, before it was zeroed

    # ---- coordinates
    def index(self, x, y):
        ix = min(max(int((x - self.x_lo) * self.inv), 0), self.nx - 1)
        iy = min(max(int((y - self.y_lo) * self.inv), 0), self.ny - 1)
        return ix, iy

    def in_map(self, x, y):
        return x < self.x_hi and x > self.x_lo and y < self.y_hi and y > self.y_lo

    def closest_point_in_map(self, pt, pos):
        diff = (pt[0] - pos[0], pt[1] - pos[1])
        max_tc = (self.x_hi - pos[0], self.y_hi - pos[1])
        min_tc = (self.x_lo - pos[0], self.y_lo - pos[1])
        min_t = 1000000.0
        for i in range(2):
            if abs(diff[i]) > 0:
                t1 = max_tc[i] / diff[i]
                if 0 < t1 < min_t:
                    min_t = t1
                t2 = min_tc[i] / diff[i]
                if 0 < t2 < min_t:
                    min_t = t2
        t = min_t - 1e-3
        return pos[0] + t * diff[0], pos[1] + t * diff[1]

    def window(self, odom):
        half = math.ceil(self.range / self.res) * self.res
        self.x_lower, self.x_upper = max(odom[0] - half, self.x_lo), min(odom[0] + half, self.x_hi)
        self.y_lower, self.y_upper = max(odom[1] - half, self.y_lo), min(odom[1] + half, self.y_hi)
        return self.index(self.x_lower, self.y_lower), self.index(self.x_upper, self.y_upper)

    # ---- raycast
    def set_cache(self, idx, occ):
        self.count_all[idx] += 1
        if self.count_all[idx] == 1:
            self.queue.append(idx)
        if occ:
            self.count_hit[idx] += 1

    @staticmethod
    def line(start, end):
        out = []
        dx, dy = abs(end[0] - start[0]), abs(end[1] - start[1])
        sx = 1 if start[0] < end[0] else -1
        sy = 1 if start[1] < end[1] else -1
        err = dx - dy
        x0, y0 = start
        while True:
            out.append((x0, y0))
            if x0 == end[0] and y0 == end[1]:
                break
            e2 = 2 * err
            if e2 > -dy:
                err -= dy
                x0 += sx
            if e2 < dx:
                err += dx
                y0 += sy
        return out

    def clip(self, cur, odom, length):
        return ((cur[0] - odom[0]) / length * self.range + odom[0], (cur[1] - odom[1]) / length * self.range + odom[1])

    def raycast(self, points, odom):
        self.last_total[:] = 0
        for p in points:
            cur = (float(p[0]), float(p[1]))
            if not (math.isfinite(cur[0]) and math.isfinite(cur[1])):
                continue
            if not self.in_map(*cur):
                cur = self.closest_point_in_map(cur, odom)
                dx, dy = cur[0] - odom[0], cur[1] - odom[1]
                length = math.sqrt(dx * dx + dy * dy)
                if length > self.range:
                    cur = self.clip(cur, odom, length)
                self.set_cache(self.index(*cur), 0)
            else:
                dx, dy = cur[0] - odom[0], cur[1] - odom[1]
                length = math.sqrt(dx * dx + dy * dy)
                if length > self.range:
                    cur = self.clip(cur, odom, length)
                    self.set_cache(self.index(*cur), 0)
                else:
                    self.set_cache(self.index(*cur), 1)
            cells = self.line(self.index(*odom), self.index(*cur))
            for c in cells[:-1]:
                self.set_cache(c, 0)
        self.update_occupancy_map()

    def update_occupancy_map(self):
        mn, mx = self.index(self.x_lower, self.y_lower), self.index(self.x_upper, self.y_upper)
        while self.queue:
            idx = self.queue.pop(0)
            hit, total = int(self.count_hit[idx]), int(self.count_all[idx])
            update = self.l_hit if hit >= total - 3 * hit else self.l_miss
            self.count_hit[idx] = self.count_all[idx] = 0
            self.last_total[idx] = total
            if update >= 0 and self.log_odds[idx] >= self.l_max:
                continue
            elif update <= 0 and self.log_odds[idx] <= self.l_min:
                self.log_odds[idx] = self.l_min
                continue
            in_local = mn[0] <= idx[0] <= mx[0] and mn[1] <= idx[1] <= mx[1]
            if not in_local:
                self.log_odds[idx] = self.l_min
            self.log_odds[idx] = min(max(float(self.log_odds[idx]) + update, self.l_min), self.l_max)

    # ---- RemoveOutliers
    def lattice_row(self, o):
        out, v = [], o - self.range
        while v < o + self.range + 1e-10:
            out.append(v)
            v += self.res
        return out

    def remove_outliers(self, odom, rows=None):
        xs, ys = rows if rows is not None else (self.lattice_row(odom[0]), self.lattice_row(odom[1]))
        xlow, xup = self.x_lo + self.res, self.x_hi - self.res
        ylow, yup = self.y_lo + self.res, self.y_hi - self.res
        g = self.grid
        for x in xs:
            for y in ys:
                if x > xlow and x < xup and y > ylow and y < yup:
                    ix, iy = self.index(x, y)
                    if ix < 1 or iy < 1 or ix > self.nx - 2 or iy > self.ny - 2:
                        continue  # the reference would read outside the map
                    if g[ix, iy] == UNKNOWN and g[ix, iy + 1] == UNOCCUPIED and g[ix, iy - 1] == UNOCCUPIED and \
                            g[ix + 1, iy] == UNOCCUPIED and g[ix - 1, iy] == UNOCCUPIED:
                        g[ix, iy] = UNOCCUPIED
        ix, iy = self.index(*odom)
        for i in (-1, 0, 1):
            for j in (-1, 0, 1):
                if 0 <= ix + i < self.nx and 0 <= iy + j < self.ny and g[ix + i, iy + j] == UNKNOWN:
                    g[ix + i, iy + j] = UNOCCUPIED

    # ---- updateOccupancyCallback
    def integrate(self, points, odom):
        odom = (float(odom[0]), float(odom[1]))
        if not self.in_map(*odom):
            raise ValueError("sensor outside the map")
        mn, mx = self.window(odom)
        g = self.grid
        if not self.perspective:
            self.raycast(points, odom)
            self.remove_outliers(odom)
            for x in range(mn[0], mx[0] + 1):
                for y in range(mn[1], mx[1] + 1):
                    v = self.log_odds[x, y]
                    if g[x, y] == UNKNOWN and v >= self.l_min and v <= self.l_occ:
                        g[x, y] = UNOCCUPIED
                    elif v > self.l_occ:
                        g[x, y] = OCCUPIED
        else:
            for x in range(mn[0], mx[0] + 1):
                for y in range(mn[1], mx[1] + 1):
                    if g[x, y] == UNKNOWN:
                        g[x, y] = UNOCCUPIED
            for p in points:
                c = (float(p[0]), float(p[1]))
                if not self.in_map(*c):
                    continue
                g[self.index(*c)] = OCCUPIED


# ---- the shapes of the tests ---------------------------------------------------------------------------------------------------
NX, NY, RES, X_LO, Y_LO, RANGE = 64, 48, 0.1, -3.2, -2.4, 2.0
POSES = [(0.03, 0.07, 0.0), (0.61, -0.22, 0.4), (2.35, 1.71, -1.0)]


def wall(p0, p1, n):
    t = np.linspace(0.0, 1.0, n)[:, None]
    return np.asarray(p0)[None] * (1 - t) + np.asarray(p1)[None] * t


def raycast_scan(pose, seed):
    """about 300 float32 points round `pose`: wall segments in range, points beyond range, points outside the map on all four
    sides, a point in the sensor's own cell, 200 points in one cell, and non-finite points: a NaN x, a NaN y, an infinite x, both
    infinite"""
    rng = np.random.default_rng(seed)
    ox, oy = pose[0], pose[1]
    parts = [wall((ox + 0.9, oy - 0.8), (ox + 0.9, oy + 0.8), 30), wall((ox - 1.2, oy + 0.7), (ox + 0.4, oy + 1.1), 25),
             wall((ox - 0.5, oy - 1.3), (ox - 1.4, oy - 0.2), 20)]
    ang = rng.uniform(-math.pi, math.pi, 12)
    parts.append(np.stack([ox + 2.6 * np.cos(ang), oy + 2.6 * np.sin(ang)], 1))                     # beyond the range (some outside)
    parts.append(np.array([[5.0, oy + 0.3], [-5.5, oy - 0.4], [ox + 0.2, 4.1], [ox - 0.3, -3.9],     # outside, all four sides
                           [7.0, 6.0], [-9.0, -4.0], [ox, 30.0], [1.0e4, oy]]))
    parts.append(np.array([[ox + 0.004, oy + 0.003]]))                                               # the sensor's own cell
    cx = (math.floor((ox + 0.75 - X_LO) / RES) + 0.5) * RES + X_LO                                   # 200 points in one cell
    cy = (math.floor((oy - 0.55 - Y_LO) / RES) + 0.5) * RES + Y_LO
    parts.append(np.stack([cx + rng.uniform(-0.03, 0.03, 200), cy + rng.uniform(-0.03, 0.03, 200)], 1))
    parts.append(np.array([[np.nan, 0.5], [ox + 0.3, np.nan], [np.inf, oy + 0.2], [-np.inf, np.inf]]))
    pts = np.concatenate(parts).astype(np.float32)
    return pts[rng.permutation(len(pts))]


def raycast_scans():
    return [(raycast_scan(p, 100 + k), p) for k, p in enumerate(POSES)]


def perspective_scans():
    out = []
    for k, p in enumerate(POSES[:2]):
        ox, oy = p[0], p[1]
        pts = np.concatenate([wall((ox + 0.6, oy - 0.5), (ox + 0.6, oy + 0.5), 20),
                              np.array([[ox - 2.7, oy + 0.2],            # beyond the range, inside the map: Occupied
                                        [9.0, 0.0], [0.0, -7.0],         # outside the map: ignored
                                        [np.nan, 1.0], [ox + 0.3, np.nan], [np.inf, 0.0], [0.2, -np.inf]])]).astype(np.float32)
        out.append((pts, p))
    return out


def large_scan(n=5000, seed=7):
    """one scan for a 160 x 160 map at res 0.1 round the origin, range 6.0: a ring of walls, far points and points outside"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-math.pi, math.pi, n)
    r = np.where(rng.uniform(size=n) < 0.7, 3.0 + 1.5 * np.sin(3 * ang), rng.uniform(0.2, 12.0, n))
    pose = (0.37, -0.21, 0.0)
    pts = np.stack([pose[0] + r * np.cos(ang), pose[1] + r * np.sin(ang)], 1).astype(np.float32)
    return pts, pose


def crowded_scan(seed=11):
    """more rays through one cell than a short holds: 36000 points on a short wall 1.5 m ahead of POSES[0], so that the sensor's
    cell and the first cells of the fan each see more than 32767 rays, 4000 points round the sensor, three hits in the sensor's
    own cell (with a wrapped, negative total the rule "hit >= total - 3 * hit" would make that cell a hit) and a NaN point"""
    rng = np.random.default_rng(seed)
    pose = POSES[0]
    ox, oy = pose[0], pose[1]
    ang, r = rng.uniform(-math.pi, math.pi, 4000), rng.uniform(0.5, 2.4, 4000)
    pts = np.concatenate([np.stack([np.full(36000, ox + 1.5), oy + rng.uniform(-0.04, 0.04, 36000)], 1),
                          np.stack([ox + r * np.cos(ang), oy + r * np.sin(ang)], 1),
                          np.array([[ox + 0.004, oy + 0.003], [ox - 0.01, oy + 0.01], [ox + 0.02, oy - 0.02], [np.nan, 0.5]])]).astype(np.float32)
    return pts[rng.permutation(len(pts))], pose


def as_short(n):
    """what the reference's short count holds after n increments"""
    return (int(n) + 32768) % 65536 - 32768


def multiplied_rows(m, odom):
    """the lattice as start + i * res would give it (what the implementation must NOT do)"""
    def row(o):
        out, i = [], 0
        while o - m.range + i * m.res < o + m.range + 1e-10:
            out.append(o - m.range + i * m.res)
            i += 1
        return out
    return row(odom[0]), row(odom[1])


# ---- scenarios: what both test files run (the CPU harness and the device) and compare with OracleMap ---------------------------
SKIP_POSE = (-2.6, 0.13, 0.0)   # its x lattice, by accumulated rounding, never enters column 8; -2.6 - 2.0 + i * 0.1 does
SKIP_HOLE, CONTROL_HOLE = (8, 26), (10, 26)
SINGLE_HOLE, PAIR_HOLES, RING_CELL = (30, 25), ((34, 25), (35, 25)), (0, 30)
NEAR_BORDER_POSE, IN_BORDER_CELL_POSE = (-3.05, 0.0, 0.0), (-3.15, 1.05, 0.0)


def outlier_seed():
    g = np.full((NX, NY), UNOCCUPIED, np.uint8)
    for c in (SKIP_HOLE, CONTROL_HOLE, SINGLE_HOLE, *PAIR_HOLES, RING_CELL):
        g[c] = UNKNOWN
    g[0:3, 23:26] = UNKNOWN   # round the sensor cell (1, 24) of NEAR_BORDER_POSE
    g[0:2, 33:36] = UNKNOWN   # round the sensor cell (0, 34) of IN_BORDER_CELL_POSE: the row x = -1 does not exist
    return g


def state_rule_scans():
    """a hit on one cell twice, then two scans whose only ray passes through it"""
    pose = POSES[0]
    hit = np.array([[pose[0] + 0.8, pose[1] + 0.31]], np.float32)
    beyond = np.array([[pose[0] + 1.6, pose[1] + 0.62]], np.float32)
    return [(hit, pose), (hit, pose), (beyond, pose), (beyond, pose)]


def scenario(name):
    small = dict(nx=NX, ny=NY, x_lo=X_LO, y_lo=Y_LO, res=RES, range=RANGE, perspective=False, seed=None)
    none = np.zeros((0, 2), np.float32)
    if name == "raycast":
        return dict(small, scans=raycast_scans())
    if name == "state_rule":
        return dict(small, scans=state_rule_scans())
    if name == "outliers":
        return dict(small, seed=outlier_seed(), scans=[(none, p) for p in (SKIP_POSE, POSES[0], NEAR_BORDER_POSE, IN_BORDER_CELL_POSE)])
    if name == "perspective":
        return dict(small, perspective=True, scans=perspective_scans())
    if name == "crowded":
        return dict(small, scans=[crowded_scan()])
    if name == "large":
        return dict(nx=160, ny=160, x_lo=-8.0, y_lo=-8.0, res=0.1, range=6.0, perspective=False, seed=None, scans=[large_scan()])
    raise KeyError(name)


SCENARIOS = ("raycast", "state_rule", "outliers", "perspective", "large", "crowded")
_expected, _totals = {}, {}


def new_oracle(s, log_odds5):
    m = OracleMap(s["nx"], s["ny"], s["x_lo"], s["y_lo"], s["res"], log_odds5, s["range"], s["perspective"])
    if s["seed"] is not None:
        m.grid[:] = s["seed"]
    return m


def expected(name, log_odds5):
    """[(grid, log_odds)] after every scan of the scenario, computed once per set of log-odds and shared"""
    key = (name, tuple(float(v) for v in log_odds5))
    if key not in _expected:
        s = scenario(name)
        m = new_oracle(s, log_odds5)
        out, tot = [], []
        for pts, pose in s["scans"]:
            m.integrate(pts, pose)
            tot.append(m.last_total.copy())
            assert not m.count_all.any() and not m.count_hit.any() and not m.queue
            g, l = m.grid.copy(), m.log_odds.copy()
            g.setflags(write=False)
            l.setflags(write=False)
            out.append((g, l))
        _expected[key], _totals[key] = out, tot
    return _expected[key]


def totals(name, log_odds5):
    """[count_all] of every scan of the scenario as the oracle's update saw it (raycast mode), before it was zeroed"""
    expected(name, log_odds5)
    return _totals[(name, tuple(float(v) for v in log_odds5))]


def default_log_odds():
    """logit of 0.99, 0.35, 0.12, 0.90, 0.80 (mapsim.yaml) with Python's log: what the CPU tests hand to both sides"""
    return [math.log(p / (1 - p)) for p in (0.99, 0.35, 0.12, 0.90, 0.80)]
