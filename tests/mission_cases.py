"""Oracle and scenario generators of the mission-map tests (test_mission_map_cpu.py, test_mission_map_gpu.py).

A sequential restatement, in the reference's own shape, of what plan_manager does to its map while a mission runs
(planning_ddr_opt/plan_manager/include/plan_manager/plan_manager.hpp): the double loops of paintSquare / paintBox / paintTable /
paintChair (:470-496) over SDFmap::setObs / setFree (utils/plan_env/src/sdf_map.cpp:485-509), "items -> OBS" and the two rules of
MapUpdateThread (:498-554), nearest_point and the goal classification of MainThread (:618-658) and the post-plan rule (:695-704).
It works on the NumPy state grid of an occupancy_cases.OracleMap; the narrowing of setObs / setFree is np.float32, everything else
plain Python floats (IEEE double, no fused multiply-add).  The kernels' shape (descriptors, masks, last writer wins, a compacted
list) is not restated here: edits are applied one after the other, cell by cell.  The oracle is unpinned, like the map oracle
(plan_manager needs ROS to build).  The deviations of csrc/mission_map.h are the oracle's too: an invalid edit is skipped and
counted, an index that rounding takes to n is clamped, all missions share one map."""
import math

import numpy as np

from tests import occupancy_cases as occ

OK, MASKED, E_POINT, E_TASKS = 0, 1, -1, -6
PHASE_NONE, PHASE_ITEM, PHASE_TARGET = 0, 1, 2
GOAL_OK, GOAL_E_POINT = 0, -1
MAX_TASKS, MAX_LATTICE = 10, 64
KIND_HALF = {1: (0.25, 0.15), 2: (0.5, 0.25), 3: (0.2, 0.2)}   # paintBox, paintTable, paintChair
PARAMS = dict(item_half=0.5, free_half=0.5, item_free_dist=2.0, target_lock_half=0.3, target_lock_dist=0.5, left_target_half=0.2,
              left_target_dist=0.3)
EDIT_DTYPE = np.dtype([("cx", np.float64), ("cy", np.float64), ("hx", np.float64), ("hy", np.float64), ("make_obs", np.int32),
                       ("reserved", np.int32)])


def new_map():
    return occ.OracleMap(occ.NX, occ.NY, occ.X_LO, occ.Y_LO, occ.RES, occ.default_log_odds(), occ.RANGE)


# ---- setObs / setFree and the paint loops ----------------------------------------------------------------------------------------
def set_cell(m, x, y, state, narrow=True):
    cx, cy = (float(np.float32(x)), float(np.float32(y))) if narrow else (x, y)
    if cx < m.x_lo or cy < m.y_lo or cx >= m.x_hi or cy >= m.y_hi:
        return
    ix, iy = int((cx - m.x_lo) * m.inv), int((cy - m.y_lo) * m.inv)
    m.grid[min(ix, m.nx - 1), min(iy, m.ny - 1)] = state


def lattice(c, h, res, accumulated=True):
    out = []
    if accumulated:
        v = c - h
        while v <= c + h:
            out.append(v)
            v += res
    else:   # what the implementation must NOT do
        i = 0
        while c - h + i * res <= c + h:
            out.append(c - h + i * res)
            i += 1
    return out


def edit_valid(e, res):
    cx, cy, hx, hy = (float(v) for v in e[:4])
    if not all(math.isfinite(v) for v in (cx, cy, hx, hy)) or hx < 0 or hy < 0:
        return False
    return all(2 * h / res < 2.0 ** 31 and int(2 * h / res) + 2 <= MAX_LATTICE for h in (hx, hy))


def paint(m, e, accumulated=True, narrow=True):
    cx, cy, hx, hy, make_obs = float(e[0]), float(e[1]), float(e[2]), float(e[3]), int(e[4])
    for x in lattice(cx, hx, m.res, accumulated):
        for y in lattice(cy, hy, m.res, accumulated):
            set_cell(m, x, y, occ.OCCUPIED if make_obs else occ.UNOCCUPIED, narrow)


def paint_list(m, edits, **how):
    """the edits one after the other; returns (n_changed, (min_x, min_y, max_x, max_y), n_skipped)"""
    before, skipped = m.grid.copy(), 0
    for e in edits:
        if edit_valid(e, m.res):
            paint(m, e, **how)
        else:
            skipped += 1
    ch = np.argwhere(m.grid != before)
    box = (m.nx, m.ny, -1, -1) if not len(ch) else (int(ch[:, 0].min()), int(ch[:, 1].min()), int(ch[:, 0].max()), int(ch[:, 1].max()))
    return len(ch), box, skipped


def as_array(edits):
    a = np.zeros(len(edits), EDIT_DTYPE)
    for k, e in enumerate(edits):
        a[k] = (float(e[0]), float(e[1]), float(e[2]), float(e[3]), int(e[4]), 0)
    return a


# ---- missions --------------------------------------------------------------------------------------------------------------------
def dist(ax, ay, bx, by):
    dx, dy = ax - bx, ay - by
    return math.sqrt(dx * dx + dy * dy)


def nearest(pts, px, py):
    best, at = 1.7976931348623157e308, -1
    for i, (x, y) in enumerate(pts):
        d = dist(px, py, x, y)
        if d < best:
            best, at = d, i
    return at, best


class Missions:
    def __init__(self, m, slots, params=None):
        self.m, self.B, self.P = m, slots, dict(PARAMS, **(params or {}))
        self.status = np.full(slots, MASKED, np.int32)
        self.phase = np.zeros(slots, np.int32)
        self.goal_item = np.full(slots, -1, np.int32)
        self.goal_target = np.full(slots, -1, np.int32)
        self.goal_status = np.zeros(slots, np.int32)
        self.items, self.targets, self.kinds = [[] for _ in range(slots)], [[] for _ in range(slots)], [[] for _ in range(slots)]
        self.edits, self.counters = [], (0, (m.nx, m.ny, -1, -1), 0)

    def _apply(self, edits):
        self.edits = edits
        self.counters = paint_list(self.m, edits)

    def set(self, n_tasks, points, kinds=None, mask=None):
        edits = []
        for b, n in enumerate(n_tasks):
            if mask is not None and not mask[b]:
                continue
            n, row = int(n), np.asarray(points[b], np.float64).reshape(-1, 2)
            T = (len(row) - 1) // 2
            k = [0] * T if kinds is None else [int(v) for v in kinds[b]]
            status = OK
            if n < 1 or n > T or any(v not in (0, 1, 2, 3) for v in k[:n]):
                status = E_TASKS
            elif not np.isfinite(row[1:1 + 2 * n]).all():
                status = E_POINT
            self.status[b], self.phase[b], self.goal_item[b], self.goal_target[b], self.goal_status[b] = status, PHASE_NONE, -1, -1, GOAL_OK
            self.items[b] = self.targets[b] = self.kinds[b] = []
            if status != OK:
                continue
            self.items[b] = [(float(x), float(y)) for x, y in row[1:1 + n]]
            self.targets[b] = [(float(x), float(y)) for x, y in row[1 + n:1 + 2 * n]]
            self.kinds[b] = k[:n]
            for (x, y), kind in zip(self.items[b], self.kinds[b]):
                hx, hy = KIND_HALF.get(kind, (self.P["item_half"],) * 2)
                edits.append((x, y, hx, hy, 1))
        self._apply(edits)

    def set_goals(self, goals, mask=None):
        for b, (gx, gy) in enumerate(goals):
            if (mask is not None and not mask[b]) or self.status[b] != OK:
                continue
            gx, gy = float(gx), float(gy)
            if not (math.isfinite(gx) and math.isfinite(gy)):
                self.phase[b], self.goal_status[b] = PHASE_NONE, GOAL_E_POINT
                continue
            self.goal_item[b], di = nearest(self.items[b], gx, gy)
            self.goal_target[b], dt = nearest(self.targets[b], gx, gy)
            self.phase[b], self.goal_status[b] = (PHASE_ITEM if di < dt else PHASE_TARGET), GOAL_OK

    def step(self, poses, after_plan=None):
        P, edits = self.P, []
        for b, (px, py) in enumerate(poses):
            if self.status[b] != OK or self.phase[b] == PHASE_NONE:
                continue
            px, py = float(px), float(py)
            if self.phase[b] == PHASE_ITEM:
                x, y = self.items[b][self.goal_item[b]]
                if dist(px, py, x, y) < P["item_free_dist"]:
                    edits.append((x, y, P["free_half"], P["free_half"], 0))
            if self.phase[b] == PHASE_TARGET:
                x, y = self.targets[b][self.goal_target[b]]
                if dist(px, py, x, y) < P["target_lock_dist"]:
                    edits.append((x, y, P["target_lock_half"], P["target_lock_half"], 1))
            if after_plan is not None and after_plan[b] and self.phase[b] == PHASE_ITEM:
                t, d = nearest(self.targets[b], px, py)
                if t >= 0 and d < P["left_target_dist"]:
                    x, y = self.targets[b][t]
                    edits.append((x, y, P["left_target_half"], P["left_target_half"], 1))
        self._apply(edits)

    def snapshot(self):
        return dict(status=self.status.copy(), phase=self.phase.copy(), goal_item=self.goal_item.copy(), goal_target=self.goal_target.copy(),
                    goal_status=self.goal_status.copy(), edits=as_array(self.edits), n_changed=self.counters[0], box=self.counters[1],
                    n_skipped=self.counters[2], grid=self.m.grid.copy())


# ---- the edit lists of the paint tests -------------------------------------------------------------------------------------------
PIN_ACCUMULATED = (0.82, 0.05, 0.5, 0.0, 1)    # x lattice: 10 accumulated points, cells 35 .. 44; multiplied: 11, .. 45
PIN_NARROWED = (-2.75, 0.05, 0.25, 0.0, 1)     # paintBox's x half: the five points land in cells 2, 2, 4, 4, 6; in double 2, 3, 4, 5, 6
HALVES = [(0.5, 0.5), (0.3, 0.3), (0.2, 0.2), (0.25, 0.15), (0.5, 0.25)]   # the reference's set
CHAIN = [(0.0, 0.0, 0.5, 0.5, 1), (0.3, 0.2, 0.5, 0.5, 0), (0.5, 0.45, 0.3, 0.3, 1)]   # lock / free / lock, overlapping


def border_edits():
    """clipped at each of the four borders and at a corner, one wholly outside, a zero-half edit (one point)"""
    x_hi, y_hi = occ.X_LO + occ.NX * occ.RES, occ.Y_LO + occ.NY * occ.RES
    return [(occ.X_LO, 0.3, 0.3, 0.3, 1), (x_hi, -0.4, 0.3, 0.3, 1), (0.7, occ.Y_LO, 0.25, 0.15, 1), (-0.9, y_hi, 0.5, 0.25, 1),
            (x_hi - 0.05, y_hi - 0.05, 0.5, 0.5, 1), (9.0, 9.0, 0.5, 0.5, 1), (1.234, -1.017, 0.0, 0.0, 1), (-1.0, -1.0, 0.2, 0.2, 0)]


def seeded_edits(n=300, seed=5):
    """centres on the centimetre grid and at random, halves from the reference's set, both values"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        if k % 2:
            cx, cy = round(rng.uniform(-3.4, 3.4), 2), round(rng.uniform(-2.6, 2.6), 2)
        else:
            cx, cy = float(rng.uniform(-3.4, 3.4)), float(rng.uniform(-2.6, 2.6))
        hx, hy = HALVES[int(rng.integers(len(HALVES)))]
        out.append((cx, cy, hx, hy, int(rng.uniform() < 0.6)))
    return out


def paint_calls():
    """the lists of the paint tests, one call each, on one map"""
    return [[PIN_ACCUMULATED, PIN_NARROWED], border_edits(), CHAIN, seeded_edits()]


_paint = None


def paint_expected():
    """[(grid, n_changed, box, n_skipped)] after every call of paint_calls(), computed once"""
    global _paint
    if _paint is None:
        m, _paint = new_map(), []
        for edits in paint_calls():
            n, box, skipped = paint_list(m, edits)
            g = m.grid.copy()
            g.setflags(write=False)
            _paint.append((g, n, box, skipped))
    return _paint


# ---- the mission scenario: 300 slots -----------------------------------------------------------------------------------------------
SLOTS, T = 300, MAX_TASKS
EPS = 2.0 ** -20


def q64(v):
    """onto the 1/64 grid: sums and differences with 2.0, 0.5 and 0.25 are then exact"""
    return np.round(np.asarray(v) * 64) / 64


def mission_inputs(seed=9):
    """n_tasks, points [SLOTS][1 + 2 T][2], kinds [SLOTS][T], mask: n from 1 to 10 mixed, kinds mixed, points on and round the map (about one in eight lies on it), every 7th slot masked, slots
    with n = 0, n = 11, a NaN item, an infinite target and a bad kind; slots 20 .. 39 hold two items (or an item and a target)
    0.25 either side of (1.0, 0.5), everything else of theirs at x < -0.5"""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, T + 1, SLOTS).astype(np.int32)
    n[20:40] = rng.integers(6, T + 1, 20)
    pts = np.full((SLOTS, 1 + 2 * T, 2), np.nan)          # beyond 1 + 2 n the rows are never read
    kinds = rng.integers(0, 4, (SLOTS, T)).astype(np.int32)
    for b in range(SLOTS):
        k = int(n[b])
        pts[b, 0] = (0.0, 0.0)
        pts[b, 1:1 + 2 * k, 0] = q64(rng.uniform(-8.0, 8.0, 2 * k))
        pts[b, 1:1 + 2 * k, 1] = q64(rng.uniform(-6.0, 6.0, 2 * k))
    for b in range(20, 40):
        k = int(n[b])
        pts[b, 1:1 + 2 * k, 0] = q64(rng.uniform(-8.0, -0.5, 2 * k))
        if b < 30:    # items 2 and 5 equidistant from (1.0, 0.5): the first wins
            pts[b, 1 + 2], pts[b, 1 + 5] = (1.25, 0.5), (0.75, 0.5)
        else:         # item 1 and target 3 equidistant: not "dist_item < dist_target", so TARGET
            pts[b, 1 + 1], pts[b, 1 + k + 3] = (0.75, 0.5), (1.25, 0.5)
    n[3], n[4] = 0, T + 1
    pts[5, 2, 1] = np.nan                                    # a NaN item
    pts[6, 1 + int(n[6]), 0] = np.inf                        # an infinite target
    kinds[8, 0] = 4                                          # a bad kind
    n[10], kinds[10, 7] = 4, 9                                # a bad kind beyond n is never read
    mask = (np.arange(SLOTS) % 7 != 2).astype(np.int32)
    return n, pts, kinds, mask


def mission_goals(n, pts, seed=10):
    """by slot % 5: an item exactly, a target exactly, a random point, a NaN goal (slot % 5 == 3), a random point; slots 20 .. 39
    the midpoint (1.0, 0.5)"""
    rng = np.random.default_rng(seed)
    g = np.stack([q64(rng.uniform(-8.0, 8.0, SLOTS)), q64(rng.uniform(-6.0, 6.0, SLOTS))], 1)
    for b in range(SLOTS):
        k = max(int(n[b]), 1) if 1 <= n[b] <= T else 1
        if b % 5 == 0:
            g[b] = pts[b, 1 + b % k]
        elif b % 5 == 1:
            g[b] = pts[b, 1 + k + b % k]
        elif b % 5 == 3:
            g[b] = (np.nan, 0.0)
    g[20:40] = (1.0, 0.5)
    return g


def mission_poses(o, step):
    """poses and after-plan mask of tick `step` (0, 1, 2) from the oracle's goals, by (slot + step) % 6: exactly at the threshold of
    the phase's rule (item + (2.0, 0), target + (0.5, 0): no edit), just inside it, a NaN pose, far away, 0.25 beside a target
    (rule 2 for its own goal, rule 3 behind the mask), 0.3 beside a target.  The mask: none at tick 0, every third slot at tick 1,
    every second at tick 2"""
    poses = np.zeros((SLOTS, 3))
    for b in range(SLOTS):
        if o.status[b] != OK or o.phase[b] == PHASE_NONE:
            poses[b, :2] = (0.125 * (b % 9), -0.25)
            continue
        goal = o.items[b][o.goal_item[b]] if o.phase[b] == PHASE_ITEM else o.targets[b][o.goal_target[b]]
        reach = 2.0 if o.phase[b] == PHASE_ITEM else 0.5
        t = o.targets[b][b % len(o.targets[b])]
        kind = (b + step) % 6
        if kind == 0:
            poses[b, :2] = (goal[0] + reach, goal[1])
        elif kind == 1:
            poses[b, :2] = (goal[0] + (reach - EPS), goal[1])
        elif kind == 2:
            poses[b, :2] = (np.nan, goal[1]) if b % 2 else (goal[0], np.inf)
        elif kind == 3:
            poses[b, :2] = (10.0, 10.0)
        elif kind == 4:
            poses[b, :2] = (t[0] + 0.25, t[1])
        else:
            poses[b, :2] = (t[0], t[1] - 0.3)
    after = None if step == 0 else (np.arange(SLOTS) % (3 if step == 1 else 2) == 0).astype(np.int32)
    return poses, after


_mission = None


def mission_expected():
    """the calls of the mission scenario and the oracle's snapshot after each, computed once:
    [("set", args, snap), ("goals", args, snap), ("step", args, snap) x 3]"""
    global _mission
    if _mission is None:
        o = Missions(new_map(), SLOTS)
        n, pts, kinds, mask = mission_inputs()
        out = []
        o.set(n, pts, kinds, mask)
        out.append(("set", (n, pts, kinds, mask), o.snapshot()))
        goals = mission_goals(n, pts)
        gmask = (np.arange(SLOTS) % 11 != 5).astype(np.int32)
        o.set_goals(goals, gmask)
        out.append(("goals", (goals, gmask), o.snapshot()))
        for step in range(3):
            poses, after = mission_poses(o, step)
            o.step(poses[:, :2], after)
            out.append(("step", (poses, after), o.snapshot()))
        _mission = out
    return _mission
