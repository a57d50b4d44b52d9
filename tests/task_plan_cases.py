"""The contract of csrc/task_plan.h as a sequential oracle, and the scenes the CPU harness and the GPU are compared on.

The oracle has the reference's shape (plan_manager.hpp:252-432): one mission at a time, one pair at a time.  Per pair (i, j), i < j,
as the reference calls jps_planner_->plan(points[i], points[j]): Dijkstra (path_search_cases.dijkstra, a heap on exact pair costs)
in the mission's window with the pair's safe distance, the GOAL at the cell of j and the cost read at the cell of i -- the kernels
do it the other way round, one field from i for every j.  (A field depends on the window, the safe distance and the goal cell only,
so pairs that share all three share the Dijkstra run through a cache.)  The greedy mode is a literal transcription of the
contract; the optimal mode is Held-Karp on Python integers, costs compared by path_search_cases.less, and for n <= 7 it is checked
against all permutations (brute_force).  Everything is compared with ==."""
import functools
import itertools
import math

import numpy as np

from tests import path_search_cases as ps

MAX_TASKS, P_MAX, MAX_LEGS = 10, 21, 20
OK, MASKED, E_ENDPOINT, E_WINDOW, E_TASKS, E_NO_ORDER = 0, 1, -1, -3, -6, -7
GREEDY, OPTIMAL = 0, 1
INF = (-1, -1)
FILL_I, FILL_D = -9, ps.SENTINEL                     # what the slab holds before a launch


def less(p, q):
    """p < q for sums of pairs; INF is larger than every sum and not less than itself"""
    if p == INF:
        return False
    if q == INF:
        return True
    return ps.less(p, q)


def add(p, q):
    return INF if INF in (p, q) else (p[0] + q[0], p[1] + q[1])


class Result:
    def __init__(self, status, **kw):
        self.status, self.n, self.P, self.matrix, self.order, self.total, self.legs, self.fields, self.window = status, 0, 0, None, [], None, [], None, None
        self.__dict__.update(kw)


_fields = {}


def _field(m, win, safe, goal):
    key = (id(m), win, safe, goal)
    if key not in _fields:
        x0, y0, x1, y1 = win
        sub = m.dist[x0:x1 + 1, y0:y1 + 1]
        free = {(x0 + int(i), y0 + int(j)) for i, j in np.argwhere(~(sub < safe))}
        _fields[key] = (m, ps.dijkstra(free, goal) if goal in free else {})
    return _fields[key][1]


def pair_safe(m, safe_dis, ci, cj):
    s = ps.std_max(ps.std_min(safe_dis, 0.8 * float(m.dist[ci])), 0.0)
    return ps.std_max(ps.std_min(s, 0.8 * float(m.dist[cj])), 0.0)


def check(m, n, max_tasks, pts, assign, mode, margin):
    """status, window"""
    if n < 1 or n > max_tasks:
        return E_TASKS, None
    if mode == OPTIMAL and assign is not None and sorted(assign[:n]) != list(range(n)):
        return E_TASKS, None
    for x, y in pts[:1 + 2 * n]:
        if not (math.isfinite(x) and math.isfinite(y)) or x < m.x_lo or x > m.x_hi or y < m.y_lo or y > m.y_hi:
            return E_ENDPOINT, None
    cells = [m.cell(x, y) for x, y in pts[:1 + 2 * n]]
    md = min(max(math.ceil(margin / m.res), 0), 10 ** 9)
    x0, x1 = max(min(c[0] for c in cells) - md, 0), min(max(c[0] for c in cells) + md, m.nx - 1)
    y0, y1 = max(min(c[1] for c in cells) - md, 0), min(max(c[1] for c in cells) + md, m.ny - 1)
    win = (x0, y0, x1, y1)
    return (E_WINDOW if (x1 - x0 + 1) * (y1 - y0 + 1) > ps.MAX_CELLS else OK), win


def cost_matrix(m, P, cells, win, safe_dis):
    mat = {(i, i): (0, 0) for i in range(P)}
    for i in range(P):
        for j in range(i + 1, P):
            if cells[i] == cells[j]:
                d = (0, 0)
            else:
                safe = pair_safe(m, safe_dis, cells[i], cells[j])
                d = INF if m.dist[cells[i]] < safe else _field(m, win, safe, cells[j]).get(cells[i], INF)
            mat[i, j] = mat[j, i] = d
    return mat


def greedy(mat, n):
    item_seen, target_seen, order, cur, total = [False] * n, [False] * n, [], 0, (0, 0)
    for _ in range(n):
        best, pick = INF, -1
        for i in range(n):
            if not item_seen[i] and less(mat[cur, 1 + i], best):
                best, pick = mat[cur, 1 + i], i
        if pick == -1:
            break
        item_seen[pick], cur, total = True, 1 + pick, add(total, best)
        order.append(pick)
        best, pick = INF, -1
        for i in range(n):
            if not target_seen[i] and less(mat[cur, n + 1 + i], best):
                best, pick = mat[cur, n + 1 + i], i
        if pick == -1:
            break
        target_seen[pick], cur, total = True, n + 1 + pick, add(total, best)
        order.append(pick)
    return order, total


def held_karp(mat, n, assign):
    """(item sequence, total) of the lexicographically smallest optimal order, or (None, INF)"""
    full = (1 << n) - 1

    @functools.lru_cache(maxsize=None)
    def togo(S, at):
        if S == full:
            return (0, 0)
        best = INF
        for i in range(n):
            if not S >> i & 1:
                c = step(S, at, i)
                if less(c, best):
                    best = c
        return best

    def step(S, at, i):
        return add(add(mat[at, 1 + i], mat[1 + i, n + 1 + assign[i]]), togo(S | 1 << i, n + 1 + assign[i]))

    total = togo(0, 0)
    if total == INF:
        return None, INF
    seq, S, at, want = [], 0, 0, total
    while S != full:
        i = next(i for i in range(n) if not S >> i & 1 and step(S, at, i) == want)
        seq.append(i)
        S, at = S | 1 << i, n + 1 + assign[i]
        want = togo(S, at)
    return seq, total


def brute_force(mat, n, assign):
    """the same by all permutations in lexicographic order, the first strict minimum"""
    best, seq = INF, None
    for perm in itertools.permutations(range(n)):
        c, at = (0, 0), 0
        for i in perm:
            c = add(add(c, mat[at, 1 + i]), mat[1 + i, n + 1 + assign[i]])
            at = n + 1 + assign[i]
        if less(c, best):
            best, seq = c, list(perm)
    return seq, best


def plan(m, n, max_tasks, pts, assign=None, mode=GREEDY, safe_dis=ps.SAFE_DIS, margin=ps.MARGIN):
    pts = [(float(x), float(y)) for x, y in pts]
    status, win = check(m, n, max_tasks, pts, assign, mode, margin)
    if status != OK:
        return Result(status, window=win)
    P = 1 + 2 * n
    cells = [m.cell(x, y) for x, y in pts[:P]]
    mat = cost_matrix(m, P, cells, win, safe_dis)
    fields = sum(len({pair_safe(m, safe_dis, cells[k], cells[j]) for j in range(k + 1, P)}) for k in range(P - 1))
    res = Result(OK, n=n, P=P, matrix=mat, fields=fields, window=win)
    if mode == OPTIMAL:
        asg = list(assign[:n]) if assign is not None else list(range(n))
        seq, total = held_karp(mat, n, asg)
        if seq is None:
            res.status = E_NO_ORDER
            return res
        res.order, res.total = [v for i in seq for v in (i, asg[i])], total
    else:
        res.order, res.total = greedy(mat, n)
    at = 0
    for e, v in enumerate(res.order):
        nxt = n + 1 + v if e & 1 else 1 + v
        res.legs.append((pts[at], pts[nxt]))
        at = nxt
    return res


def expected_arrays(r):
    """what a pre-filled slab row holds after the mission (sweeps left out: the oracle does not sweep)"""
    out = {"status": r.status, "matrix": np.full((P_MAX, P_MAX, 2), FILL_I, np.int32), "order": np.full(MAX_LEGS, FILL_I, np.int32),
           "n_order": FILL_I if r.status == MASKED else len(r.order), "total": np.full(2, FILL_I, np.int32),
           "leg_start_xy": np.full((MAX_LEGS, 2), FILL_D), "leg_goal_xy": np.full((MAX_LEGS, 2), FILL_D),
           "fields": FILL_I if r.fields is None else r.fields}
    if r.matrix is not None:
        for (i, j), d in r.matrix.items():
            out["matrix"][i, j] = d
    if r.status == OK:
        out["order"][:len(r.order)] = r.order
        out["total"][:] = r.total
        for e, (a, b) in enumerate(r.legs):
            out["leg_start_xy"][e], out["leg_goal_xy"][e] = a, b
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------------
NX, NY, RES, X_LO, Y_LO = ps.NX, ps.NY, ps.RES, ps.X_LO, ps.Y_LO
pt = ps.pt


def mission(n, robot, items, targets, assign=None, max_tasks=None):
    """points packed as the contract has them; the row is padded with NaN up to max_tasks"""
    return {"n": n, "pts": [robot] + list(items[:n]) + list(targets[:n]), "assign": assign, "max_tasks": max_tasks or max(n, 1)}


def _scene(occ, missions, mode=GREEDY, safe_dis=ps.SAFE_DIS, margin=ps.MARGIN, max_tasks=None, m=None):
    m = m or ps.Map(ps.brute_dist(occ), X_LO, Y_LO, RES)
    T = max_tasks or max(ms["max_tasks"] for ms in missions)
    return {"map": m, "missions": missions, "mode": mode, "safe_dis": safe_dis, "margin": margin, "max_tasks": T}


# ten items on the left, ten targets on the right, all at least five cells from every wall of the scenes below
ITEMS = [pt(6 + 2 * (i % 5), 6 + 8 * i // 2, 0.2 + 0.06 * i, 0.7 - 0.05 * i) for i in range(10)]
TARGETS = [pt(44 + 3 * (i % 5), 5 + 4 * i, 0.9 - 0.07 * i, 0.1 + 0.08 * i) for i in range(10)]
ROBOT = pt(24, 24, 0.4, 0.6)
SIZES = (1, 3, 10)


@functools.lru_cache(maxsize=None)
def scene(name):
    occ = np.zeros((NX, NY), bool)
    kind, _, arg = name.partition(":")
    n = int(arg) if arg.isdigit() else 0
    if kind == "open":
        return _scene(occ, [mission(n, ROBOT, ITEMS, TARGETS)])
    if kind == "wall_gap":
        occ[32, :] = True
        occ[32, 30:39] = False
        return _scene(occ, [mission(n, ROBOT, ITEMS, TARGETS)])
    if kind == "clamp":             # item 0 two cells from a wall: 0.8 * 0.2 caps the safe distance of its pairs
        occ[3, 0:20] = True
        items = [pt(5, 10)] + ITEMS[1:]
        return _scene(occ, [mission(n, ROBOT, items, TARGETS)])
    if kind == "box":               # target 0 inside a closed box
        occ[40:51, 20] = occ[40:51, 30] = True
        occ[40, 20:31] = occ[50, 20:31] = True
        targets = [pt(45, 25)] + [pt(56 + (i % 2) * 3, 4 + 4 * i) for i in range(1, 10)]
        return _scene(occ, [mission(n, ROBOT, ITEMS, targets)], safe_dis=0.05)
    if kind == "same_cell":         # item 0 and target 0 in one cell
        targets = [pt(6, 6, 0.9, 0.1)] + TARGETS[1:]
        items = [pt(6, 6, 0.1, 0.8)] + ITEMS[1:]
        return _scene(occ, [mission(n, ROBOT, items, targets)])
    if kind == "whole_map":         # 48 x 48, the window of the mission and of every pair is the whole map
        o = np.zeros((48, 48), bool)
        o[24, 0:30] = True
        o[10:20, 40] = True
        o[34:41, 8] = o[34:41, 14] = True
        o[34, 8:15] = o[40, 8:15] = True
        m = ps.Map(ps.brute_dist(o), -2.4, -2.4, RES)
        q = lambda ix, iy: (-2.4 + (ix + 0.5) * RES, -2.4 + (iy + 0.5) * RES)
        items = [q(5, 5), q(12, 30), q(8, 44), q(18, 12)]
        targets = [q(37, 11), q(44, 40), q(30, 4), q(40, 25)]          # target 0 inside the closed box
        return _scene(o, [mission(4, q(20, 20), items, targets)], margin=10.0, m=m, safe_dis=0.05)
    if kind == "leg_window":        # two walls that overlap in y: inside the pair's window (margin 0.5 m) the way from the robot to
        occ[28, 14:29] = True      # the item zigzags between them; the mission's window reaches down to the target, and round the
        occ[32, 20:35] = True      # lower end of the first wall it is shorter
        ms = mission(1, pt(10, 24), [pt(50, 24)], [pt(30, 4)])
        return _scene(occ, [ms], safe_dis=0.05, margin=0.5)
    if kind == "differ":            # greedy and optimal differ: the nearest item first is the wrong start
        ms = mission(2, pt(10, 24), [pt(14, 26), pt(4, 22)], [pt(60, 20), pt(2, 25)])
        return _scene(occ, [ms], mode=GREEDY if arg == "greedy" else OPTIMAL)
    if kind == "mirror":            # item 0 on the axis x = 32, items 1 and 2 and their targets mirror images: a tie at the second step
        ms = mission(3, pt(32, 4), [pt(32, 10), pt(42, 30), pt(22, 30)], [pt(32, 20), pt(42, 40), pt(22, 40)])
        return _scene(occ, [ms], mode=GREEDY if arg == "greedy" else OPTIMAL)
    if kind == "assign":            # the scene where they differ with the assignment crossed, and a rotation for three tasks
        a = mission(2, pt(10, 24), [pt(14, 26), pt(4, 22)], [pt(60, 20), pt(2, 25)], assign=[1, 0], max_tasks=3)
        b = mission(3, ROBOT, ITEMS, TARGETS, assign=[1, 2, 0], max_tasks=3)
        return _scene(occ, [a, b], mode=OPTIMAL)
    if kind == "unreachable":       # target 0 inside the closed box: greedy stops after an item, optimal has no order
        s = scene("box:3")
        ms = dict(s["missions"][0], n=2, pts=[ROBOT] + ITEMS[:2] + s["missions"][0]["pts"][4:6])
        return {**s, "missions": [ms], "mode": GREEDY if arg == "greedy" else OPTIMAL}
    if kind == "bad":               # n = 0, n > max_tasks, no permutation (twice), a NaN, outside the map, then a good one
        good = [ROBOT] + ITEMS[:2] + TARGETS[:2]
        nan = float("nan")
        return _scene(occ, [dict(n=0, pts=good, assign=None, max_tasks=2), dict(n=3, pts=good, assign=None, max_tasks=2),
                            dict(n=2, pts=good, assign=[0, 0], max_tasks=2), dict(n=2, pts=good, assign=[0, 2], max_tasks=2),
                            dict(n=2, pts=good[:3] + [(nan, 0.0)] + good[4:], assign=[1, 0], max_tasks=2),
                            dict(n=2, pts=good[:4] + [(0.0, Y_LO - 0.01)], assign=[1, 0], max_tasks=2),
                            dict(n=0, pts=[(nan, nan)] * 5, assign=[5, 5], max_tasks=2),      # tasks comes before end point
                            dict(n=1, pts=good[:4] + [(nan, nan)], assign=[0, 7], max_tasks=2),  # beyond n nothing is read
                            dict(n=2, pts=good, assign=[1, 0], max_tasks=2)], mode=OPTIMAL)
    if kind == "window":            # 400 x 400 at 0.1 m: points 30 m apart need more than 32768 cells
        m = ps.Map(np.full((400, 400), 10.0), -20.0, -20.0, RES)
        far = dict(n=1, pts=[(-15.05, -15.05), (14.95, -14.0), (-14.0, 14.95)], assign=None, max_tasks=1)
        near = dict(n=1, pts=[(-15.05, -15.05), (-12.0, -14.0), (-14.0, -11.5)], assign=None, max_tasks=1)
        return _scene(None, [far, near], m=m)
    raise KeyError(name)


MATRIX_SCENES = tuple("%s:%d" % (k, n) for k in ("open", "wall_gap", "clamp", "box", "same_cell") for n in SIZES)
ORDER_SCENES = ("differ:greedy", "differ:optimal", "mirror:greedy", "mirror:optimal", "assign", "unreachable:greedy", "unreachable:optimal")
SCENES = MATRIX_SCENES + ("whole_map", "leg_window") + ORDER_SCENES + ("bad", "window")

RANDOM_MISSIONS, RANDOM_T = 64, 10
RNX, RNY = 36, 28


@functools.lru_cache(maxsize=None)
def random_scene(mode):
    """64 missions of mixed n on one small map with box obstacles and a closed ring; four in five have their points clear of the obstacles by 0.4 m,
    the others anywhere; in the optimal mode every mission has a random assignment"""
    rng = np.random.default_rng(20261018)
    occ = np.zeros((RNX, RNY), bool)
    for _ in range(3):
        w, h = rng.integers(2, 5, 2)
        x, y = rng.integers(0, RNX - w), rng.integers(0, RNY - h)
        occ[x:x + w, y:y + h] = True
    occ[24:31, 4] = occ[24:31, 10] = occ[24, 4:11] = occ[30, 4:11] = True     # a closed ring: a point inside it is cut off
    m = ps.Map(ps.brute_dist(occ), -1.8, -1.4, RES)
    missions = []
    for k in range(RANDOM_MISSIONS):
        n = int(rng.choice([1, 2, 3, 4, 5, 6, 8, 10], p=[0.15, 0.2, 0.2, 0.15, 0.1, 0.1, 0.05, 0.05]))
        clear = rng.random() < 0.8
        pts = []
        while len(pts) < 1 + 2 * n:
            x, y = float(rng.uniform(m.x_lo, m.x_hi)), float(rng.uniform(m.y_lo, m.y_hi))
            if not clear or m.dist[m.cell(x, y)] >= 0.4:
                pts.append((x, y))
        assign = [int(v) for v in rng.permutation(n)] + [0] * (RANDOM_T - n)
        missions.append(dict(n=n, pts=pts, assign=assign if mode == OPTIMAL else None, max_tasks=RANDOM_T))
    return _scene(occ, missions, mode=mode, margin=float(1.0), m=m)


def get_scene(name):
    return random_scene(name[1]) if isinstance(name, tuple) else scene(name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's results of a scene (name, or ("random", mode)), computed once"""
    s = get_scene(name)
    return tuple(plan(s["map"], ms["n"], s["max_tasks"], ms["pts"], ms["assign"], s["mode"], s["safe_dis"], s["margin"]) for ms in s["missions"])


def arrays(s):
    """the inputs of a scene as the calls take them: n_tasks [count], points [count][1 + 2 T][2] (NaN beyond a mission's points),
    assignment [count][T] or None"""
    T, ms = s["max_tasks"], s["missions"]
    pts = np.full((len(ms), 1 + 2 * T, 2), np.nan)
    asg = np.zeros((len(ms), T), np.int32)
    for k, q in enumerate(ms):
        p = np.asarray(q["pts"][:1 + 2 * T], np.float64)
        pts[k, :len(p)] = p
        if q["assign"] is not None:
            asg[k, :len(q["assign"][:T])] = q["assign"][:T]
    has = any(q["assign"] is not None for q in ms)
    return np.array([q["n"] for q in ms], np.int32), pts, asg if has else None
