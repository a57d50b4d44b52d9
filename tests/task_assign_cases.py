"""The modes of csrc/task_plan.h that choose the item-to-target assignment (ASSIGNED, JOINT) as a sequential oracle, and the scenes
the CPU harness and the GPU are compared on.

The matrix, the exact order of sums, the routing of a fixed assignment (held_karp) and the scene helpers are those of
tests/task_plan_cases.py.  The matching (least sum of carry legs, lexicographically smallest vector) and the joint programme (least
route over all item orders and bijections, lexicographically smallest published order) run on Python integers with memoisation;
each has a brute force that walks every candidate in lexicographic order and keeps the first strict minimum.  Everything is
compared with ==."""
import functools
import itertools

import numpy as np

from tests import path_search_cases as ps
from tests import task_plan_cases as tc

MAX_TASKS, P_MAX, MAX_LEGS = tc.MAX_TASKS, tc.P_MAX, tc.MAX_LEGS
OK, MASKED, E_ENDPOINT, E_WINDOW, E_TASKS, E_NO_ORDER = tc.OK, tc.MASKED, tc.E_ENDPOINT, tc.E_WINDOW, tc.E_TASKS, tc.E_NO_ORDER
GREEDY, OPTIMAL, ASSIGNED, JOINT = tc.GREEDY, tc.OPTIMAL, 2, 3
JOINT_MAX_TASKS = 5
INF, FILL_I, FILL_D = tc.INF, tc.FILL_I, tc.FILL_D
less, add, pt = tc.less, tc.add, tc.pt
MODE_NAMES = {"assigned": ASSIGNED, "joint": JOINT}


def carry_sum(mat, n, assign):
    total = (0, 0)
    for i in range(n):
        total = add(total, mat[1 + i, n + 1 + assign[i]])
    return total


def matching(mat, n):
    """(assignment, sum of its carry legs) of the lexicographically smallest optimal bijection, or (None, INF)"""
    full = (1 << n) - 1

    @functools.lru_cache(maxsize=None)
    def rest(T):
        if T == full:
            return (0, 0)
        k, best = bin(T).count("1"), INF
        for t in range(n):
            if not T >> t & 1:
                c = add(mat[1 + k, n + 1 + t], rest(T | 1 << t))
                if less(c, best):
                    best = c
        return best

    if rest(0) == INF:
        return None, INF
    assign, T = [], 0
    for k in range(n):
        t = next(t for t in range(n) if not T >> t & 1 and add(mat[1 + k, n + 1 + t], rest(T | 1 << t)) == rest(T))
        assign.append(t)
        T |= 1 << t
    return assign, rest(0)


def matching_brute_force(mat, n):
    """the same by all bijections in lexicographic order, the first strict minimum"""
    best, assign = INF, None
    for perm in itertools.permutations(range(n)):
        c = carry_sum(mat, n, perm)
        if less(c, best):
            best, assign = c, list(perm)
    return assign, best


def joint(mat, n):
    """(published order, total) of the lexicographically smallest optimal route over all item orders and bijections, or (None, INF)"""
    full = (1 << n) - 1

    @functools.lru_cache(maxsize=None)
    def togo(Si, St, at):
        if Si == full:
            return (0, 0)
        best = INF
        for i in range(n):
            for t in range(n):
                if not Si >> i & 1 and not St >> t & 1:
                    c = step(Si, St, at, i, t)
                    if less(c, best):
                        best = c
        return best

    def step(Si, St, at, i, t):
        return add(add(mat[at, 1 + i], mat[1 + i, n + 1 + t]), togo(Si | 1 << i, St | 1 << t, n + 1 + t))

    total = togo(0, 0, 0)
    if total == INF:
        return None, INF
    order, Si, St, at, want = [], 0, 0, 0, total
    while Si != full:
        i, t = next((i, t) for i in range(n) for t in range(n) if not Si >> i & 1 and not St >> t & 1 and step(Si, St, at, i, t) == want)
        order += [i, t]
        Si, St, at = Si | 1 << i, St | 1 << t, n + 1 + t
        want = togo(Si, St, at)
    return order, total


def joint_brute_force(mat, n):
    """the same by all (item order, bijection) pairs, the first strict minimum in lexicographic order of the published sequence"""
    routes = sorted([v for k in range(n) for v in (pi[k], sg[k])] for pi in itertools.permutations(range(n)) for sg in itertools.permutations(range(n)))
    best, order = INF, None
    for r in routes:
        c, at = (0, 0), 0
        for k in range(n):
            c = add(add(c, mat[at, 1 + r[2 * k]]), mat[1 + r[2 * k], n + 1 + r[2 * k + 1]])
            at = n + 1 + r[2 * k + 1]
        if less(c, best):
            best, order = c, r
    return order, best


def plan(m, n, max_tasks, pts, mode, safe_dis=ps.SAFE_DIS, margin=ps.MARGIN):
    """one mission in the mode ASSIGNED or JOINT: a task_plan_cases.Result with assignment and assign_total (None where the
    contract leaves the rows untouched).  A given assignment is not an input"""
    pts = [(float(x), float(y)) for x, y in pts]
    if mode == JOINT and n > JOINT_MAX_TASKS:
        return tc.Result(E_TASKS, assignment=None, assign_total=None)
    status, win = tc.check(m, n, max_tasks, pts, None, mode, margin)
    if status != OK:
        return tc.Result(status, window=win, assignment=None, assign_total=None)
    P = 1 + 2 * n
    cells = [m.cell(x, y) for x, y in pts[:P]]
    mat = tc.cost_matrix(m, P, cells, win, safe_dis)
    fields = sum(len({tc.pair_safe(m, safe_dis, cells[k], cells[j]) for j in range(k + 1, P)}) for k in range(P - 1))
    res = tc.Result(OK, n=n, P=P, matrix=mat, fields=fields, window=win, assignment=None, assign_total=None)
    if mode == ASSIGNED:
        asg, carry = matching(mat, n)
        if asg is None:
            res.status = E_NO_ORDER
            return res
        res.assignment, res.assign_total = asg, carry
        seq, total = tc.held_karp(mat, n, asg)
        if seq is None:
            res.status = E_NO_ORDER
            return res
        res.order, res.total = [v for i in seq for v in (i, asg[i])], total
    else:
        order, total = joint(mat, n)
        if order is None:
            res.status = E_NO_ORDER
            return res
        res.order, res.total = order, total
        res.assignment = [order[2 * order[0::2].index(i) + 1] for i in range(n)]
        res.assign_total = carry_sum(mat, n, res.assignment)
    at = 0
    for e, v in enumerate(res.order):
        nxt = n + 1 + v if e & 1 else 1 + v
        res.legs.append((pts[at], pts[nxt]))
        at = nxt
    return res


def expected_arrays(r):
    """what a pre-filled row of both slabs holds after the mission"""
    out = tc.expected_arrays(r)
    out["assignment"], out["assign_total"] = np.full(MAX_TASKS, FILL_I, np.int32), np.full(2, FILL_I, np.int32)
    if r.assignment is not None:
        out["assignment"][:r.n] = r.assignment
        out["assign_total"][:] = r.assign_total
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def _with_mode(s, mode, **kw):
    return {**s, "mode": mode, **kw}


# found by search_joint_beats_assigned(): the cheapest carry legs send the robot the long way round between them
JOINT_BEATS_ASSIGNED = [(39, 38), (55, 14), (48, 32), (53, 41), (16, 20), (51, 15), (28, 24)]   # cells: robot, items, targets


def search_joint_beats_assigned(seed=20261020, tries=400):
    """the seeded search the literal coordinates of the scene "joint_beats_assigned" come from: three tasks on the open map"""
    rng = np.random.default_rng(seed)
    occ = np.zeros((tc.NX, tc.NY), bool)
    m = ps.Map(ps.brute_dist(occ), tc.X_LO, tc.Y_LO, tc.RES)
    for _ in range(tries):
        cells = [(int(rng.integers(6, tc.NX - 6)), int(rng.integers(6, tc.NY - 6))) for _ in range(7)]
        if len(set(cells)) < 7:
            continue
        pts = [pt(x, y) for x, y in cells]
        a, j = plan(m, 3, 3, pts, ASSIGNED), plan(m, 3, 3, pts, JOINT)
        if a.status == OK and j.status == OK and less(j.total, a.total):
            return cells
    return None


@functools.lru_cache(maxsize=None)
def scene(name):
    """name: "<kind>:<assigned|joint>"; the dictionaries of task_plan_cases._scene"""
    kind, _, arg = name.partition(":")
    mode = MODE_NAMES[arg]
    occ = np.zeros((tc.NX, tc.NY), bool)
    if kind == "crossed":           # the geometry of task_plan_cases "differ" with the two targets exchanged: the identity crosses
        ms = tc.mission(2, pt(10, 24), [pt(14, 26), pt(4, 22)], [pt(2, 25), pt(60, 20)])
        return tc._scene(occ, [ms], mode=mode)
    if kind == "mirror":            # task_plan_cases "mirror": every item below its own target, the order ties at the second step
        return _with_mode(tc.scene("mirror:optimal"), mode)
    if kind == "tie":               # items 1 and 2 mirror images, targets 0 and 2 on the axis: [1, 0, 2] and [1, 2, 0] carry equally far
        ms = tc.mission(3, pt(32, 4), [pt(32, 10), pt(22, 30), pt(42, 30)], [pt(32, 44), pt(32, 14), pt(32, 36)])
        return tc._scene(occ, [ms], mode=mode)
    if kind == "joint_beats_assigned":
        c = JOINT_BEATS_ASSIGNED
        return tc._scene(occ, [tc.mission(3, pt(*c[0]), [pt(*v) for v in c[1:4]], [pt(*v) for v in c[4:7]])], mode=mode)
    if kind == "box":               # target 0 inside a closed box: no bijection has a finite sum
        return _with_mode(tc.scene("box:3"), mode)
    if kind == "unroutable":        # the robot inside the closed box: every carry leg is finite, no leg from the robot is
        s = tc.scene("box:3")
        ms = tc.mission(2, pt(45, 25), tc.ITEMS, s["missions"][0]["pts"][5:7])
        return _with_mode(s, mode, missions=[ms])
    if kind == "too_many":          # six tasks in a row for ten, the same with a NaN point, five tasks in a row for ten
        six = [tc.ROBOT] + tc.ITEMS[:6] + tc.TARGETS[:6]
        five = [tc.ROBOT] + tc.ITEMS[:5] + tc.TARGETS[:5]
        nan = float("nan")
        return tc._scene(occ, [dict(n=6, pts=six, assign=None, max_tasks=10), dict(n=6, pts=six[:3] + [(nan, nan)] + six[4:], assign=None, max_tasks=10),
                               dict(n=5, pts=five, assign=None, max_tasks=10)], mode=mode)
    if kind == "ignored_assignment":  # assignments that the optimal mode refuses: these modes do not read them
        good = [tc.ROBOT] + tc.ITEMS[:2] + tc.TARGETS[:2]
        return tc._scene(occ, [dict(n=2, pts=good, assign=[0, 0], max_tasks=2), dict(n=2, pts=good, assign=[7, -1], max_tasks=2)], mode=mode)
    raise KeyError(name)


KINDS = ("crossed", "mirror", "tie", "joint_beats_assigned", "box", "unroutable", "too_many", "ignored_assignment")
SCENES = tuple("%s:%s" % (k, a) for k in KINDS for a in ("assigned", "joint"))

RANDOM_MISSIONS, RANDOM_T, JOINT_SEED = tc.RANDOM_MISSIONS, tc.RANDOM_T, 20261020


@functools.lru_cache(maxsize=None)
def random_scene(mode):
    """ASSIGNED: the 64 missions of task_plan_cases.random_scene(GREEDY), n up to 10.  JOINT: 64 missions of the same making on the
    same map, n drawn from 1..5, a seed of their own"""
    base = tc.random_scene(GREEDY)
    if mode == ASSIGNED:
        return _with_mode(base, ASSIGNED)
    rng, m, missions = np.random.default_rng(JOINT_SEED), base["map"], []
    for _ in range(RANDOM_MISSIONS):
        n = int(rng.integers(1, JOINT_MAX_TASKS + 1))
        clear = rng.random() < 0.8
        pts = []
        while len(pts) < 1 + 2 * n:
            x, y = float(rng.uniform(m.x_lo, m.x_hi)), float(rng.uniform(m.y_lo, m.y_hi))
            if not clear or m.dist[m.cell(x, y)] >= 0.4:
                pts.append((x, y))
        missions.append(dict(n=n, pts=pts, assign=None, max_tasks=RANDOM_T))
    return _with_mode(base, JOINT, missions=missions)


def get_scene(name):
    return random_scene(name[1]) if isinstance(name, tuple) else scene(name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's results of a scene (name, or ("random", mode)), computed once"""
    s = get_scene(name)
    return tuple(plan(s["map"], ms["n"], s["max_tasks"], ms["pts"], s["mode"], s["safe_dis"], s["margin"]) for ms in s["missions"])


arrays = tc.arrays
