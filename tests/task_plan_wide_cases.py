"""The contract of csrc/task_plan.h for missions on windows beyond LDS (paragraph WIDE; alore_backend_task_reserve) as a sequential
oracle, and the scenes the CPU harness and the GPU are compared on.

plan_wide() is tests/task_plan_cases.plan and tests/task_assign_cases.plan -- all four modes -- with the cap on the window as an
argument, plus the range rule.  The fields come from the same Dijkstra on exact integer pairs (task_plan_cases._field), but ROOTED AS
THE CONTRACT ROOTS THEM: at the cell of source k, with safe_kj, for the targets j > k; a field is empty where that cell is not
free.  (task_plan_cases roots a pair's field at j and reads it at i; the costs are the same, the graph is symmetric, but the range
flag is a property of the root.)  A mission is E_RANGE if any field it computes -- one per source k < P - 1 and distinct safe_kj,
whether or not a target shares the source's cell -- holds a cost with a component of 32767 or more: decided from the Dijkstra
fields, which know nothing of tiles or of refused extensions.  The orders, tie rules and legs are those modules' own functions.
Everything is compared with ==; the matrix of an E_RANGE mission is unspecified and not compared."""
import functools

import numpy as np

from tests import path_search_cases as ps
from tests import path_search_wide_cases as wide
from tests import task_assign_cases as ta
from tests import task_plan_cases as tc

MAX_TASKS, P_MAX, MAX_LEGS = tc.MAX_TASKS, tc.P_MAX, tc.MAX_LEGS
OK, MASKED, E_ENDPOINT, E_WINDOW, E_TASKS, E_NO_ORDER = tc.OK, tc.MASKED, tc.E_ENDPOINT, tc.E_WINDOW, tc.E_TASKS, tc.E_NO_ORDER
E_RANGE = -8
GREEDY, OPTIMAL, ASSIGNED, JOINT = ta.GREEDY, ta.OPTIMAL, ta.ASSIGNED, ta.JOINT
MODES = (GREEDY, OPTIMAL, ASSIGNED, JOINT)
MODE_IDS = ("greedy", "optimal", "assigned", "joint")
INF, FILL_I, FILL_D = tc.INF, tc.FILL_I, tc.FILL_D
RANGE_LIMIT, RESERVED, WIDE_MAX_CELLS = wide.RANGE_LIMIT, wide.RESERVED, wide.WIDE_MAX_CELLS
less, add = tc.less, tc.add


def check_wide(m, n, max_tasks, pts, assign, mode, margin, max_cells):
    """task_plan_cases.check with the cap as an argument: the order of the checks is unchanged"""
    status, win = tc.check(m, n, max_tasks, pts, assign, mode, margin)
    if status != E_WINDOW:
        return status, win
    x0, y0, x1, y1 = win
    return (E_WINDOW if (x1 - x0 + 1) * (y1 - y0 + 1) > max_cells else OK), win


def window_cells(r):
    x0, y0, x1, y1 = r.window
    return (x1 - x0 + 1) * (y1 - y0 + 1)


def rooted_matrix(m, P, cells, win, safe_dis):
    """(matrix, number of fields, range flag): one field per source k < P - 1 and distinct safe_kj, rooted at the cell of k"""
    mat = {(i, i): (0, 0) for i in range(P)}
    n_fields, out_of_range = 0, False
    for k in range(P - 1):
        seen = set()
        for j in range(k + 1, P):
            safe = tc.pair_safe(m, safe_dis, cells[k], cells[j])
            field = tc._field(m, win, safe, cells[k])
            if safe not in seen:
                seen.add(safe)
                n_fields += 1
                out_of_range |= _flag(m, win, safe, cells[k])
            mat[k, j] = mat[j, k] = (0, 0) if cells[k] == cells[j] else field.get(cells[j], INF)
    return mat, n_fields, out_of_range


_flags = {}


def _flag(m, win, safe, root):
    key = (id(m), win, safe, root)
    if key not in _flags:
        _flags[key] = any(a >= RANGE_LIMIT or b >= RANGE_LIMIT for a, b in tc._field(m, win, safe, root).values())
    return _flags[key]


def plan_wide(m, n, max_tasks, pts, assign=None, mode=GREEDY, safe_dis=ps.SAFE_DIS, margin=ps.MARGIN, max_cells=RESERVED):
    """one mission in any of the four modes: a task_plan_cases.Result with assignment and assign_total (None where the contract
    leaves the rows untouched).  A given assignment is read in the optimal mode only"""
    pts = [(float(x), float(y)) for x, y in pts]
    none = dict(assignment=None, assign_total=None)
    if mode == JOINT and n > ta.JOINT_MAX_TASKS:
        return tc.Result(E_TASKS, **none)
    status, win = check_wide(m, n, max_tasks, pts, assign if mode == OPTIMAL else None, mode, margin, max_cells)
    if status != OK:
        return tc.Result(status, window=win, **none)
    P = 1 + 2 * n
    cells = [m.cell(x, y) for x, y in pts[:P]]
    mat, n_fields, out_of_range = rooted_matrix(m, P, cells, win, safe_dis)
    res = tc.Result(OK, n=n, P=P, matrix=mat, fields=n_fields, window=win, **none)
    if out_of_range:                                                       # after the matrix, before any ordering
        res.status = E_RANGE
        return res
    if mode == GREEDY:
        res.order, res.total = tc.greedy(mat, n)
    elif mode == JOINT:
        order, total = ta.joint(mat, n)
        if order is None:
            res.status = E_NO_ORDER
            return res
        res.order, res.total = order, total
        res.assignment = [order[2 * order[0::2].index(i) + 1] for i in range(n)]
        res.assign_total = ta.carry_sum(mat, n, res.assignment)
    else:
        if mode == ASSIGNED:
            asg, carry = ta.matching(mat, n)
            if asg is None:
                res.status = E_NO_ORDER
                return res
            res.assignment, res.assign_total = asg, carry
        else:
            asg = list(assign[:n]) if assign is not None else list(range(n))
        seq, total = tc.held_karp(mat, n, asg)
        if seq is None:
            res.status = E_NO_ORDER
            return res
        res.order, res.total = [v for i in seq for v in (i, asg[i])], total
    at = 0
    for e, v in enumerate(res.order):
        nxt = n + 1 + v if e & 1 else 1 + v
        res.legs.append((pts[at], pts[nxt]))
        at = nxt
    return res


def expected_arrays(r):
    """what a pre-filled row of both slabs holds after the mission; "matrix" is None where it is unspecified (E_RANGE)"""
    out = ta.expected_arrays(r)
    if r.status == E_RANGE:
        out["matrix"] = None
    return out


# ---- scenes: the maps of tests/path_search_wide_cases.py, 0.1 m, a reservation of RESERVED cells --------------------------------
def _ms(m, n, cells, assign=None, max_tasks=None):
    """a mission from cells: robot, n items, n targets"""
    return tc.mission(n, wide.cell_pt(m, *cells[0]), [wide.cell_pt(m, *c) for c in cells[1:1 + n]],
                      [wide.cell_pt(m, *c) for c in cells[1 + n:1 + 2 * n]], assign=assign, max_tasks=max_tasks)


def _scene(m, missions, mode, safe_dis=ps.SAFE_DIS, margin=ps.MARGIN, mask=None, reserved=RESERVED):
    s = tc._scene(None, missions, mode=mode, safe_dis=safe_dis, margin=margin, m=m)
    s["mask"], s["reserved"] = mask, reserved
    return s


def near_wall_cells(m):
    """the first and the last cell, in scan order, between 0.15 m and 0.3 m from an obstacle of the boxes map and at least 12 cells
    from the map's edge: 0.8 dist caps the safe distance of their pairs below safe_dis, differently for the two"""
    d = m.dist
    c = [(int(x), int(y)) for x, y in np.argwhere((d > 0.15) & (d < 0.3)) if 12 <= x < d.shape[0] - 12 and 12 <= y < d.shape[1] - 12]
    a = c[0]
    b = next(v for v in reversed(c) if float(d[v]) != float(d[a]))
    return a, b


@functools.lru_cache(maxsize=None)
def scene(name):
    if name in ("boxes", "mixed"):
        m = wide.wide_scene("boxes")["map"]
        a, b = near_wall_cells(m)
        one = _ms(m, 1, [(3, 3), (256, 196), (256, 3)], max_tasks=3)                   # corner to corner: the whole map, 52 000 cells
        three = _ms(m, 3, [(3, 3), (256, 196), (30, 15), (215, 150), (3, 196), (200, 185), (256, 3)], assign=[1, 2, 0], max_tasks=3)
        narrow = _ms(m, 1, [(5, 10), (15, 90), (12, 50)], max_tasks=3)                 # 46 x 121 cells: the LDS route in the same call
        walls = _ms(m, 1, [a, (256, 196), b], max_tasks=3)                             # safe_kj differs within source 0
        if name == "boxes":
            return _scene(m, [one, three, narrow, walls], OPTIMAL)
        nan = float("nan")
        no_tasks = dict(one, n=0)
        bad_point = dict(three, pts=three["pts"][:2] + [(nan, 0.0)] + three["pts"][3:])
        return _scene(m, [one, three, no_tasks, walls, bad_point, narrow, three], GREEDY, mask=[1, 0, 1, 1, 1, 1, 1])
    if name == "open":                                                                  # one field per source, all 20 sources
        m = wide._map(np.full((wide.NX, wide.NY), 10.0))
        cells = [(130, 100)] + [(8 + 3 * i, 12 + 19 * i) for i in range(10)] + [(250 - 4 * i, 190 - 18 * ((3 * i) % 10)) for i in range(10)]
        return _scene(m, [_ms(m, 10, cells)], ASSIGNED)
    if name == "comb":                                                                  # the field crosses tile borders many times
        m = wide.wide_scene("comb")["map"]
        return _scene(m, [_ms(m, 1, [(5, 100), (255, 100), (130, 100)])], GREEDY, margin=10.0)
    if name == "closed":                                                                # the robot and item 0 inside the closed box
        m = wide.wide_scene("closed")["map"]
        return _scene(m, [_ms(m, 2, [(210, 160), (215, 165), (20, 150), (100, 50), (60, 120)])], GREEDY, safe_dis=0.05)
    if name == "edge":                              # 256 x 128 = 32768 cells, the last LDS window, and 257 x 128, the first wide one
        m = wide.wide_scene("edge")["map"]
        return _scene(m, [_ms(m, 1, [(40, 40), (235, 107), (100, 60)]), _ms(m, 1, [(40, 40), (236, 107), (100, 60)])], OPTIMAL)
    if name == "serpentine_range":                  # a route exists, its cost does not fit the packed word
        m = wide.wide_scene("serpentine_range")["map"]
        return _scene(m, [_ms(m, 1, [(0, 0), (299, 239), (298, 0)])], GREEDY, safe_dis=0.05, margin=10.0)
    raise KeyError(name)


WIDE_SCENES = ("boxes", "open", "comb", "closed", "edge", "serpentine_range", "mixed")


@functools.lru_cache(maxsize=None)
def expected(name, mode=None, max_cells=None):
    """the oracle's results of a wide scene in `mode` (None: the scene's own) under a reservation of max_cells cells (None: the
    scene's), computed once; a masked-out mission is a Result with status MASKED"""
    s = scene(name)
    mode = s["mode"] if mode is None else mode
    cap = s["reserved"] if max_cells is None else max_cells
    mask = s["mask"] or [1] * len(s["missions"])
    return tuple(plan_wide(s["map"], ms["n"], s["max_tasks"], ms["pts"], ms["assign"], mode, s["safe_dis"], s["margin"], cap) if on
                 else tc.Result(MASKED, assignment=None, assign_total=None) for ms, on in zip(s["missions"], mask))


def arrays(s):
    """task_plan_cases.arrays; the assignment always as an array (the identity where a mission gives none)"""
    n_tasks, pts, asg = tc.arrays(s)
    if asg is None:
        asg = np.tile(np.arange(s["max_tasks"], dtype=np.int32), (len(n_tasks), 1))
    else:
        for k, q in enumerate(s["missions"]):
            if q["assign"] is None:
                asg[k] = np.arange(s["max_tasks"])
    return n_tasks, pts, asg
