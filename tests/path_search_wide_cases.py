"""The contract of csrc/path_search_wide.h as a sequential oracle, and the scenes that take the wide route of
alore_backend_search_paths (windows of more than 32768 cells, after alore_backend_search_reserve).

search_wide() is tests/path_search_cases.search with the cap on the window as an argument, plus the range rule: the field comes
from the same Dijkstra on exact integer pairs, and if any cell the goal reaches has a least cost with a component of 32767 or
more the status is E_RANGE -- decided from the Dijkstra field, which knows nothing of tiles or of refused extensions.  The walk
and the pruning are restated from that module's search(), operation for operation; tests/test_path_search_wide_cpu.py holds the
two against each other on every scene of that module.  That module's MAX_CELLS and its cached expected() are left alone."""
import functools
import math

import numpy as np

from tests.path_search_cases import (DIRS, E_ENDPOINT, E_NO_PATH, E_POINTS, E_SAME_CELL, E_WINDOW, K, MARGIN, MAX_CELLS, MAX_NODES, OK,  # noqa: F401
                                     SAFE_DIS, Map, Result, brute_dist, check_result, dijkstra, key, less, line_cells, setup, std_max,
                                     std_min)

E_RANGE = -6
RANGE_LIMIT = 32767
WIDE_MAX_CELLS = 1 << 22
RES = 0.1


def setup_wide(m, s, g, safe_dis, margin, max_cells):
    """setup with the cap as an argument: the order of the statuses is unchanged"""
    status, win, sc, gc, safe = setup(m, s, g, safe_dis, margin)
    if status != E_WINDOW:
        return status, win, sc, gc, safe
    x0, y0, x1, y1 = win
    if (x1 - x0 + 1) * (y1 - y0 + 1) > max_cells:
        return E_WINDOW, win, sc, gc, None
    ds, dg = float(m.dist[sc]), float(m.dist[gc])
    safe = std_max(std_min(safe_dis, 0.8 * ds), 0.0)
    safe = std_max(std_min(safe, 0.8 * dg), 0.0)
    if ds < safe or dg < safe:
        return E_NO_PATH, win, sc, gc, safe
    return OK, win, sc, gc, safe


def search_wide(m, s, g, safe_dis=SAFE_DIS, margin=MARGIN, max_cells=WIDE_MAX_CELLS):
    s, g = (float(s[0]), float(s[1])), (float(g[0]), float(g[1]))
    status, win, sc, gc, safe = setup_wide(m, s, g, safe_dis, margin, max_cells)
    if status != OK:
        return Result(status, window=win, safe=safe)
    x0, y0, x1, y1 = win
    sub = m.dist[x0:x1 + 1, y0:y1 + 1]
    free = {(x0 + int(i), y0 + int(j)) for i, j in np.argwhere(~(sub < safe))}
    field = dijkstra(free, gc)
    res = Result(E_RANGE, window=win, safe=safe, field=field, free=free)
    if any(a >= RANGE_LIMIT or b >= RANGE_LIMIT for a, b in field.values()):     # before the walk
        return res
    res.status = E_NO_PATH
    if sc not in field:
        return res
    raw, c, prev = [sc], sc, None
    while c != gc:
        pick = None
        for k in ([prev] if prev is not None else []) + list(range(8)):
            n = (c[0] + DIRS[k][0], c[1] + DIRS[k][1])
            if n in field:
                a, b = field[n]
                if ((a, b + 1) if k & 1 else (a + 1, b)) == field[c]:
                    pick = k
                    break
        assert pick is not None
        if c != sc and pick != prev:
            raw.append(c)
        c, prev = (c[0] + DIRS[pick][0], c[1] + DIRS[pick][1]), pick
    raw.append(gc)
    res.raw = raw
    if len(raw) > MAX_NODES:
        res.status = E_POINTS
        return res
    pts = [s] + [m.centre(*c) for c in raw[1:-1]] + [g]
    for p, c in zip(pts, raw):
        assert m.cell(*p) == c

    def blocked(i, j):
        return any(m.dist[c] < safe for c in line_cells(raw[i], raw[j]))

    def norm(i, j):
        dx, dy = pts[i][0] - pts[j][0], pts[i][1] - pts[j][1]
        return math.sqrt(dx * dx + dy * dy)

    def cost(i, j):
        return math.inf if blocked(i, j) else norm(i, j)

    out, prev_i = [pts[0]], 0
    cost1 = cost(0, 1)
    for i in range(1, len(pts) - 1):
        cost2, cost3 = cost(i, i + 1), cost(prev_i, i + 1)
        if cost3 < cost1 + cost2:
            cost1 = cost3
        else:
            out.append(pts[i])
            cost1 = norm(i, i + 1)
            prev_i = i
    out.append(pts[-1])
    if len(out) > K:
        res.status = E_POINTS
        return res
    res.status, res.n_points, res.xy, res.cost = OK, len(out), out, field[sc]
    return res


def window_cells(r):
    x0, y0, x1, y1 = r.window
    return (x1 - x0 + 1) * (y1 - y0 + 1)


# ---- scenes: all at 0.1 m, the map's origin at the centre --------------------------------------------------------------------
NX, NY = 260, 200
RESERVED = 80000           # cells of the reservation the scenes are searched with
SEED = 20261021


def _map(dist):
    nx, ny = dist.shape
    return Map(dist, -nx * RES / 2, -ny * RES / 2, RES)


def cell_pt(m, ix, iy, fx=0.5, fy=0.5):
    """a point in cell (ix, iy) of map m at the fraction (fx, fy) of the cell"""
    return (m.x_lo + (ix + fx) * m.res, m.y_lo + (iy + fy) * m.res)


def _pairs(m, cells):
    return [(cell_pt(m, *a), cell_pt(m, *b)) for a, b in cells]


def _boxes():
    """14 random boxes of 4 to 24 cells a side, at least 20 cells from the map's edge; distances to their perimeters.  The four
    corner-to-corner problems (52 000 cells: 3 x 2 tiles of 126 with ragged edges of 8 and 74), one 170-cell diagonal (46 200)
    and two problems with short windows that take the LDS route in the same call"""
    rng = np.random.default_rng(SEED)
    occ = np.zeros((NX, NY), bool)
    for _ in range(14):
        w, h = (int(v) for v in rng.integers(4, 25, 2))
        x, y = int(rng.integers(20, NX - 20 - w)), int(rng.integers(20, NY - 20 - h))
        occ[x:x + w, y] = occ[x:x + w, y + h - 1] = True
        occ[x, y:y + h] = occ[x + w - 1, y:y + h] = True
    m = _map(brute_dist(occ, RES))
    cells = [((3, 3), (256, 196)), ((256, 196), (3, 3)), ((256, 3), (3, 196)), ((3, 196), (256, 3)), ((30, 15), (200, 185)),
             ((5, 10), (15, 90)), ((250, 190), (215, 150))]
    return {"map": m, "problems": _pairs(m, cells), "safe_dis": SAFE_DIS, "margin": MARGIN, "occ": occ}


def _comb(margin):
    """six walls two cells thick, every 35 columns, from alternating sides, with gaps of 12 cells at the far side: the way from
    the left to the right edge at mid height goes up and down the whole map, and the field crosses the tile boundaries a dozen
    times in both directions.  It needs the 10 m margin; with 3 m the window is 260 x 61 cells and holds no gap"""
    occ = np.zeros((NX, NY), bool)
    for k, x in enumerate(range(35, 35 * 7, 35)):
        if k % 2:
            occ[x:x + 2, 12:NY] = True
        else:
            occ[x:x + 2, 0:NY - 12] = True
    m = _map(brute_dist(occ, RES))
    return {"map": m, "problems": _pairs(m, [((5, 100), (255, 100))]), "safe_dis": SAFE_DIS, "margin": margin}


def _closed():
    """a closed one-cell box round the goal, 29 x 29 cells inside: the goal reaches those 841 cells and no other"""
    occ = np.zeros((NX, NY), bool)
    gx, gy = 215, 165
    occ[gx - 15:gx + 16, gy - 15] = occ[gx - 15:gx + 16, gy + 15] = True
    occ[gx - 15, gy - 15:gy + 16] = occ[gx + 15, gy - 15:gy + 16] = True
    m = _map(brute_dist(occ, RES))
    return {"map": m, "problems": _pairs(m, [((10, 10), (gx, gy))]), "safe_dis": 0.05, "margin": MARGIN}


def _edge():
    """an open 400 x 160 map: end points (195, 67) cells apart have a window of 256 x 128 = 32768 cells, the last that takes the
    LDS route; (196, 67) apart 257 x 128 = 32 896 cells, the first that goes wide, in tiles of 126 + 126 + 5 by 126 + 2"""
    m = _map(np.full((400, 160), 10.0))
    return {"map": m, "problems": _pairs(m, [((40, 40), (235, 107)), ((40, 40), (236, 107))]), "safe_dis": SAFE_DIS, "margin": MARGIN}


def _serpentine_range():
    """300 x 240 cells, one-cell walls at every odd column up to 297 with one-cell doors alternating at y = 0 and y = 239: the way
    from corner to corner runs the length of every even column, some 35 000 steps, so the costs pass 32767 although the walk would
    find a path.  dist is 0 on the walls and 10.0 elsewhere: the search compares dist with the safe distance and nothing else,
    so a distance array need not be a true distance field"""
    dist = np.full((300, 240), 10.0)
    for k, x in enumerate(range(1, 298, 2)):
        dist[x, :] = 0.0
        dist[x, 239 if k % 2 else 0] = 10.0
    m = _map(dist)
    return {"map": m, "problems": _pairs(m, [((0, 0), (299, 239))]), "safe_dis": 0.05, "margin": 10.0}


WIDE_SCENES = ("boxes", "comb", "comb_tight", "closed", "edge", "serpentine_range")


@functools.lru_cache(maxsize=None)
def wide_scene(name):
    return {"boxes": _boxes, "comb": lambda: _comb(10.0), "comb_tight": lambda: _comb(3.0), "closed": _closed, "edge": _edge,
            "serpentine_range": _serpentine_range}[name]()


@functools.lru_cache(maxsize=None)
def wide_expected(name, max_cells=RESERVED):
    """the oracle's results of a wide scene under a reservation of max_cells cells, computed once"""
    s = wide_scene(name)
    return tuple(search_wide(s["map"], a, b, s["safe_dis"], s["margin"], max_cells) for a, b in s["problems"])
