"""The contract of csrc/path_search.h as a sequential oracle, and the scenes the CPU harness and the GPU are compared on.

The oracle has the reference's shape (JPSPlanner::plan, removeCornerPts): one problem at a time, the field by Dijkstra with a
heap (`heapq`) on exact pair costs -- not by sweeps --, then the walk by the written tie rule and the pruning.  A cost is the
integer pair (a, b) for a + b sqrt 2; pairs are ordered exactly in integers (the sign of da + db sqrt 2 is the sign of
da |da| + 2 db |db|), the heap's float key a + b * SQRT2 only sorts the heap and is asserted to agree.  Everything that ends up
in a result is a correctly rounded double operation written as the header writes it, so results are compared with ==.

check_result() is a second, independent check of a result: the raw path is connected, free and inside the window, its pair equals
the field's value at the start, and the way-points are a subsequence of the raw nodes."""
import functools
import heapq
import math

import numpy as np

MAX_CELLS, MAX_NODES, K = 32768, 1024, 31
OK, MASKED, E_ENDPOINT, E_SAME_CELL, E_WINDOW, E_NO_PATH, E_POINTS = 0, 1, -1, -2, -3, -4, -5
DIRS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
SQRT2 = 1.4142135623730951
SAFE_DIS, MARGIN = 0.3, 3.0
SENTINEL = -777.0


class Map:
    def __init__(self, dist, x_lo, y_lo, res):
        self.dist = np.ascontiguousarray(dist, np.float64)
        self.nx, self.ny = self.dist.shape
        self.x_lo, self.y_lo, self.res = float(x_lo), float(y_lo), float(res)
        self.x_hi, self.y_hi = self.x_lo + self.nx * self.res, self.y_lo + self.ny * self.res
        self.inv = 1 / self.res

    def cell(self, x, y):
        return cell_1d(x, self.x_lo, self.inv, self.nx), cell_1d(y, self.y_lo, self.inv, self.ny)

    def centre(self, ix, iy):
        return (float(ix) + 0.5) * self.res + self.x_lo, (float(iy) + 0.5) * self.res + self.y_lo


def cell_1d(p, lo, inv, n):
    v = (p - lo) * inv
    if not v > 0.0:
        return 0
    if v >= float(n):
        return n - 1
    return int(v)


def less(p, q):
    """a_p + b_p sqrt 2 < a_q + b_q sqrt 2, exactly"""
    da, db = p[0] - q[0], p[1] - q[1]
    return da * abs(da) + 2 * db * abs(db) < 0


def key(p):
    return float(p[0]) + float(p[1]) * SQRT2


def std_min(a, b):
    return b if b < a else a


def std_max(a, b):
    return b if a < b else a


class Result:
    def __init__(self, status, **kw):
        self.status, self.n_points, self.xy, self.cost = status, 0, [], None
        self.raw, self.field, self.window, self.safe = [], {}, None, None
        self.__dict__.update(kw)


def setup(m, s, g, safe_dis, margin):
    """status, window (x0, y0, x1, y1), start cell, goal cell, safe"""
    if not all(math.isfinite(v) for v in (*s, *g)):
        return E_ENDPOINT, None, None, None, None
    for x, y in (s, g):
        if x < m.x_lo or x > m.x_hi or y < m.y_lo or y > m.y_hi:
            return E_ENDPOINT, None, None, None, None
    sc, gc = m.cell(*s), m.cell(*g)
    if sc == gc:
        return E_SAME_CELL, None, sc, gc, None
    md = math.ceil(margin / m.res)
    md = min(max(md, 0), 10 ** 9)
    x0, x1 = max(min(sc[0], gc[0]) - md, 0), min(max(sc[0], gc[0]) + md, m.nx - 1)
    y0, y1 = max(min(sc[1], gc[1]) - md, 0), min(max(sc[1], gc[1]) + md, m.ny - 1)
    win = (x0, y0, x1, y1)
    if (x1 - x0 + 1) * (y1 - y0 + 1) > MAX_CELLS:
        return E_WINDOW, win, sc, gc, None
    ds, dg = float(m.dist[sc]), float(m.dist[gc])
    safe = std_max(std_min(safe_dis, 0.8 * ds), 0.0)
    safe = std_max(std_min(safe, 0.8 * dg), 0.0)
    if ds < safe or dg < safe:
        return E_NO_PATH, win, sc, gc, safe
    return OK, win, sc, gc, safe


def dijkstra(free, goal):
    """free: {cell}; returns {cell: (a, b)}, the least cost to the goal"""
    g = {goal: (0, 0)}
    done = set()
    heap = [(0.0, 0, 0, goal)]
    while heap:
        k, a, b, c = heapq.heappop(heap)
        if c in done:
            continue
        assert g[c] == (a, b) and k == key((a, b))
        done.add(c)
        for i, (dx, dy) in enumerate(DIRS):
            n = (c[0] + dx, c[1] + dy)
            if n not in free or n in done:
                continue
            new = (a, b + 1) if i & 1 else (a + 1, b)
            old = g.get(n)
            if old is None or less(new, old):
                assert old is None or key(new) < key(old)  # the float order agrees with the exact one
                g[n] = new
                heapq.heappush(heap, (key(new), new[0], new[1], n))
    return g


def line_cells(a, b):
    """JPSPlanner::getGridsBetweenPoints2D"""
    dx, dy = abs(b[0] - a[0]), abs(b[1] - a[1])
    sx, sy = (1 if a[0] < b[0] else -1), (1 if a[1] < b[1] else -1)
    err = dx - dy
    x, y = a
    out = []
    while True:
        out.append((x, y))
        if (x, y) == tuple(b):
            return out
        e2 = 2 * err
        if e2 > -dy:
            err -= dy
            x += sx
        if e2 < dx:
            err += dx
            y += sy


def search(m, s, g, safe_dis=SAFE_DIS, margin=MARGIN):
    s, g = (float(s[0]), float(s[1])), (float(g[0]), float(g[1]))
    status, win, sc, gc, safe = setup(m, s, g, safe_dis, margin)
    if status != OK:
        return Result(status, window=win, safe=safe)
    x0, y0, x1, y1 = win
    sub = m.dist[x0:x1 + 1, y0:y1 + 1]
    free = {(x0 + int(i), y0 + int(j)) for i, j in np.argwhere(~(sub < safe))}
    field = dijkstra(free, gc)
    res = Result(E_NO_PATH, window=win, safe=safe, field=field, free=free)
    if sc not in field:
        return res
    # the walk
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
    # removeCornerPts
    pts = [s] + [m.centre(*c) for c in raw[1:-1]] + [g]
    for p, c in zip(pts, raw):
        assert m.cell(*p) == c  # coord2gridIndex of a way-point is its node's cell

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


def check_result(m, s, g, r):
    """the second check: nothing of it uses the walk or the heap"""
    if r.status != OK and not r.raw:
        return
    x0, y0, x1, y1 = r.window
    a = b = 0
    for p, q in zip(r.raw[:-1], r.raw[1:]):
        dx, dy = q[0] - p[0], q[1] - p[1]
        n = max(abs(dx), abs(dy))
        assert n >= 1 and (dx == 0 or dy == 0 or abs(dx) == abs(dy)), (p, q)   # a straight run in one of the eight directions
        ux, uy = dx // n, dy // n
        for k in range(1, n + 1):
            c = (p[0] + k * ux, p[1] + k * uy)
            assert x0 <= c[0] <= x1 and y0 <= c[1] <= y1 and not m.dist[c] < r.safe, c
        if ux and uy:
            b += n
        else:
            a += n
    assert (a, b) == r.field[r.raw[0]] and r.raw[0] == m.cell(*s) and r.raw[-1] == m.cell(*g)
    for i in range(1, len(r.raw) - 1):                                          # the direction changes at every interior raw node
        p, c, q = r.raw[i - 1], r.raw[i], r.raw[i + 1]
        assert np.sign(c[0] - p[0]) != np.sign(q[0] - c[0]) or np.sign(c[1] - p[1]) != np.sign(q[1] - c[1])
    if r.status == OK:
        assert (a, b) == r.cost and 2 <= r.n_points <= K
        assert r.xy[0] == (float(s[0]), float(s[1])) and r.xy[-1] == (float(g[0]), float(g[1]))
        centres = [m.centre(*c) for c in r.raw[1:-1]]
        at = 0
        for p in r.xy[1:-1]:                                                     # a subsequence of the raw nodes' centres
            at = centres.index(p, at) + 1
        lower = math.hypot(g[0] - s[0], g[1] - s[1])
        length = sum(math.hypot(q[0] - p[0], q[1] - p[1]) for p, q in zip(r.xy[:-1], r.xy[1:]))
        assert lower - 1e-9 <= length <= (key(r.cost) + 2.0) * m.res + 1e-9       # no longer than the grid path and the two end offsets


# ---- scenes ----------------------------------------------------------------------------------------------------------------
NX, NY, RES = 64, 48, 0.1
X_LO, Y_LO = -3.2, -2.4


def brute_dist(occ, res=RES, free_value=10.0):
    """distance from every cell centre to the nearest occupied cell's centre, by brute force; free_value without obstacles"""
    occ = np.asarray(occ, bool)
    o = np.argwhere(occ)
    if not len(o):
        return np.full(occ.shape, free_value)
    ix, iy = np.meshgrid(np.arange(occ.shape[0]), np.arange(occ.shape[1]), indexing="ij")
    d2 = np.full(occ.shape, np.iinfo(np.int64).max, np.int64)
    for k in range(0, len(o), 256):
        blk = o[k:k + 256]
        d2 = np.minimum(d2, ((ix[..., None] - blk[:, 0]) ** 2 + (iy[..., None] - blk[:, 1]) ** 2).min(-1))
    return np.sqrt(d2.astype(np.float64)) * res


def pt(ix, iy, fx=0.5, fy=0.5):
    """a point in cell (ix, iy) of the small map, at the fraction (fx, fy) of the cell"""
    return (X_LO + (ix + fx) * RES, Y_LO + (iy + fy) * RES)


def _scene(occ, problems, safe_dis=SAFE_DIS, margin=MARGIN):
    return {"map": Map(brute_dist(occ), X_LO, Y_LO, RES), "problems": problems, "safe_dis": safe_dis, "margin": margin}


def _spiral(pitch=4):
    """nested rectangular rings of one-cell walls, four cells apart, each with a one-cell door: at the bottom for even rings, at
    the top for odd ones, so the way to the centre goes half round every ring"""
    occ = np.zeros((NX, NY), bool)
    k = 0
    while (NY - 2 - pitch * k) - (1 + pitch * k) >= 6:
        x0, y0, x1, y1 = 1 + pitch * k, 1 + pitch * k, NX - 2 - pitch * k, NY - 2 - pitch * k
        occ[x0:x1 + 1, y0] = occ[x0:x1 + 1, y1] = True
        occ[x0, y0:y1 + 1] = occ[x1, y0:y1 + 1] = True
        occ[NX // 2, y1 if k % 2 else y0] = False
        k += 1
    return occ


def _serpentine():
    occ = np.zeros((NX, NY), bool)
    for k, x in enumerate(range(3, NX - 3, 3)):
        if k % 2:
            occ[x, 0:NY - 3] = True
        else:
            occ[x, 3:NY] = True
    return occ


@functools.lru_cache(maxsize=None)
def scene(name):
    occ = np.zeros((NX, NY), bool)
    if name == "open":
        return _scene(occ, [(pt(7, 7, 0.3, 0.8), pt(52, 35, 0.9, 0.1)), (pt(60, 3), pt(60, 44)), (pt(5, 40), pt(40, 5))])
    if name == "wall_gap":
        occ[32, :] = True
        occ[32, 30:39] = False
        return _scene(occ, [(pt(10, 8), pt(55, 10)), (pt(55, 40, 0.1, 0.2), pt(8, 4))])
    if name == "spiral":
        return _scene(_spiral(), [(pt(0, 0), pt(NX // 2, NY // 2)), (pt(NX // 2, NY // 2), pt(0, 0))], safe_dis=0.05)
    if name == "box":
        occ[40:51, 20] = occ[40:51, 30] = True
        occ[40, 20:31] = occ[50, 20:31] = True
        return _scene(occ, [(pt(5, 5), pt(45, 25))], safe_dis=0.05)
    if name == "corner":
        occ[5, 0:4] = True
        return _scene(occ, [(pt(1, 2), pt(9, 1)), (pt(62, 46), pt(57, 40))], safe_dis=0.05)
    if name == "detour":            # the way round the wall needs more than three cells of margin
        occ[32, 0:25] = True
        return _scene(occ, [(pt(27, 4), pt(37, 4))])
    if name == "detour_tight":
        s = scene("detour")
        return {**s, "margin": 0.3}
    if name == "safe_rule":         # the start is two cells from a wall: 0.8 * 0.2 caps the safe distance
        occ[20, 10:40] = True
        return _scene(occ, [(pt(22, 20), pt(50, 30)), (pt(50, 30), pt(18, 25))])
    if name == "bad":               # the same cell, a NaN, outside the map on every side, an infinity
        nan, inf = float("nan"), float("inf")
        return _scene(occ, [(pt(10, 10, 0.1, 0.1), pt(10, 10, 0.9, 0.9)), ((nan, 0.0), pt(5, 5)), (pt(5, 5), (0.0, nan)),
                            ((X_LO - 0.01, 0.0), pt(5, 5)), (pt(5, 5), (0.0, Y_LO + NY * RES + 0.01)), ((inf, 0.0), pt(5, 5)),
                            (pt(5, 5), pt(30, 30))])
    if name == "serpentine":
        return _scene(_serpentine(), [(pt(0, 0), pt(NX - 1, NY - 1)), (pt(0, 0), pt(13, 40))], safe_dis=0.05)
    if name == "window":            # 400 x 100 cells: the window of end points 380 cells apart has 400 x 100 cells
        m = Map(np.full((400, 100), 10.0), -20.0, -5.0, RES)
        return {"map": m, "problems": [((-19.05, -2.05), (18.95, 1.95)), ((-19.05, -2.05), (-15.05, 1.95))], "safe_dis": SAFE_DIS, "margin": MARGIN}
    raise KeyError(name)


SCENES = ("open", "wall_gap", "spiral", "box", "corner", "detour", "detour_tight", "safe_rule", "bad", "serpentine", "window")
RANDOM_FIELDS, RANDOM_PER_FIELD = 4, 50


@functools.lru_cache(maxsize=None)
def random_scene(k):
    """field k of the random scenes: box obstacles, 50 problems with end points anywhere in the map"""
    rng = np.random.default_rng(20261018 + k)
    occ = np.zeros((NX, NY), bool)
    for _ in range(7):
        w, h = rng.integers(2, 9, 2)
        x, y = rng.integers(0, NX - w), rng.integers(0, NY - h)
        occ[x:x + w, y:y + h] = True
    problems = []
    for _ in range(RANDOM_PER_FIELD):
        p = rng.uniform([X_LO, Y_LO, X_LO, Y_LO], [X_LO + NX * RES, Y_LO + NY * RES, X_LO + NX * RES, Y_LO + NY * RES])
        problems.append(((float(p[0]), float(p[1])), (float(p[2]), float(p[3]))))
    return _scene(occ, problems, margin=float(rng.choice([0.5, 1.0, 3.0])))


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's results of a scene (name, or ("random", k)), computed once"""
    s = random_scene(name[1]) if isinstance(name, tuple) else scene(name)
    return tuple(search(s["map"], a, b, s["safe_dis"], s["margin"]) for a, b in s["problems"])


def get_scene(name):
    return random_scene(name[1]) if isinstance(name, tuple) else scene(name)


def random_no_path_share():
    res = [r for k in range(RANDOM_FIELDS) for r in expected(("random", k))]
    return sum(r.status == E_NO_PATH for r in res) / len(res), res
