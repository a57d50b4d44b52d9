"""The cases the ESDF construction (csrc/esdf_build.hip, oracle/backend_oracle.c: be_update_esdf2d) is compared on, shared by
tests/test_esdf_cases_cpu.py and tests/test_esdf_cases_gpu.py, and a plain reference of the same operation.

A geometry is (nx, ny, res, x_lo, y_lo, odom, range) with the window (min_x, min_y, max_x, max_y) it must produce, worked out by
hand from csrc/esdf_window.h and checked against the header by tests/test_esdf_window_cpu.py.  The windows are thin (X << Y,
Y << X, X = 1, Y = 1), clipped at each corner of the map, tiny, and one row and / or column past the map where
ceil((n res) (1 / res)) rounds up (n = 3, 48, 97, 101 at 0.1).  Every geometry gets the 14 contents of contents(): the ones that put
seeds, or none at all, on the window's first row and its first and last columns, where the reference's aliased scratch shows.

The reference (plain) uses no envelope algorithm: brute-force minima over exact integers.  It restates what the reference's
(X + 1) x (Y + 1) scratch with stride Y does when it is run sequentially: element Y of a row is element 0 of the next, so column
Y reads the row transform of column 0 one row down and its results land on column 0 one row down (alias=True).  alias=False is
the exact Euclidean transform, which differs from it in column 0 of the window, rows >= 1, and nowhere else."""
import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
NO_SEED = 1 << 40  # above every squared distance of a window (< 2^31), below the overflow of its sums in int64

_MAP = (64, 48, 0.1, -3.2, -2.4)

#            name         nx   ny   res   x_lo  y_lo   odom            range  window
GEOMETRIES = {
    "tall_whole": ((37, 150, 0.1, -1.0, -7.0, (0.0, 0.0), 1e3), (0, 0, 36, 149)),    # Y >> X
    "wide_whole": ((150, 37, 0.1, -7.0, -1.0, (0.0, 0.0), 1e3), (0, 0, 149, 36)),    # X >> Y
    "roundup_xy": ((101, 97, 0.1, -5.0, -4.0, (0.0, 0.0), 1e3), (0, 0, 101, 97)),    # a row and a column past the map
    "roundup_x": ((101, 40, 0.1, -5.0, -2.0, (0.0, 0.0), 1e3), (0, 0, 101, 39)),     # a row past the map
    "roundup_y": ((40, 97, 0.1, -2.0, -5.0, (0.0, 0.0), 1e3), (0, 0, 39, 97)),       # g[Y] is the next row's first cell
    "two_rows": ((2, 120, 0.1, 0.0, 0.0, (0.0, 0.0), 1e3), (0, 0, 1, 119)),          # X = 1
    "two_cols": ((120, 2, 0.1, 0.0, 0.0, (0.0, 0.0), 1e3), (0, 0, 119, 1)),          # Y = 1: every written cell is column 0
    "three_rows": ((3, 90, 0.1, 0.0, 0.0, (0.0, 0.0), 1e3), (0, 0, 3, 89)),          # the smallest rounded-up map
    "corner_ll": (_MAP + ((-2.9, -2.2), 2.0), (0, 0, 23, 21)),                       # clipped at each corner; ny = 48 rounds up
    "corner_ur": (_MAP + ((3.0, 2.3), 2.0), (42, 26, 63, 48)),
    "corner_ul": (_MAP + ((-3.0, 2.3), 2.0), (0, 26, 21, 48)),
    "corner_lr": (_MAP + ((3.0, -2.2), 2.0), (42, 0, 63, 21)),
    "tiny_mid": (_MAP + ((0.03, 0.04), 0.1), (31, 23, 33, 25)),                      # X = Y = 2
    "tiny_edge": (_MAP + ((3.15, 2.35), 0.12), (62, 46, 63, 48)),                    # X = 1, Y = 2 at the corner
    "res005": ((81, 63, 0.05, -2.0, -1.5, (0.3, -0.2), 1.3), (20, 0, 71, 51)),       # another resolution
}
NAMES = list(GEOMETRIES)
CONTENTS = ["free", "occupied", "unknown", "corner_00", "corner_0n", "corner_n0", "corner_nn", "col_first", "col_last", "row_first",
            "row_last", "hole", "checker", "random"]


def geometry(name):
    return GEOMETRIES[name][0]


def window(name):
    return GEOMETRIES[name][1]


def contents(nx, ny):
    """the 14 state grids uint8 [nx][ny] (0 unknown, 1 free, 2 occupied) by name, in the order of CONTENTS"""
    free = np.ones((nx, ny), np.uint8)
    out = {"free": free.copy(), "occupied": np.full((nx, ny), 2, np.uint8), "unknown": np.zeros((nx, ny), np.uint8)}
    for key, (x, y) in (("corner_00", (0, 0)), ("corner_0n", (0, ny - 1)), ("corner_n0", (nx - 1, 0)), ("corner_nn", (nx - 1, ny - 1))):
        out[key] = free.copy()
        out[key][x, y] = 2
    for key, sl in (("col_first", np.s_[:, 0]), ("col_last", np.s_[:, ny - 1]), ("row_first", np.s_[0, :]), ("row_last", np.s_[nx - 1, :])):
        out[key] = free.copy()
        out[key][sl] = 2
    out["hole"] = np.full((nx, ny), 2, np.uint8)
    out["hole"][nx // 2, ny // 2] = 1
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    out["checker"] = (1 + (x + y) % 2).astype(np.uint8)
    out["random"] = np.random.default_rng(5).choice([0, 1, 2], size=(nx, ny), p=[.1, .75, .15]).astype(np.uint8)
    assert list(out) == CONTENTS
    return out


def cases():
    """every (geometry name, content name, grid): 15 x 14 = 210"""
    for name in NAMES:
        nx, ny = geometry(name)[:2]
        for key, g in contents(nx, ny).items():
            yield name, key, g


def window_cells(grid, win):
    """the (X + 1) x (Y + 1) cells the construction reads: the grid flattened and followed by ny + 1 unknown cells, so that a y
    past the row's end is the next row's first cell, as in the code"""
    nx, ny = grid.shape
    min_x, min_y, max_x, max_y = win
    flat = np.concatenate([np.ascontiguousarray(grid, np.uint8).ravel(), np.zeros(ny + 1, np.uint8)])
    idx = (np.arange(min_x, max_x + 1)[:, None]) * ny + np.arange(min_y, max_y + 1)[None, :]
    assert idx.max() < flat.size
    return flat[idx]


def _transform(seed, res, alias):
    """res sqrt(squared distance to the nearest seed) on the (X + 1) x (Y + 1) window, DBL_MAX under the root where no seed is
    in reach; with `alias`, column 0 as the stride-Y scratch leaves it"""
    X, Y = seed.shape[0] - 1, seed.shape[1] - 1
    ys = np.arange(Y + 1, dtype=np.int64)
    xs = np.arange(X + 1, dtype=np.int64)
    dy2 = (ys[:, None] - ys[None, :]) ** 2                                        # [y][y']
    r = np.where(seed[:, None, :], dy2[None, :, :], NO_SEED).min(axis=2)          # r[x][y]: the row part, NO_SEED without a seed
    dx2 = (xs[:, None] - xs[None, :]) ** 2                                        # [x][x']
    full = (dx2[:, :, None] + r[None, :, :]).min(axis=1)                          # full[x][y] = min over x' of (x - x')^2 + r[x'][y]
    if alias and X >= 1:
        s = np.concatenate([r[1:, 0], r[X:, Y]])                                  # what column Y reads through the scratch
        col_y = (dx2 + s[None, :]).min(axis=1)                                    # the transform of column Y ...
        full[1:, 0] = col_y[:X]                                                   # ... lands on column 0, one row down
    sq = np.where(full >= NO_SEED, DBL_MAX, full.astype(np.float64))
    return res * np.sqrt(sq)


def plain(grid, geom, win, dist=None, alias=True):
    """be_update_esdf2d on `dist` (None: DBL_MAX everywhere): a new [nx][ny] array, updated in the cells min .. max - 1 of `win`"""
    res = geom[2]
    min_x, min_y, max_x, max_y = win
    X, Y = max_x - min_x, max_y - min_y
    assert X >= 1 and Y >= 1
    st = window_cells(grid, win)
    pos = _transform(st == 2, res, alias)
    neg = _transform(st != 2, res, alias)
    d = pos.copy()
    inside = neg > 0.0
    d[inside] = d[inside] + (-neg[inside] + res)
    out = np.full(grid.shape, DBL_MAX) if dist is None else np.array(dist, np.float64)
    out[min_x:max_x, min_y:max_y] = d[:X, :Y]
    return out
