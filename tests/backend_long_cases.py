"""Problems of 33 to 64 pieces for the 64-piece build of the back_end optimiser (tests/test_backend_long_cpu.py pins the oracle and
the scenes on the CPU, tests/test_backend_long_gpu.py compares the kernel with the oracle).

Piece counts and what they exercise in backend::knot_pcr / eval_cost / lbfgs:
  33      the first count the 32-piece build cannot hold; 32 knots, so the elimination step of stride 32 does not run yet
  34      nk = 33: the stride-32 step runs with exactly one partner
  48, 49  mid range; the 8 M + 1 panel ends cross a multiple of 64
  63, 64  nk = 62 and 63: all lanes but one hold a knot; 3 M - 1 = 191 variables is the last lane of the third register; 17 M = 1088
          nodes is exactly 17 rounds

No GPU imports here."""
import functools
import math

import numpy as np

from alore_legged_manipulator_amd.flat_traj import FrontEndParams, waypoint_path
from tests import backend_eval_cases as ec
from tests import path_search_wide_cases as wide

COUNTS = (33, 34, 48, 49, 63, 64)
CONFIGS = {"default": {}, "all-active": ec.ALL_ACTIVE, "direct": ec.DIRECT}
GRIDS = ("free", "disc")

# way-point routes of 36 to 54 m at the default front end (sample_time 0.4, max_vel 3, max_acc 2, distance_weight 1.4)
ROUTES = {46: [[-16, -10], [0, -3], [14, 9]], 59: [[-20, -12], [0, -3], [20, 12]], 64: [[-22, -12], [0, -3], [22, 13]],
          69: [[-24, -13], [0, -3], [24, 14]]}
PAST_DISC = ([[-20, -12], [20, 12]], 0.54, 0.54)       # two points, straight past the disc of disc_grid()
BOXES_PIECES = (43, 44, 45, 43, 34, 14, 12)
COMB_PIECES = 149


@functools.lru_cache(maxsize=None)
def route(pieces):
    ft = waypoint_path(ROUTES[pieces], 0.0, 1.0)
    assert ft.pieces == pieces, (ft.pieces, pieces)
    return ft


@functools.lru_cache(maxsize=None)
def past_disc():
    pts, y0, y1 = PAST_DISC
    return waypoint_path(pts, y0, y1)


def route_path(pieces):
    """the route as a path of tests/flat_traj_cases.py: (xy, start_yaw, end_yaw, start_vaj, start_oaj)"""
    return (np.array(ROUTES[pieces], np.float64), 0.0, 1.0, np.zeros(3), np.zeros(3))


@functools.lru_cache(maxsize=None)
def free_grid():
    from oracle.backend_driver import EsdfGrid
    return EsdfGrid.free(half=40.0)


@functools.lru_cache(maxsize=None)
def disc_grid():
    """a disc of radius 1.2 at (0, 0.4) on a map of +-30 m: on the straight line of PAST_DISC"""
    from oracle.backend_driver import EsdfGrid
    return EsdfGrid.from_field(lambda X, Y: np.hypot(X - 0.0, Y - 0.4) - 1.2, half=30.0, res=0.1)


@functools.lru_cache(maxsize=None)
def boxes_grid():
    from oracle.backend_driver import EsdfGrid
    m = wide.wide_scene("boxes")["map"]
    return EsdfGrid(m.dist, m.x_lo, m.y_lo, m.res)


def searched_paths(name):
    """the oracle's searched paths of a wide scene as paths of tests/flat_traj_cases.py (yaw 0 at both ends, at rest)"""
    zeros = np.zeros(3)
    return [(np.array(w.xy, np.float64), 0.0, 0.0, zeros, zeros) for w in wide.wide_expected(name)]


@functools.lru_cache(maxsize=None)
def boxes_problems():
    from tests import flat_traj_cases
    return tuple(flat_traj_cases.oracle(p, FrontEndParams()) for p in searched_paths("boxes"))


# ---- exact piece counts for eval and short L-BFGS runs
def long_bent_path(rng, M):
    """backend_eval_cases.bent_path with legs that grow with M: that table cuts legs of 1.5 to 3.5 m into 9 pieces, and its noise on
    the decision vector (0.05) is sized for pieces of that length; here a piece is as long as there, whatever M"""
    p0 = rng.uniform(-2.0, 2.0, 2)
    b0 = rng.uniform(-math.pi, math.pi)
    l0, l1 = rng.uniform(1.5, 3.5, 2) * (M / ec.M_CONFIG)
    turn = rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 1.4)
    p1 = p0 + l0 * np.array([math.cos(b0), math.sin(b0)])
    p2 = p1 + l1 * np.array([math.cos(b0 + turn), math.sin(b0 + turn)])
    return ec.exact_pieces([p0, p1, p2], b0 + rng.uniform(-0.8, 0.8), b0 + turn + rng.uniform(-0.8, 0.8), M)


def grid_of(name):
    return {"free": free_grid, "disc": disc_grid}[name]()


@functools.lru_cache(maxsize=None)
def eval_problems(grid):
    """one problem per count of COUNTS, in a shuffled order: bent paths on the free grid; on the disc grid straight lines through
    the origin, 0.7 m per piece, which the disc of disc_grid() sits on"""
    order = [int(m) for m in np.random.default_rng(64).permutation(COUNTS)]
    if grid == "free":
        rng = np.random.default_rng(164)
        return tuple(long_bent_path(rng, M) for M in order)
    return tuple(ec.exact_pieces([[-0.3 * M, -0.18 * M], [0.3 * M, 0.18 * M]], 0.54, 0.54, M) for M in order)


@functools.lru_cache(maxsize=None)
def eval_vectors(grid):
    return tuple(ec.decision_vectors(list(eval_problems(grid)), np.random.default_rng(3)))


def piece_problems(counts, seed):
    rng = np.random.default_rng(seed)
    return [long_bent_path(rng, M) for M in counts]


def lbfgs_problems():
    """33 and 64 pieces for the short L-BFGS runs"""
    return piece_problems((33, 64), seed=264)


def batch_problems():
    """one launch on a 64-piece handle with counts that belong to each of the three builds"""
    return piece_problems((1, 16, 17, 32, 33, 64), seed=364)


FD_STEP = 1e-7


def fd_grad(orc, grid, ft, stage, x, **kw):
    """central differences of the oracle's cost with an absolute step.  backend_eval_cases.fd_grad steps by 1e-6 max(1, |x_i|): here
    the arc lengths among the x_i reach 30 m where that table's reach 5, its step grows with them and so does the truncation error
    (h^2 / 6 times the third derivative) of the steep penalty terms: 3.8e-4 of the largest entry at 64 pieces with its step,
    1.4e-8 with this one, against the same analytic gradient.  Rounding: eps |cost| / h = 2e-16 x 1e5 / 1e-7 = 2e-4 against
    entries of 1e5"""
    g = np.zeros_like(x)
    for i in range(len(x)):
        xp = x.copy(); xp[i] += FD_STEP; xm = x.copy(); xm[i] -= FD_STEP
        g[i] = (orc.eval(grid, ft, stage, xp, **kw)["cost"] - orc.eval(grid, ft, stage, xm, **kw)["cost"]) / (xp[i] - xm[i])
    return g


def stable_order(pieces):
    """most pieces first, stable in the slot index"""
    return np.argsort(-np.asarray(pieces, np.int64), kind="stable")
