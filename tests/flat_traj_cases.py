"""Way-point paths for the tests of the device FlatTrajData builder (test_flat_traj_build_cpu.py, test_flat_traj_build_gpu.py) and
their oracle, alore_legged_manipulator_amd.flat_traj (NumPy).

A path is (xy [n][2], start_yaw, end_yaw, start_vaj [3], start_oaj [3]).  The generator rejects a path whose piece count is
decided by a last-ulp difference: total_t / sample_time + 0.5 within 1e-6 of an integer (the divisor of sample_t), or a sample time
within 1e-6 of total_t - 1e-3 (the end of the sampling loop)."""
import math

import numpy as np

from alore_legged_manipulator_amd import flat_traj


def oracle(path, prm):
    xy, sy, ey, vaj, oaj = path
    return flat_traj.with_time(flat_traj.sample_path(np.asarray(xy, np.float64), float(sy), float(ey)), prm, tuple(vaj), tuple(oaj))


def on_a_knife_edge(path, prm) -> bool:
    ft = oracle(path, prm)
    total_t = ft.meta["total_time"]
    q = total_t / prm.sample_time + 0.5
    if abs(q - round(q)) < 1e-6:
        return True
    t = ft.init_T
    for _ in range(200):  # every sample time up to the first one past the end
        if abs(t - (total_t - 1e-3)) < 1e-6:
            return True
        if not t < total_t - 1e-3:
            break
        t += ft.init_T
    return False


def _random_path(rng, kind):
    n = int(rng.integers(2, 7))
    p0 = rng.uniform(-5, 5, 2)
    sy, ey = rng.uniform(-math.pi, math.pi, 2)
    vaj, oaj = np.zeros(3), np.zeros(3)
    if kind == "straight":      # two points
        n = 2
    bearings = rng.uniform(-math.pi, math.pi, n - 1)
    if kind == "collinear":     # every turn node between the drives has zero weighted length
        n = max(n, 3)
        bearings = np.full(n - 1, rng.uniform(-math.pi, math.pi))
    if kind == "aligned":       # the start yaw is the first heading: nodes 1 and 2 have zero weighted length
        sy = bearings[0]
    steps = rng.uniform(0.5, 2.5, n - 1)
    xy = np.concatenate([[p0], p0 + np.cumsum(np.stack([steps * np.cos(bearings), steps * np.sin(bearings)], 1), 0)])
    if kind == "moving":        # a start speed of 1.5
        vaj = np.array([1.5, rng.uniform(-0.5, 0.5), 0.0]); oaj = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 0.0])
    if kind == "fast":          # a start speed above max_vel
        vaj = np.array([3.5, 0.0, 0.0])
    return xy, float(sy), float(ey), vaj, oaj


KINDS = ("straight", "collinear", "aligned", "moving", "fast", "any", "any", "any", "any", "any")


def make_paths(count, prm, seed=20261018, max_pieces=None):
    """`count` accepted paths of the kinds above in turn (fixed seed) and the number of candidates rejected for a knife edge;
    max_pieces: paths with more pieces are passed over (not counted as rejected)"""
    rng = np.random.default_rng(seed)
    out, rejected = [], 0
    while len(out) < count:
        path = _random_path(rng, KINDS[len(out) % len(KINDS)])
        if max_pieces is not None and oracle(path, prm).pieces > max_pieces:
            continue
        if on_a_knife_edge(path, prm):
            rejected += 1
            continue
        out.append(path)
    return out, rejected


def pack(paths, K):
    """the arrays of alore_backend_paths, padded to K way-points"""
    n = len(paths)
    npts = np.array([len(p[0]) for p in paths], np.int32)
    xy = np.zeros((n, K, 2))
    for b, p in enumerate(paths):
        xy[b, :len(p[0])] = p[0]
    sy = np.array([p[1] for p in paths], np.float64)
    ey = np.array([p[2] for p in paths], np.float64)
    vaj = np.array([p[3] for p in paths], np.float64).reshape(n, 3)
    oaj = np.array([p[4] for p in paths], np.float64).reshape(n, 3)
    return npts, xy, sy, ey, vaj, oaj
