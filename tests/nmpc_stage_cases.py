"""Stage-varying planar NMPC problems (test data, NumPy only).

scenarios.make_batch and make_wide_batch give every stage of a problem the same W, the same ICR triple od and the same
bounds, so a kernel that read another stage's record -- stage 0 for every stage, the neighbouring lane's stage, slot s of
the wrong lane -- would return the same numbers.  vary_stages() makes every one of them differ from stage to stage, keeps W
symmetric positive definite, and (reverse, warm) makes both bounds bind and the iterate generic.  broadcast_stage0() and
swap_stages() are the two index bugs as mutations of ONE problem: tests/test_nmpc_stages_cpu.py shows with the oracle alone
that the cases tell them apart."""
from __future__ import annotations

import numpy as np

# floats per stage of the members that carry one record per stage (od: per node, N + 1 of them)
STAGE_FIELDS = {"W": 25, "od": 3, "y": 5, "lbValues": 2, "ubValues": 2}


def _add_aat(rng, M, lo, hi):
    """M[..., lo:hi, lo:hi] += A A', A standard normal times 0.3 sqrt(mean of the block's diagonal), one A per leading index"""
    n = hi - lo
    blk = M[..., lo:hi, lo:hi]
    amp = 0.3 * np.sqrt(np.mean(np.diagonal(blk, axis1=-2, axis2=-1), axis=-1))
    A = rng.standard_normal(blk.shape[:-2] + (n, n)) * amp[..., None, None]
    M[..., lo:hi, lo:hi] = blk + A @ np.swapaxes(A, -1, -2)


def vary_stages(batch: dict, seed: int, weights: str = "keep", warm: bool = False, reverse: bool = False) -> dict:
    """A copy of `batch` (layout of scenarios.py) whose W, od and bounds differ at every stage; all draws from
    default_rng([seed, 7]); float32.

    weights: "diag" -- off-diagonal entries of W, WN exactly 0.0 (the stage-block kernel then takes its diagonal-weights body);
             "full" -- the same, then A A' added inside the state (3 x 3) and input (2 x 2) blocks of every stage and to WN, A drawn
             per problem and stage (the state-input cross blocks stay zero: the generated code ignores them, see make_wide_batch);
             "keep" -- the pattern as it came.
    Then W_k <- S_k W_k S_k with S_k = diag(3 ** uniform(-0.5, 0.5)) per problem, stage and entry (WN likewise): symmetric
    positive definite as before, the same sparsity pattern.
    od: + uniform(-0.05, 0.05, 3) * k / N per problem (drift) + uniform(-0.01, 0.01) per node (jitter).
    bounds: ubValues and lbValues each times uniform(0.5, 1.0) per problem, stage and input.
    reverse: odd problems drive backwards (x, y of the reference poses and the reference wheel speeds negated), so that lower
             bounds bind as well.
    warm: x[k] += normal(0, 0.05) for k >= 1, x[0] = x0; u = clip(0.5 * reference wheel speeds + normal(0, 0.3), lb, ub)."""
    if weights not in ("diag", "full", "keep"):
        raise ValueError(weights)
    rng = np.random.default_rng([int(seed), 7])
    out = {k: np.array(v, dtype=np.float64) for k, v in batch.items()}
    B, N = out["u"].shape[:2]
    W, WN = out["W"], out["WN"]
    if weights != "keep":
        W *= np.eye(5)
        WN *= np.eye(3)
    if weights == "full":
        _add_aat(rng, W, 0, 3)
        _add_aat(rng, W, 3, 5)
        _add_aat(rng, WN, 0, 3)
    s = 3.0 ** rng.uniform(-0.5, 0.5, (B, N, 5))
    W *= s[..., :, None] * s[..., None, :]
    sN = 3.0 ** rng.uniform(-0.5, 0.5, (B, 3))
    WN *= sN[..., :, None] * sN[..., None, :]
    drift = rng.uniform(-0.05, 0.05, (B, 1, 3)) * (np.arange(N + 1)[None, :, None] / N)
    out["od"] += drift + rng.uniform(-0.01, 0.01, (B, N + 1, 3))
    out["ubValues"] *= rng.uniform(0.5, 1.0, (B, N, 2))
    out["lbValues"] *= rng.uniform(0.5, 1.0, (B, N, 2))
    if reverse:
        odd = np.arange(B) % 2 == 1
        out["y"][odd, :, 0:2] *= -1.0
        out["y"][odd, :, 3:5] *= -1.0
        out["yN"][odd, 0:2] *= -1.0
    if warm:
        out["x"][:, 1:, :] += rng.normal(0.0, 0.05, (B, N, 3))
        out["x"][:, 0, :] = out["x0"]
        out["u"] = np.clip(0.5 * out["y"][:, :, 3:5] + rng.normal(0.0, 0.3, (B, N, 2)), out["lbValues"], out["ubValues"])
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def nominal(B: int, N: int, weights: str, seed: int | None = None, warm: bool = True) -> dict:
    """The nominal cases of the stage tests: the benchmark's distribution with a tenth of fast references, every stage different,
    odd problems backwards, a generic iterate (warm; False: the cold start).  seed None: the default stream of make_batch, stage
    data drawn with seed N; otherwise other problems (stream 1000 + seed) with other stage data."""
    from alore_legged_manipulator_amd.scenarios import SEED, make_batch
    base = make_batch(B, N, seed=SEED if seed is None else 1000 + int(seed), fast_tail=0.1)
    return vary_stages(base, N if seed is None else seed, weights, warm=warm, reverse=True)


def _stages(problem: dict, field: str):
    a = np.array(problem[field], dtype=np.float32).reshape(-1, STAGE_FIELDS[field])
    return a


def broadcast_stage0(problem: dict, field: str) -> dict:
    """`problem` (flat arrays, scenarios.problem) with stage 0's record of `field` at every stage: what a kernel solves that reads
    stage 0's data for every stage"""
    a = _stages(problem, field)
    a[:] = a[0]
    return dict(problem, **{field: a.reshape(-1)})


def swap_stages(problem: dict, field: str, k: int) -> dict:
    """`problem` with the records of stages k and k + 1 of `field` exchanged: what a kernel solves that reads its neighbour's stage"""
    a = _stages(problem, field)
    a[[k, k + 1]] = a[[k + 1, k]]
    return dict(problem, **{field: a.reshape(-1)})
