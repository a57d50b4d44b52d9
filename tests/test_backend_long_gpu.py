"""The 64-piece build of the back_end optimiser (BatchedMSPlanner(n, 33 .. 64)) on the GPU against the float64 oracle, and the chain
it is for: wide search -> set_paths -> plan -> check_plans -> trajectory store.

The problems are those of tests/backend_long_cases.py; tests/test_backend_long_cpu.py pins the oracle on them.  Tolerances are the
project's: one evaluation as tests/test_backend_eval_gpu.py (cost 1e-10 relative, gradient 1e-10 of its largest entry, xy_err 1e-11),
short L-BFGS runs as tests/test_backend_gpu.py (equal return code, iterations and evaluations, x within 1e-6, cost 1e-7 relative),
whole plans as test_obstacle_is_avoided_and_retry_logic_runs / test_long_paths_use_the_32_piece_kernel, the builder as
tests/test_flat_traj_build_gpu.py (1e-10), path_points / predicted_state as their tests there (1e-10, 1e-9).

Run with -s for the measured figures."""
import numpy as np
import pytest

from alore_legged_manipulator_amd.flat_traj import FrontEndParams
from tests import backend_eval_cases as ec
from tests import backend_long_cases as lc
from tests import flat_traj_cases
from tests.test_backend_eval_gpu import COST_TOL, GRAD_TOL, XY_TOL, assert_close, errors, same

pytestmark = pytest.mark.gpu

RESULT_KEYS = ("ok", "attempts", "alm_rounds", "evals", "lbfgs_ret", "path_ret", "collision", "n_pieces", "cost", "min_dist", "tail_s",
               "xy_err", "inner", "T", "coef")
KW = dict(lam=ec.LAM, rho=ec.RHO)


@pytest.fixture(scope="module")
def orc():
    from oracle.backend_driver import BackendOracle
    return BackendOracle()


def planner(grid, n, max_pieces=64, cfg=None):
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    pl = BatchedMSPlanner(n, max_pieces, cfg)
    assert pl.P == (16 if max_pieces <= 16 else 32 if max_pieces <= 32 else 64)
    pl.set_map(grid.dist, grid.x_lo, grid.y_lo, grid.res)
    return pl


def same_results(a, b, ia=None, ib=None):
    for k in RESULT_KEYS:
        x = a[k] if ia is None else a[k][ia]
        y = b[k] if ib is None else b[k][ib]
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), k


# ---- 1. one evaluation
@pytest.mark.parametrize("grid", lc.GRIDS)
@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("config", list(lc.CONFIGS))
def test_eval_matches_the_oracle_at_33_to_64_pieces(orc, config, stage, grid):
    """one launch per config, stage and map with M = 33, 34, 48, 49, 63, 64 submitted shuffled: a slot compared with another
    problem's oracle value is off in the first digit"""
    overrides = lc.CONFIGS[config]
    fts, xs, g = lc.eval_problems(grid), lc.eval_vectors(grid), lc.grid_of(grid)
    pl = planner(g, len(fts), 64, ec.handle_config(overrides))
    pl.set_problems(fts)
    out = pl.eval(stage, xs, **KW)
    pl.close()
    with ec.oracle_config(orc, overrides):
        refs = [orc.eval(g, ft, stage, x, **KW) for ft, x in zip(fts, xs)]
    per_slot = [errors(out, b, ref) for b, ref in enumerate(refs)]
    print(f"\neval {config} stage {stage} {grid}: " + "  ".join(f"M {ft.pieces}: {e[0]:.1e} {e[1]:.1e} {e[2]:.1e}" for ft, e in zip(fts, per_slot)) +
          f"  (bounds {COST_TOL:.0e} {GRAD_TOL:.0e} {XY_TOL:.0e})")
    for b, e in enumerate(per_slot):
        assert len(out["grad"][b]) == 3 * fts[b].pieces - 1
        assert_close(e, (config, stage, grid, fts[b].pieces))


# ---- 2. short L-BFGS runs
def lbfgs_against_the_oracle(orc, pl, fts, stage, iters):
    grid = lc.free_grid()
    xs = [orc.x0(ft) for ft in fts]
    out = pl.lbfgs(stage, xs, max_iter=iters)
    refs = [orc.lbfgs_run(grid, ft, stage, x, lam=(0.0, 0.0), rho=(1e4, 1e4), max_iter=iters) for ft, x in zip(fts, xs)]
    for b, (ft, ref) in enumerate(zip(fts, refs)):
        print(f"\nlbfgs stage {stage} k {iters} M {ft.pieces}: ret {out['ret'][b]} / {ref['ret']}  iters {out['iters'][b]} / {ref['iters']}  "
              f"evals {out['evals'][b]} / {ref['evals']}  |x - oracle| {np.max(np.abs(out['x'][b] - ref['x'])):.1e}  "
              f"cost {abs(out['cost'][b] - ref['cost']) / abs(ref['cost']):.1e}")
    for b, (ft, ref) in enumerate(zip(fts, refs)):
        M = ft.pieces
        assert out["ret"][b] == ref["ret"] and out["iters"][b] == ref["iters"] and out["evals"][b] == ref["evals"], M
        assert np.max(np.abs(out["x"][b] - ref["x"])) <= 1e-6, M
        assert abs(out["cost"][b] - ref["cost"]) <= 1e-7 * abs(ref["cost"]), M
    return refs


@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("iters", [3, 5, 20])
def test_short_lbfgs_runs_track_the_oracle(orc, iters, stage):
    """M = 33 and 64: three registers per vector in the two-loop recursion (pair by pair; the chunked form is the 16-piece build's)"""
    fts = lc.lbfgs_problems()
    pl = planner(lc.free_grid(), len(fts))
    pl.set_problems(fts)
    lbfgs_against_the_oracle(orc, pl, fts, stage, iters)
    pl.close()


def test_lbfgs_with_a_short_history_tracks_the_oracle(orc):
    """mem_size 5 in a run of 25 iterations: the history wraps (tests/test_backend_gpu.py, same name)"""
    from alore_legged_manipulator_amd.backend import default_config
    mem, iters = 5, 25
    cfg = default_config()
    cfg.lbfgs.mem_size = mem
    cfg.path_lbfgs.mem_size = mem
    fts = lc.lbfgs_problems()
    keep = (orc.cfg.lbfgs.mem_size, orc.cfg.path_lbfgs.mem_size)
    orc.cfg.lbfgs.mem_size = mem
    orc.cfg.path_lbfgs.mem_size = mem
    try:
        pl = planner(lc.free_grid(), len(fts), cfg=cfg)
        pl.set_problems(fts)
        refs = lbfgs_against_the_oracle(orc, pl, fts, 2, iters)
        pl.close()
        assert all(ref["iters"] > mem + 2 for ref in refs)               # the runs are long enough to wrap
    finally:
        orc.cfg.lbfgs.mem_size, orc.cfg.path_lbfgs.mem_size = keep


# ---- 3. whole plans
def plans_against_the_oracle(orc, grid, fts):
    pl = planner(grid, len(fts))
    res = pl.minco_plan(fts)
    for b, ft in enumerate(fts):
        ref = orc.minco_plan(grid, ft)
        M = ft.pieces
        print(f"\nplan M {M}: ok {res['ok'][b]} / {ref['ok']}  attempts {res['attempts'][b]} / {ref['attempts']}  evals {res['evals'][b]}  "
              f"min_dist {res['min_dist'][b]:.3f}  cost {res['cost'][b]:.6g} / {ref['cost']:.6g}")
        assert res["n_pieces"][b] == M
        assert bool(res["ok"][b]) == ref["ok"] and ref["ok"]
        assert res["attempts"][b] == ref["attempts"]
        assert np.hypot(*res["xy_err"][b]) < orc.cfg.tol
        assert res["min_dist"][b] > orc.cfg.final_min_safe_dis
        assert abs(res["cost"][b] - ref["cost"]) <= 0.1 * abs(ref["cost"])   # chaotic iteration: tests/test_backend_long_cpu.py measures the oracle's own spread
        tail = ft.final_state.copy(); tail[1, 0] = res["tail_s"][b]
        coef = orc.spline(res["T"][b, :M], res["inner"][b, :M - 1], ft.start_state, tail)
        assert np.max(np.abs(res["coef"][b, :6 * M] - coef)) <= 1e-9 * max(1.0, np.max(np.abs(coef)))
    again = pl.minco_plan(fts)
    same_results(again, res)
    pl.close()
    return res


def test_whole_plans_of_46_59_and_64_pieces_on_the_free_grid(orc):
    plans_against_the_oracle(orc, lc.free_grid(), [lc.route(46), lc.route(59), lc.route(64)])


def test_a_long_plan_avoids_the_disc(orc):
    ft = lc.past_disc()
    assert 32 < ft.pieces <= 64
    res = plans_against_the_oracle(orc, lc.disc_grid(), [ft])
    assert res["min_dist"][0] < 5.0                                       # the disc was in the way: on the free grid min_dist is 100


# ---- 4. batch mates and the launch order
def test_a_problem_alone_has_the_bits_of_its_slot_in_the_mixed_launch(orc):
    """M = 1, 16, 17, 32, 33 and 64 in one launch on a 64-piece handle: every slot has the bits of the same problem alone on its own
    64-piece handle.  The slots of at most 32 pieces meet the oracle at the tolerances of one evaluation; bit equality with the
    16- and 32-piece builds is NOT required of them (another reduction width in knot_pcr and in the two-loop recursion) and is not
    asserted"""
    grid = lc.free_grid()
    fts = lc.batch_problems()
    xs = ec.decision_vectors(fts, np.random.default_rng(3))
    pl = planner(grid, len(fts))
    pl.set_problems(fts)
    pieces = [ft.pieces for ft in fts]
    assert np.array_equal(pl.launch_order(), lc.stable_order(pieces))
    out = {stage: pl.eval(stage, xs, **KW) for stage in (1, 2)}
    pl.plan()
    res = pl.results()
    pl.close()
    assert res["ok"].all()
    for b, ft in enumerate(fts):
        one = planner(grid, 1)
        one.set_problems([ft])
        for stage in (1, 2):
            alone = one.eval(stage, [xs[b]], **KW)
            assert same(out[stage]["cost"][b], alone["cost"][0]) and same(out[stage]["grad"][b], alone["grad"][0]), (stage, ft.pieces)
            assert same(out[stage]["xy_err"][b], alone["xy_err"][0]), (stage, ft.pieces)
            assert_close(errors(out[stage], b, orc.eval(grid, ft, stage, xs[b], **KW)), (stage, ft.pieces))
        one.plan()
        same_results(one.results(), res, 0, b)
        one.close()


def test_the_device_launch_order_after_set_paths(orc):
    """most pieces first, stable in the slot index, by launch_order_kernel in its 65-bucket shape: equal piece counts on both sides
    of a longer one, and a slot that does not build in between (it keeps the count it had)"""
    from alore_legged_manipulator_amd.backend import BackendError
    short = np.array([[0.0, 0.0], [3.0, 1.0]])
    paths = [lc.ROUTES[46], short, lc.ROUTES[64], lc.ROUTES[59], short, lc.ROUTES[46], [[-1.0, 0.0], [19.0, 2.0]], lc.ROUTES[64]]
    pl = planner(lc.free_grid(), len(paths))
    pl.set_paths([np.array(p, np.float64) for p in paths], 0.0, 1.0)
    pieces = pl.problems()["n_pieces"]
    assert pieces[0] == 46 and pieces[2] == 64 and pieces[3] == 59 and pieces[1] == pieces[4] <= 16 and 16 < pieces[6] <= 32
    order = pl.launch_order()
    assert np.array_equal(order, lc.stable_order(pieces)) and list(order[:2]) == [2, 7]
    paths[3] = lc.ROUTES[69]
    with pytest.raises(BackendError, match="-5"):
        pl.set_paths([np.array(p, np.float64) for p in paths], 0.0, 1.0)
    assert np.array_equal(pl.problems()["n_pieces"], pieces)
    assert np.array_equal(pl.launch_order(), order)
    pl.close()


# ---- 5. set_paths
def test_set_paths_builds_64_pieces_and_refuses_more(orc):
    from alore_legged_manipulator_amd.backend import BUILD_E_PIECES, BUILD_OK, BackendError
    from tests.test_flat_traj_build_gpu import against_the_oracle
    prm = FrontEndParams()
    paths = [lc.route_path(64), lc.route_path(46), lc.route_path(59)]
    pl = planner(lc.free_grid(), 4)
    pl.set_paths([p[0] for p in paths], 0.0, 1.0, params=prm)
    assert list(pl.build_status()) == [BUILD_OK] * 3
    pr = pl.problems()
    for b, p in enumerate(paths):
        against_the_oracle(pr, b, flat_traj_cases.oracle(p, prm))
    comb = lc.searched_paths("comb")[0]
    with pytest.raises(BackendError, match="-5"):
        pl.set_paths([paths[0][0], lc.route_path(69)[0], comb[0], paths[1][0]], [0.0, 0.0, comb[1], 0.0], [1.0, 1.0, comb[2], 1.0], params=prm)
    assert list(pl.build_status()) == [BUILD_OK, BUILD_E_PIECES, BUILD_E_PIECES, BUILD_OK]
    pl.close()
    small = planner(lc.free_grid(), 1, 32)
    with pytest.raises(BackendError, match="-5"):
        small.set_paths([paths[1][0]], 0.0, 1.0, params=prm)
    assert list(small.build_status()) == [BUILD_E_PIECES]
    small.close()


# ---- 6. limits
def test_more_than_64_pieces_is_refused():
    from alore_legged_manipulator_amd.backend import BackendError, BatchedMSPlanner
    with pytest.raises(BackendError):
        BatchedMSPlanner(1, 65)
    pl = planner(lc.free_grid(), 1)
    with pytest.raises(BackendError):
        pl.set_problems([lc.route(69)])
    pl.close()


# ---- 7. object classes
CLASS_OVERRIDES = (dict(n_check=2, check_pts=ec.CHECK_PTS), dict(ec.DIRECT, n_check=7, check_pts=ec.CHECK_PTS))


@pytest.mark.parametrize("stage", [1, 2])
def test_mixed_class_launch_equals_single_config_handles(orc, stage):
    """two configs as the classes of ONE 64-piece launch at M = 40 on the disc map (the <64, true> build): every slot has the bits of
    a handle created with its class's config, and the oracle's value under that config"""
    grid = lc.disc_grid()
    probs = [ec.exact_pieces([[-12.0, -7.2], [12.0, 7.2]], 0.54, 0.54, 40), lc.long_bent_path(np.random.default_rng(40), 40)]
    layout = [(p, k) for p in range(len(probs)) for k in range(len(CLASS_OVERRIDES))]
    fts = [probs[p] for p, _ in layout]
    assert all(ft.pieces == 40 for ft in fts)
    xs = ec.decision_vectors(fts, np.random.default_rng(3))
    cfgs = [ec.handle_config(ov) for ov in CLASS_OVERRIDES]
    mixed = planner(grid, len(layout), 64, cfgs[0])
    mixed.set_classes(cfgs)
    mixed.set_problem_classes(np.array([k for _, k in layout], np.int32))
    mixed.set_problems(fts)
    out = mixed.eval(stage, xs, **KW)
    mixed.close()
    costs = {}
    for b, (p, k) in enumerate(layout):
        one = planner(grid, 1, 64, cfgs[k])
        one.set_problems([fts[b]])
        single = one.eval(stage, [xs[b]], **KW)
        one.close()
        assert same(out["cost"][b], single["cost"][0]) and same(out["grad"][b], single["grad"][0]), (stage, b, p, k)
        assert same(out["xy_err"][b], single["xy_err"][0]), (stage, b, p, k)
        with ec.oracle_config(orc, CLASS_OVERRIDES[k]):
            ref = orc.eval(grid, fts[b], stage, xs[b], **KW)
        assert_close(errors(out, b, ref), ("classes", stage, b, p, k))
        costs[p, k] = ref["cost"]
    for p in range(len(probs)):   # a table that is ignored cannot pass
        assert costs[p, 0] != costs[p, 1], (p, costs)


# ---- 8. the chain the feature is for
def test_wide_search_to_trajectory_store_on_a_64_piece_handle(orc):
    """wide_scene("boxes"): search_paths_device -> set_paths_device -> plan -> check_plans -> path_points / predicted_state -> the
    NMPC trajectory store.  A 32-piece handle answers BUILD_E_PIECES for the five wide slots (tests/test_path_search_wide_gpu.py)"""
    import torch
    from alore_legged_manipulator_amd.backend import BUILD_OK
    from alore_legged_manipulator_amd.nmpc import BatchedNmpc
    from oracle.backend_driver import path_points, predicted_state
    from tests import path_search_wide_cases as wide
    from tests.test_path_search_gpu import prefill, same_as_oracle
    s, want = wide.wide_scene("boxes"), wide.wide_expected("boxes")
    n = len(want)
    grid = lc.boxes_grid()
    pl = planner(grid, n)
    pl.search_reserve(wide.RESERVED, 2)
    prefill(pl, n)                                                        # same_as_oracle looks for the fill beyond every path
    starts = torch.tensor([a for a, _ in s["problems"]], dtype=torch.float64, device="cuda")
    goals = torch.tensor([b for _, b in s["problems"]], dtype=torch.float64, device="cuda")
    pl.search_paths_device(n, starts, goals, safe_dis=s["safe_dis"], window_margin=s["margin"])
    got = pl.paths(n)
    got["status"] = pl.search_status(n)
    for b in range(n):
        same_as_oracle(got, b, want[b], ("chain", b))
    v = pl.device_paths()
    yaw = torch.zeros(n, dtype=torch.float64, device="cuda")
    pl.set_paths_device(n, v.max_points, v.n_points, v.xy, yaw, yaw, params=FrontEndParams())
    torch.cuda.synchronize()
    assert list(pl.build_status(n)) == [BUILD_OK] * n
    pieces = pl.problems()["n_pieces"]
    assert tuple(pieces) == lc.BOXES_PIECES
    assert np.array_equal(pl.launch_order(), lc.stable_order(pieces))
    pl.plan()
    res = pl.results()
    print(f"\nchain: pieces {list(pieces)}  ok {list(res['ok'])}  attempts {list(res['attempts'])}  evals {list(res['evals'])}  "
          f"min_dist {[round(float(d), 3) for d in res['min_dist']]}  launch {pl.last_plan_ms():.1f} ms")
    assert res["ok"].all() and (res["attempts"] == 1).all()
    chk = pl.check_plans()
    assert not chk["collision"].any() and (chk["n_checked"] == 16 * pieces).all()
    fts = lc.boxes_problems()
    # path_points and predicted_state at 64-piece strides, against the oracle's restatement fed with the same coefficients
    pts = pl.path_points(3)
    total = np.array([res["T"][b, :pieces[b]].sum() for b in range(n)])
    times = np.array([res["T"][b, :41].sum() + 0.5 * res["T"][b, 41] if pieces[b] > 42 else 0.6 * total[b] for b in range(n)])
    assert (pieces > 42).sum() >= 4
    pred = pl.predicted_state(times, resolution=0.01)
    for b, ft in enumerate(fts):
        M = pieces[b]
        T, coef = res["T"][b, :M], res["coef"][b, :6 * M].reshape(-1)
        xy, yw = pts[b]
        exy, eyaw = path_points(T, coef, 3, ft.start_xytheta[:2])
        assert xy.shape == exy.shape == (4 * M, 2) and np.max(np.abs(xy - exy)) < 1e-10 and np.max(np.abs(yw - eyaw)) < 1e-10
        assert np.hypot(*(xy[-1] - np.array(ft.final_xytheta[:2]))) < 0.05
        xyt, vaj, oaj, fwd = predicted_state(T, coef, 0.01, times[b], start_xytheta=ft.start_xytheta)
        assert np.max(np.abs(pred["xytheta"][b] - xyt)) < 1e-10 and np.max(np.abs(pred["vaj"][b] - vaj)) < 1e-9
        assert np.max(np.abs(pred["oaj"][b] - oaj)) < 1e-9 and bool(pred["forward"][b]) == fwd
    # the trajectory store takes the plans device to device: durations and coefficients are the planner's result slabs
    eng = BatchedNmpc(n, 20, 0.01)
    eng.refs_init(max_pieces=64, max_checkpoints=512)
    eng.refs_set_from_backend(pl, traj_start_time=0.25)
    for b in range(n):
        M = pieces[b]
        d = eng.refs_download(b)
        assert d["valid"] and d["start_time"] == 0.25 and d["durations"].shape == (M,)
        assert d["durations"].tobytes() == res["T"][b, :M].tobytes()
        stored = np.ascontiguousarray(res["coef"][b, :6 * M].reshape(M, 6, 2).transpose(0, 2, 1))
        assert np.ascontiguousarray(d["coeffs"]).tobytes() == stored.tobytes(), b
    pl.close()
