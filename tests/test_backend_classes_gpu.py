"""Object classes of the back_end on the GPU (alore_backend_set_classes, include/alore_backend.h): a table of whole configs on the
handle, a class index per problem slot, every call that reads robot-model parameters honours them, and the result reaches the
NMPC store with the right xv per slot.

Scene (tests/backend_classes_cases.py): the three problems of monte_carlo_goals(3, seed=44) (14, 12 and 8 pieces), a map with one
disc of radius 0.4 per problem next to the middle of its straight line, and four classes: k0 the default, k1 the ICR model with
xv 0.2, k2 xv 0.3 with lower limits, more clearance and a third check point, k3 xv 0.1 without check points.  On the CPU oracle
k0..k2 plan every problem in one attempt and k3 fails problems 0 and 2 after three attempts with a final collision.

The optimiser's loose stopping rule makes whole plans bimodal against the oracle (tests/test_backend_gpu.py), so whole plans are
compared between device routes, BIT FOR BIT: slot b of a mixed launch against a handle created with that class's config planning
the same problem alone.  The oracle pins single evaluations (1e-10, the tolerances of tests/test_backend_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import backend_classes_cases as cases

pytestmark = pytest.mark.gpu

STATUS = ("ok", "attempts", "alm_rounds", "evals", "lbfgs_ret", "path_ret", "collision", "n_pieces", "cost", "xy_err", "min_dist", "tail_s")
SLABS = ("T", "coef", "inner", "tail")
CHECK = ("collision", "first_panel", "n_checked", "first_time", "first_xy", "min_dist")
NK, NP_ = cases.N_CLASSES, 3
INTERLEAVED = [(b // NK, b % NK) for b in range(NK * NP_)]   # slot b: (problem, class); classes interleaved (b % 4)
PERMUTED = [(b % NP_, (b // NP_ + 1) % NK) for b in range(NK * NP_)]   # every pair once more, other slot, other neighbours


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b))))


def planner(grid, n, cfg=None, max_pieces=16):
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    pl = BatchedMSPlanner(n, max_pieces, cfg)
    pl.set_map(grid.dist, grid.x_lo, grid.y_lo, grid.res)
    return pl


def full(pl, n=None):
    """results() and the tail slab of the device view"""
    import torch
    from alore_legged_manipulator_amd.backend import _DeviceArray
    n = int(n or pl.count)
    out = pl.results(n)
    out["tail"] = torch.as_tensor(_DeviceArray(pl.device_view().tail, (n, 6), "<f8"), device="cuda").cpu().numpy()
    return out


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_slot_equals(mixed, b, single, what):
    for k in STATUS + SLABS:
        assert same(mixed[k][b], single[k][0]), (what, b, k, mixed[k][b], single[k][0])


def mixed_planner(sc, layout):
    pl = planner(sc["grid"], len(layout))
    pl.set_classes(sc["cfgs"])
    pl.set_problem_classes(np.array([k for _, k in layout], np.int32))
    pl.set_problems([sc["fts"][p] for p, _ in layout])
    return pl


@pytest.fixture(scope="module")
def sc():
    """the scene, the single-class handles (one per (problem, class), each planning its problem alone) and the mixed launch"""
    from oracle.backend_driver import BackendOracle
    fts = cases.problems()
    assert [ft.pieces for ft in fts] == [14, 12, 8]
    grid = cases.disc_grid(cases.disc_centres(fts))
    cfgs = cases.class_configs()
    s = {"fts": fts, "grid": grid, "cfgs": cfgs, "orc": BackendOracle(), "single": {}, "single_res": {}}
    for p in range(NP_):
        for k in range(NK):
            pl = planner(grid, 1, cfgs[k])
            pl.set_problems([fts[p]])
            pl.plan()
            s["single"][p, k], s["single_res"][p, k] = pl, full(pl)
    s["mixed"] = mixed_planner(s, INTERLEAVED)
    s["mixed"].plan()
    s["mixed_res"] = full(s["mixed"])
    return s


def oracle_cfg(orc, cfg):
    """the oracle's config <- a class (the structs share their layout up to the oracle's own trailing field)"""
    from alore_legged_manipulator_amd.backend import BackendConfig
    C.memmove(C.byref(orc.cfg), C.byref(cfg), C.sizeof(BackendConfig))


def test_mixed_launch_equals_single_class_handles(sc):
    """12 slots = 4 classes x 3 problems in ONE launch: T, coef, inner, tail, n_pieces and every field of the status record of a
    slot are the bits of a handle created with the slot's class planning that problem alone -- for the interleaved assignment and
    for a permuted one (other slot, other neighbours).  The classes matter: the durations of a problem differ by class."""
    for layout, res in ((INTERLEAVED, sc["mixed_res"]), (PERMUTED, None)):
        if res is None:
            pl = mixed_planner(sc, layout)
            pl.plan()
            res = full(pl)
            pl.close()
        for b, (p, k) in enumerate(layout):
            assert_slot_equals(res, b, sc["single_res"][p, k], layout is PERMUTED)
    dur = {(p, k): float(sc["single_res"][p, k]["T"][0].sum()) for p in range(NP_) for k in range(NK)}
    for p in range(NP_):
        assert len({dur[p, k] for k in range(NK)}) == NK, [dur[p, k] for k in range(NK)]   # a table that is ignored cannot pass
    st = sc["mixed"].class_state(12)
    assert st["n_classes"] == NK and st["clamped"] == 0 and st["class_of"].tolist() == [k for _, k in INTERLEAVED]
    assert st["xv"].tolist() == [cases.effective_xv(sc["cfgs"][k]) for _, k in INTERLEAVED]


def test_one_class_equal_to_the_config_is_no_table(sc):
    from alore_legged_manipulator_amd.backend import default_config
    plain = planner(sc["grid"], NP_)
    plain.set_problems(sc["fts"])
    plain.plan()
    a = full(plain)
    one = planner(sc["grid"], NP_)
    one.set_classes([default_config()])
    one.set_problems(sc["fts"])
    one.plan()
    b = full(one)
    for k in STATUS + SLABS:
        assert same(a[k], b[k]), k
    # ... and a table that is removed again leaves the handle as it was
    one.set_classes([])
    one.plan()
    c = full(one)
    for k in STATUS + SLABS:
        assert same(a[k], c[k]), k
    assert one.class_state(NP_)["xv"].tolist() == [0.0] * NP_


def assert_eval_close(out, b, ref, what):
    """the tolerances of tests/test_backend_gpu.py: cost 1e-10 relative, gradient 1e-10 of its largest entry, xy_err 1e-11"""
    assert abs(out["cost"][b] - ref["cost"]) <= 1e-10 * abs(ref["cost"]), (what, b, out["cost"][b], ref["cost"])
    assert rel(out["grad"][b], ref["grad"]) <= 1e-10, (what, b)
    assert np.max(np.abs(out["xy_err"][b] - ref["xy_err"])) <= 1e-11, (what, b)


@pytest.mark.parametrize("configured", [True, False], ids=["configured", "explicit"])
@pytest.mark.parametrize("stage", [1, 2])
def test_evaluation_matches_the_oracle_per_class(sc, stage, configured):
    """alore_backend_eval at the initial decision vector of the 12 slots against BackendOracle.eval under the slot's class's cfg.
    configured: safe_dis and time_weight are left at "the configured value" on both sides, so every slot is evaluated with its
    CLASS's safe_dis and w_time (k2: 0.8, not the handle's 0.6).  explicit: the arguments override the config for every slot, as
    ever, and both sides get the same values."""
    orc, pl = sc["orc"], sc["mixed"]
    xs = [orc.x0(sc["fts"][p]) for p, _ in INTERLEAVED]
    kw = dict(lam=(3.0, -2.0), rho=(5e3, 2e4))
    if not configured:
        kw.update(safe_dis=0.7, time_weight=40.0)
    out = pl.eval(stage, xs, **kw)
    costs = {}
    for b, (p, k) in enumerate(INTERLEAVED):
        oracle_cfg(orc, sc["cfgs"][k])
        ref = orc.eval(sc["grid"], sc["fts"][p], stage, xs[b], **kw)
        assert_eval_close(out, b, ref, (stage, configured))
        costs[p, k] = ref["cost"]
        if configured:   # ... and the bits of the handle created with the class, asked the same way
            one = sc["single"][p, k].eval(stage, [xs[b]], **kw)
            assert same(out["cost"][b], one["cost"][0]) and same(out["grad"][b], one["grad"][0]), (b, p, k)
    if stage == 2:
        assert all(costs[p, 2] != costs[p, 0] and costs[p, 3] != costs[p, 1] for p in range(NP_))   # the classes differ where it counts


def test_configured_safe_dis_and_time_weight_are_the_class_s(sc):
    """The arguments of eval / lbfgs that stand for the configured value on a table whose classes differ in BOTH: k0, and k2 with
    w_time 80 (safe_dis 0.8 already).  A handle created with k0 evaluates a k2 slot like the oracle under k2, and like a handle
    created with k2, bit for bit; lbfgs (stage 1 and 2, six iterations) leaves the bits of the single-class handles; a given value
    still holds for every slot."""
    orc, fts, grid = sc["orc"], sc["fts"], sc["grid"]
    heavy = cases.copy_config(sc["cfgs"][2])
    heavy.w_time = 80.0
    table = [sc["cfgs"][0], heavy]
    ft = fts[1]
    x = orc.x0(ft)
    mixed = planner(grid, 2)
    mixed.set_classes(table)
    mixed.set_problem_classes(np.array([0, 1], np.int32))
    mixed.set_problems([ft, ft])
    singles = []
    for cfg in table:
        one = planner(grid, 1, cfg)
        one.set_problems([ft])
        singles.append(one)
    kw = dict(lam=(3.0, -2.0), rho=(5e3, 2e4))
    for stage in (1, 2):
        out = mixed.eval(stage, [x, x], **kw)
        for b, cfg in enumerate(table):
            oracle_cfg(orc, cfg)
            ref = orc.eval(grid, ft, stage, x, **kw)
            assert_eval_close(out, b, ref, stage)
            one = singles[b].eval(stage, [x], **kw)
            assert same(out["cost"][b], one["cost"][0]) and same(out["grad"][b], one["grad"][0]), (stage, b)
        assert not same(out["grad"][0], out["grad"][1]), stage
        given = mixed.eval(stage, [x, x], safe_dis=0.8, time_weight=80.0, **kw)    # the heavy class's values for both slots
        assert same(given["cost"][1], out["cost"][1]) and same(given["grad"][1], out["grad"][1]), stage
        assert not same(given["grad"][0], out["grad"][0]), stage               # w_time enters the duration gradient
        run = mixed.lbfgs(stage, [x, x], max_iter=6)
        for b in range(2):
            one = singles[b].lbfgs(stage, [x], max_iter=6)
            for f in ("x", "cost", "ret", "iters", "evals", "xy_err"):
                assert same(run[f][b], one[f][0]), (stage, b, f, run[f][b], one[f][0])
        assert not same(run["x"][0], run["x"][1]), stage
    for pl in [mixed] + singles:
        pl.close()


@pytest.mark.parametrize("configured", [True, False], ids=["configured", "explicit"])
def test_the_32_piece_kernel_reads_the_class(sc, configured):
    from alore_legged_manipulator_amd.flat_traj import waypoint_path
    from oracle.backend_driver import EsdfGrid
    orc = sc["orc"]
    grid = EsdfGrid.free(half=40.0)
    ft = waypoint_path([[-6.0, -4.0], [0.0, -1.0], [6.0, 4.0]], 0.0, 1.0)
    assert 16 < ft.pieces <= 32
    pl = planner(grid, 2, max_pieces=32)
    pl.set_classes([sc["cfgs"][0], sc["cfgs"][2]])
    pl.set_problem_classes(np.array([0, 1], np.int32))
    pl.set_problems([ft, ft])
    x = orc.x0(ft)
    kw = dict(lam=(3.0, -2.0), rho=(5e3, 2e4)) if configured else dict(safe_dis=0.6, time_weight=50.0)
    out = pl.eval(2, [x, x], **kw)
    for b, k in enumerate((0, 2)):
        oracle_cfg(orc, sc["cfgs"][k])
        ref = orc.eval(grid, ft, 2, x, **kw)
        assert_eval_close(out, b, ref, configured)
    assert out["cost"][0] != out["cost"][1]
    pl.close()


def test_check_plans_reads_the_class(sc):
    """body = 1 and min_safe_dis = 0 (the configured threshold): xv, the check points, final_check_num and the threshold of every
    slot are its class's; a k3 slot (no check points) checks the reference point alone.  Once on the planning map, once with a disc
    moved onto a planned path."""
    mixed, grid = sc["mixed"], sc["grid"]

    ok = sc["mixed_res"]["ok"] != 0

    def compare():
        got = mixed.check_plans(body=True)
        for b, (p, k) in enumerate(INTERLEAVED):
            ref = sc["single"][p, k].check_plans(body=sc["cfgs"][k].n_check > 0)
            for f in CHECK:
                assert same(got[f][b], ref[f][0]), (b, f, got[f][b], ref[f][0])
        return got
    first = compare()
    assert not first["collision"][ok].any()                     # what the optimiser accepted is free (a rejected k3 plan is not)
    assert np.all(first["n_checked"][ok] == 16 * sc["mixed_res"]["n_pieces"][ok])
    path = mixed.path_points(3, 12)[0][0]                       # slot 0: problem 0, class k0 (ok)
    centre = path[len(path) // 2]
    moved = cases.disc_grid([tuple(centre)] + cases.disc_centres(sc["fts"])[1:])
    try:
        for pl in [mixed] + list(sc["single"].values()):
            pl.set_map(moved.dist, moved.x_lo, moved.y_lo, moved.res)
        hit = compare()
        assert hit["collision"][0] == 1 and hit["first_panel"][0] >= 0 and hit["n_checked"][0] < first["n_checked"][0]
    finally:
        for pl in [mixed] + list(sc["single"].values()):
            pl.set_map(grid.dist, grid.x_lo, grid.y_lo, grid.res)


def test_predicted_state_and_path_points_read_the_class(sc):
    import torch
    from oracle.backend_driver import path_points, predicted_state
    mixed, res = sc["mixed"], sc["mixed_res"]
    n = len(INTERLEAVED)
    total = np.array([res["T"][b, :res["n_pieces"][b]].sum() for b in range(n)])
    times = total * np.linspace(0.35, 0.9, n)
    host = mixed.predicted_state(times, resolution=0.01)
    dev = {"xytheta": torch.zeros(n, 3, dtype=torch.float64, device="cuda"), "vaj": torch.zeros(n, 3, dtype=torch.float64, device="cuda"),
           "oaj": torch.zeros(n, 3, dtype=torch.float64, device="cuda"), "forward": torch.zeros(n, dtype=torch.int32, device="cuda")}
    mixed.predicted_state_device(n, torch.as_tensor(times, device="cuda"), dev["xytheta"], dev["vaj"], dev["oaj"], dev["forward"], resolution=0.01)
    torch.cuda.synchronize()
    paths = mixed.path_points(3, n)
    moved = 0
    for b, (p, k) in enumerate(INTERLEAVED):
        cfg, single, ft = sc["cfgs"][k], sc["single"][p, k], sc["fts"][p]
        ref = single.predicted_state(times[b:b + 1], resolution=0.01)
        for f in ("xytheta", "vaj", "oaj"):
            assert same(host[f][b], ref[f][0]), (b, f)
            assert same(dev[f][b].cpu().numpy(), ref[f][0]), (b, f, "device route")
        assert bool(host["forward"][b]) == bool(ref["forward"][0]) == bool(dev["forward"][b].item())
        M = res["n_pieces"][b]
        T, coef = res["T"][b, :M], res["coef"][b, :6 * M].reshape(-1)
        model = dict(standard_diff=bool(cfg.standard_diff), xv=float(cfg.icr_xv))
        xyt, vaj, oaj, fwd = predicted_state(T, coef, 0.01, times[b], start_xytheta=ft.start_xytheta, **model)
        assert np.max(np.abs(host["xytheta"][b] - xyt)) < 1e-10 and bool(host["forward"][b]) == fwd, b
        xy0, _, _, _ = predicted_state(T, coef, 0.01, times[b], start_xytheta=ft.start_xytheta)
        moved += int(np.max(np.abs(xy0 - xyt)) > 1e-6)
        xy, yaw = paths[b]
        rxy, ryaw = single.path_points(3, 1)[0]
        assert same(xy, rxy) and same(yaw, ryaw), b
        if res["ok"][b]:
            exy, eyaw = path_points(T, coef, 3, ft.start_xytheta[:2], **model)
            assert xy.shape == exy.shape and np.max(np.abs(xy - exy)) < 1e-10 and np.max(np.abs(yaw - eyaw)) < 1e-10, b
        else:
            assert xy.shape[0] == 0
    assert moved >= 6       # the ICR classes integrate another path than xv = 0 does


def test_set_paths_builds_with_the_class_front_end(sc):
    from alore_legged_manipulator_amd.flat_traj import FrontEndParams
    fe = [FrontEndParams() for _ in range(NK)]
    fe[2] = FrontEndParams(max_vel=2.0, max_acc=1.0)
    paths = [np.array([ft.start_xytheta[:2], ft.final_xytheta[:2]]) for ft in sc["fts"]]
    sy = [float(ft.start_xytheta[2]) for ft in sc["fts"]]
    ey = [float(ft.final_xytheta[2]) for ft in sc["fts"]]
    pl = planner(sc["grid"], len(INTERLEAVED), max_pieces=32)     # the slower trapezoid of k2 takes more than 16 samples
    pl.set_classes(sc["cfgs"], front_end=fe)
    pl.set_problem_classes(np.array([k for _, k in INTERLEAVED], np.int32))
    args = ([paths[p] for p, _ in INTERLEAVED], [sy[p] for p, _ in INTERLEAVED], [ey[p] for p, _ in INTERLEAVED])
    pl.set_paths(*args)
    got = pl.problems()
    override = None
    for b, (p, k) in enumerate(INTERLEAVED):
        one = planner(sc["grid"], 1, sc["cfgs"][k], max_pieces=32)
        one.set_paths([paths[p]], [sy[p]], [ey[p]], params=fe[k])
        ref = one.problems()
        for f in ref:
            assert same(got[f][b], ref[f][0]), (b, f)
        one.close()
    for p in range(NP_):
        assert got["init_T"][p * NK + 2] != got["init_T"][p * NK], p          # the heavier class starts from a longer trapezoid
        assert got["init_T"][p * NK + 1] == got["init_T"][p * NK], p
    # a non-NULL fe argument applies to every slot
    pl.set_paths(*args, params=fe[2])
    override = pl.problems()
    for p in range(NP_):
        assert len({override["init_T"][p * NK + k] for k in range(NK)}) == 1 and override["init_T"][p * NK] == got["init_T"][p * NK + 2]
    pl.close()


def test_device_route_of_set_problem_classes(sc):
    import torch
    from alore_legged_manipulator_amd.backend import BackendError
    pl = planner(sc["grid"], len(INTERLEAVED))
    pl.set_classes(sc["cfgs"])
    pl.set_problem_classes(torch.tensor([k for _, k in INTERLEAVED], dtype=torch.int32, device="cuda"))
    pl.set_problems([sc["fts"][p] for p, _ in INTERLEAVED])
    pl.plan()
    res = full(pl)
    for k in STATUS + SLABS:
        assert same(res[k], sc["mixed_res"][k]), k
    assert pl.class_state(12)["clamped"] == 0
    # two indices out of range: clamped into the table and counted
    idx = [k for _, k in INTERLEAVED]
    idx[1], idx[6] = -1, 9          # slot 1: problem 0, slot 6: problem 1
    pl.set_problem_classes(torch.tensor(idx, dtype=torch.int32, device="cuda"))
    st = pl.class_state(12)
    assert st["clamped"] == 2 and st["class_of"][1] == 0 and st["class_of"][6] == 3
    assert st["xv"][1] == 0.0 and st["xv"][6] == cases.effective_xv(sc["cfgs"][3])
    pl.plan()
    res = full(pl)
    assert_slot_equals(res, 1, sc["single_res"][0, 0], "clamped to 0")
    assert_slot_equals(res, 6, sc["single_res"][1, 3], "clamped to 3")
    # the host route refuses such an index and changes nothing
    before = pl.class_state(12)
    for bad in (-1, 4):
        host = [0] * 12
        host[5] = bad
        with pytest.raises(BackendError, match="slot 5"):
            pl.set_problem_classes(np.array(host, np.int32))
    after = pl.class_state(12)
    assert after["class_of"].tolist() == before["class_of"].tolist() and after["clamped"] == 2
    # a class that does not fit the handle is refused by name, and the table of before stays
    bad_cfgs = cases.class_configs()
    bad_cfgs[2].n_check = 9
    with pytest.raises(BackendError, match=r"class 2: n_check"):
        pl.set_classes(bad_cfgs)
    bad_cfgs = cases.class_configs()
    bad_cfgs[1].sparse_res = 4
    with pytest.raises(BackendError, match=r"class 1: sparse_res"):
        pl.set_classes(bad_cfgs)
    assert pl.class_state(12)["n_classes"] == NK
    pl.close()


def status_arrays(res):
    return {k: res[k] for k in ("ok", "attempts", "evals", "collision", "n_pieces", "min_dist")}


def test_class_stats_equal_numpy(sc):
    import torch
    mixed = sc["mixed"]
    class_of = np.array([k for _, k in INTERLEAVED])
    got = mixed.class_stats()
    ref = cases.stats_numpy(class_of, status_arrays(sc["mixed_res"]), sc["mixed_res"]["T"], NK)
    assert got.tobytes() == ref.tobytes(), (got, ref)
    assert got["n"].tolist() == [3] * NK and got["n_ok"][:3].tolist() == [3, 3, 3]
    assert got["n_ok"][3] < 3 and got["n_collision"][3] > 0 and got["sum_attempts"][3] > 3
    assert got["max_duration"][2] > got["max_duration"][0] > 0.0
    # after a masked launch that replans the k1 slots alone: the records of the other slots stay, so do the statistics
    mask = torch.tensor((class_of == 1).astype(np.int32), device="cuda")
    mixed.plan(mask=mask)
    res = full(mixed)
    again = mixed.class_stats()
    assert again.tobytes() == cases.stats_numpy(class_of, status_arrays(res), res["T"], NK).tobytes()
    for k in STATUS + SLABS:
        assert same(res[k], sc["mixed_res"][k]), k            # a replan of the same problem with the same class: the same bits
    # without a table: one class, every slot
    single = sc["single"][0, 2]
    one = single.class_stats()
    assert one.shape == (1,) and one.tobytes() == cases.stats_numpy(np.zeros(1, int), status_arrays(sc["single_res"][0, 2]),
                                                                     sc["single_res"][0, 2]["T"], 1).tobytes()
    # fetch=False leaves the records in the slab of the view
    from alore_legged_manipulator_amd.backend import CLASS_STAT_DTYPE, _DeviceArray
    mixed.class_stats(fetch=False)
    torch.cuda.synchronize()
    slab = torch.as_tensor(_DeviceArray(mixed.class_view().stats, (NK * CLASS_STAT_DTYPE.itemsize,), "|u1"), device="cuda").cpu().numpy()
    assert slab.tobytes() == again.tobytes()


def engine(n):
    from alore_legged_manipulator_amd.nmpc import BatchedNmpc
    eng = BatchedNmpc(n, 20, 0.01)
    eng.refs_init(max_pieces=16, max_checkpoints=256)
    return eng


def entry(eng, b, pending=False):
    d = eng.refs_download(b, pending=pending)
    return {k: np.asarray(d[k]) for k in ("start_time", "duration", "xv", "res", "valid", "durations", "coeffs", "checkpoints")}


def test_hand_over_carries_the_xv_of_every_slot(sc):
    import torch
    mixed, res = sc["mixed"], sc["mixed_res"]
    n = len(INTERLEAVED)
    xv = mixed.class_xv()
    assert xv.dtype == torch.float64 and xv.is_cuda and xv.shape == (n,)
    eng = engine(n)
    empty = [entry(eng, b) for b in range(n)]
    eng.refs_set_from_backend(mixed, xv=xv, traj_start_time=0.25)
    pend = engine(n)
    mask = torch.tensor([1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1], dtype=torch.int32, device="cuda")
    pend.refs_set_pending_from_backend(mixed, mask=mask, traj_start_time=0.25, xv=xv)
    pend.refs_promote(0.5)
    failed = 0
    for b, (p, k) in enumerate(INTERLEAVED):
        got = entry(eng, b)
        if not res["ok"][b]:                                    # a rejected plan leaves its slot as it was
            failed += 1
            assert all(same(got[f], empty[b][f]) for f in got) and not got["valid"], b
            continue
        want = cases.effective_xv(sc["cfgs"][k])
        assert got["valid"] and got["xv"] == want, (b, got["xv"], want)
        ref_eng = engine(1)
        ref_eng.refs_set_from_backend(sc["single"][p, k], xv=want, traj_start_time=0.25)   # the scalar call, the single-class handle
        ref = entry(ref_eng, 0)
        for f in got:
            assert same(got[f], ref[f]), (b, f)
        promoted = entry(pend, b)
        if mask[b].item():
            for f in got:
                assert same(promoted[f], ref[f]), (b, f, "pending route")
        else:
            assert not promoted["valid"], b
    assert failed >= 1
    # the scalar route leaves what it always left: a float for every slot, on a handle with and without a table
    plain = planner(sc["grid"], NP_)
    plain.set_problems(sc["fts"])
    plain.plan()
    a, b_ = engine(NP_), engine(NP_)
    a.refs_set_from_backend(plain, xv=0.15)
    plain.set_classes(sc["cfgs"][:1])
    plain.plan()
    b_.refs_set_from_backend(plain, xv=0.15)
    for s in range(NP_):
        ea, eb = entry(a, s), entry(b_, s)
        assert ea["xv"] == 0.15 and all(same(ea[f], eb[f]) for f in ea), s


def test_a_tensor_xv_passes_through_replan_cycle(sc):
    """replan.replan_cycle forwards xv as it comes: with planner.class_xv() the pending entry of a replanned robot carries its
    class's xv.  A disc is put on the planned path of slot 0 and one cycle runs."""
    import torch
    from alore_legged_manipulator_amd.replan import replan_cycle
    n = len(INTERLEAVED)
    pl = mixed_planner(sc, INTERLEAVED)
    pl.plan()
    eng = engine(n)
    xv = pl.class_xv()
    eng.refs_set_from_backend(pl, xv=xv)
    path = pl.path_points(3, n)[0][0]
    moved = cases.disc_grid([tuple(path[len(path) // 2])] + cases.disc_centres(sc["fts"])[1:])
    pl.set_map(moved.dist, moved.x_lo, moved.y_lo, moved.res)
    goals = torch.tensor(np.array([sc["fts"][p].final_xytheta[:2] for p, _ in INTERLEAVED]), dtype=torch.float64, device="cuda")
    end_yaw = torch.tensor([sc["fts"][p].final_xytheta[2] for p, _ in INTERLEAVED], dtype=torch.float64, device="cuda")
    w = replan_cycle(pl, eng, 0.1, 0.05, goals, end_yaw, start_times=0.0, xv=xv)
    torch.cuda.synchronize()
    mask = w.mask[:n].cpu().numpy()
    assert mask.any(), (mask, pl.check_plans(fetch=True)["collision"], pl.search_status(n), pl.build_status(n), pl.results(n)["ok"])
    for b in np.nonzero(mask)[0]:
        d = eng.refs_download(int(b), pending=True)
        assert d["valid"] and d["start_time"] == 0.1 + 0.05 and d["xv"] == cases.effective_xv(sc["cfgs"][INTERLEAVED[b][1]]), b
    pl.close()


def test_a_tensor_xv_passes_through_manager_cycle(sc):
    """replan.manager_cycle forwards xv as it comes: the FRESH plans of one period are delivered with the xv of their classes"""
    import torch
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner
    from alore_legged_manipulator_amd.replan import manager_cycle
    start = np.array([[-1.5, -2.5, 0.0], [-1.5, 2.5, 0.0], [-2.0, 0.0, 0.0], [3.0, 4.5, 0.0]])
    goal = np.array([[1.5, -2.5, 0.0], [1.5, 2.5, 0.0], [2.0, 0.5, 0.0], [0.0, 0.0, 0.0]])
    class_of = [1, 2, 3, 0]
    pl = BatchedMSPlanner(4, 16)
    pl.set_free_map(half=6.4)
    pl.set_classes(sc["cfgs"])
    pl.set_problem_classes(np.array(class_of, np.int32))
    pl.manager_create(replan_time=1.0, max_replan_time=0.5)
    eng = engine(4)
    pl.manager_request(start, goal, np.array([1, 1, 1, 0], np.int32))
    manager_cycle(pl, eng, 10.0, torch.as_tensor(start).cuda(), nmpc_plant=False, xv=pl.class_xv())
    torch.cuda.synchronize()
    ok = pl.results(4)["ok"]
    assert ok[:3].tolist() == [1, 1, 1]
    for b in range(3):
        d = eng.refs_download(b, pending=True)
        assert d["valid"] and d["start_time"] == 10.0 and d["xv"] == cases.effective_xv(sc["cfgs"][class_of[b]]), b
    assert not eng.refs_download(3, pending=True)["valid"]
    pl.close()


def test_config4_with_the_model_carried_through():
    """configs[4], the small case of tests/test_config4_pipeline.py: 4 classes x 16 robots on a free map, the planner classes with
    the ICR of that file's CLASSES, the store filled with class_xv(), the plant with the same ICR; closed loop to the end of the
    plans.  Every tick solves and every robot reaches its goal flag.  The route of before (planner and store at xv = 0) runs too;
    which route ends closer is reported (profiles/backend_classes.txt), not asserted."""
    from alore_legged_manipulator_amd.backend import BatchedMSPlanner, default_config
    from alore_legged_manipulator_amd.flat_traj import monte_carlo_goals
    from alore_legged_manipulator_amd.nmpc import BatchedNmpc
    from tests.test_config4_pipeline import CLASSES
    per, N, dt = 16, 20, 0.01
    B = 4 * per
    fts = monte_carlo_goals(B, seed=44)
    icr = np.array([CLASSES[b % 4] for b in range(B)])
    pose0 = np.array([ft.start_xytheta for ft in fts])
    final = np.array([ft.final_xytheta for ft in fts])
    W = np.tile(np.diag([10, 10, 0.5, 0.1, 0.1]).astype(np.float32), (B, N, 1, 1))
    WN = np.tile(np.diag([10, 10, 0.5]).astype(np.float32), (B, 1, 1))
    report = {}
    for route in ("classes", "xv = 0"):
        pl = BatchedMSPlanner(B, 16)
        pl.set_free_map(half=20.0)
        if route == "classes":
            cfgs = []
            for xv, _, _ in CLASSES:
                c = default_config()
                c.standard_diff, c.icr_xv = 0, xv
                cfgs.append(c)
            pl.set_classes(cfgs)
            pl.set_problem_classes(np.arange(B, dtype=np.int32) % 4)
        res = pl.minco_plan(fts)
        assert np.all(res["ok"] == 1)
        eng = BatchedNmpc(B, N, dt)
        eng.load({"W": W, "WN": WN})
        eng.refs_init(max_pieces=16, max_checkpoints=128)
        eng.refs_set_from_backend(pl, xv=pl.class_xv() if route == "classes" else 0.0)
        if route == "classes":
            assert [eng.refs_download(b)["xv"] for b in range(8)] == [CLASSES[b % 4][0] for b in range(8)]
        eng.plant_init()
        eng.plant_set_state(pose0, icr)
        eng.closed_loop_reset()
        ticks = int((float(res["T"].sum(1).max()) + 1.5) / dt)
        status_ok, done, chunk = True, 0, 100
        while done < ticks:                                  # the status of every tick: read after every chunk of ticks
            m = min(chunk, ticks - done)
            for i in range(m):
                eng.closed_loop_tick(0.05 + (done + i) * dt, delay_num=1)
                status_ok = status_ok & (eng.t["status"] == 0).all()
            done += m
        assert bool(status_ok), route
        pose, vw, goal = eng.plant_get_state()
        dist = np.hypot(pose[:, 0] - final[:, 0], pose[:, 1] - final[:, 1])
        assert np.all(goal), route
        report[route] = (float(np.median(dist)), float(dist.max()))
        pl.close()
    print("\nconfigs[4], 4 x 16 robots, distance to the goal at the end, median / max [m]: " +
          "; ".join(f"{k}: {v[0]:.4f} / {v[1]:.4f}" for k, v in report.items()))
