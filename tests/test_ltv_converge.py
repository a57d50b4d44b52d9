"""LTV-MPC with the reference's stopping rule (alore_ltv_get_cmd_converge / _tick_converge, include/alore_ltv_mpc.h):
relinearise until du = sum |change of the output| <= du_th (mpc_controller/src/mpc.cpp:581-584), per robot.
The oracle side drives oracle.ltv_mpc_oracle.solve_mpcv pass by pass, records the du history and stops by the same rule; its
own commands drive the plant.  The dense oracle takes 40 - 80 s per set-up (some 200 QPs each), so what it computes is kept
in tests/golden/ltv_converge_oracle.npz (`python tests/test_ltv_converge.py` writes it anew with scenario() below); a CPU
test recomputes a sample of it with the live oracle, so the file cannot drift from the code that made it."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

from oracle.ltv_mpc_oracle import LtvParams, linear_model, predict_motion, solve_mpcv

DU_TH = 0.01          # the reference's du_threshold
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ltv_converge_oracle.npz")
TOL = 1e-6            # test_gpu_get_cmd_tracks_the_oracle_over_relinearisations_and_ticks
IP = C.POINTER(C.c_int)
DP = C.POINTER(C.c_double)


def arc(p, v, w, t0):
    ts = t0 + (np.arange(p.T) + 1) * p.dt
    return (np.stack([v / w * np.sin(w * ts), v / w * (1 - np.cos(w * ts)), w * ts]), np.stack([np.full(p.T, v), np.full(p.T, w)]))


def converge_oracle(now, output, buff, xref, dref, p, max_relin, du_th):
    """getCmd with `du <= du_th` as the stopping rule: (output, buffer, count, du of every pass run)"""
    hist, count = [], -max_relin
    for k in range(1, max_relin + 1):
        new, _, info, _ = solve_mpcv(now, output, buff, xref, dref, p)
        assert max(info.values()) < 1e-7
        hist.append(float(np.abs(new - output).sum()))
        output = new
        if hist[-1] <= du_th:
            count = k
            break
    nb = list(buff)
    if p.delay_num > 0:
        nb = nb[1:] + [output[:, p.delay_num].copy()]
    return output, nb, count, hist


def xopt_oracle(now, output, p):
    """predictMotion(xopt), mpc.cpp:271-302, about the rollout of `output`"""
    xbar = predict_motion(now, output, p)
    x = [np.array(now[:3], float)]
    for i in range(1, p.T + 1):
        A, Bm, Cm = linear_model(xbar[i - 1], p)
        x.append(A @ x[-1] + Bm @ output[:, i - 1] + Cm)
    return np.array(x)


def scenario(T, delay, B, seed, max_relin, du_th, ticks, off_every=2):
    """B robots on arcs, every `off_every`-th one starting 0.3 m / 0.5 rad off its reference, the others on it; a cold tick
    (reset) and warm ones, the plant driven by the oracle's own commands.  Per tick: states, refs, and per robot the oracle's
    output, delay buffer, count and du history."""
    p = LtvParams(T=T, delay_num=delay)
    rng = np.random.default_rng(seed)
    specs = [(rng.uniform(0.5, 2.5), rng.uniform(0.3, 1.5) * rng.choice([-1.0, 1.0])) for _ in range(B)]
    state = np.zeros((B, 3))
    for b in range(B):
        if b % off_every == 1:
            a = rng.uniform(0, 2 * math.pi)
            state[b] = [0.3 * math.cos(a), 0.3 * math.sin(a), 0.5 * rng.choice([-1.0, 1.0])]
    out = [np.zeros((2, T)) for _ in range(B)]
    buff = [[np.zeros(2) for _ in range(delay)] for _ in range(B)]
    rec = []
    for tick in range(ticks):
        refs = [arc(p, v, w, tick * p.dt) for v, w in specs]
        row = {"state": state.copy(), "xref": np.stack([r[0].T for r in refs]), "dref": np.stack([r[1].T for r in refs]),
               "out": [], "buff": [], "count": [], "hist": [], "xopt": []}
        for b in range(B):
            now = list(state[b]) + [0.0]
            out[b], buff[b], k, hist = converge_oracle(now, out[b], buff[b], refs[b][0], refs[b][1], p, max_relin, du_th)
            row["out"].append(out[b].T.copy()); row["buff"].append([x.copy() for x in buff[b]]); row["count"].append(k); row["hist"].append(hist)
            row["xopt"].append(xopt_oracle(now, out[b], p))
            v, w = out[b][:, delay]
            state[b] += [v * math.cos(state[b, 2]) * p.dt, v * math.sin(state[b, 2]) * p.dt, w * p.dt]
        rec.append(row)
    return p, rec


# (T, delay, B, seed, max_relin, du_th).  du_th: the reference's 0.01, except at delay 0, where 0.1 makes the robots that start on
# their reference stop after ONE pass within the three warm ticks (their first-pass du is 0.03 - 0.06 there and shrinks slowly)
ORACLE_SETUPS = [(30, 0, 13, 101, 8, 0.1), (30, 1, 13, 102, 8, DU_TH), (30, 3, 13, 103, 8, DU_TH), (50, 1, 5, 104, 6, DU_TH)]
TICKS = 4
FIELDS = ("state", "xref", "dref", "out", "buff", "count", "hist", "xopt")


def pack(p, rec, max_relin):
    """the records of scenario() as arrays: hist padded with NaN to max_relin, buff to at least one row"""
    d = {}
    for f in ("state", "xref", "dref", "out", "xopt", "count"):
        d[f] = np.array([row[f] for row in rec])
    d["buff"] = np.array([[np.array(bf).reshape(-1, 2) if len(bf) else np.zeros((1, 2)) for bf in row["buff"]] for row in rec])
    d["hist"] = np.array([[h + [np.nan] * (max_relin - len(h)) for h in row["hist"]] for row in rec])
    return d


@functools.lru_cache(maxsize=None)
def golden(T, delay):
    z = np.load(GOLDEN)
    return {f: z[f"T{T}_d{delay}_{f}"] for f in FIELDS}


def check_not_borderline(g, du_th):
    """A count can only be compared if no oracle du sits on the threshold: every du_k of every case is more than 1e-3
    (relative) away from du_th.  A condition on the inputs, not a tolerance."""
    du = g["hist"][np.isfinite(g["hist"])]
    assert np.all(np.abs(du - du_th) > 1e-3 * du_th), du[np.abs(du - du_th) <= 1e-3 * du_th]


def test_oracle_counts_are_not_borderline_and_cover_one_two_and_more_passes():
    counts = set()
    for T, delay, B, seed, max_relin, du_th in ORACLE_SETUPS:
        g = golden(T, delay)
        assert g["count"].shape == (TICKS, B) and g["hist"].shape == (TICKS, B, max_relin)
        check_not_borderline(g, du_th)
        # the counts follow from the du histories by the rule
        for k, h in zip(g["count"].reshape(-1), g["hist"].reshape(-1, max_relin)):
            n = int(np.isfinite(h).sum())
            assert np.all(h[:n - 1] > du_th) and ((k == n and h[n - 1] <= du_th) or (k == -max_relin and n == max_relin and h[n - 1] > du_th))
        counts |= {min(abs(int(k)), 3) for k in g["count"].reshape(-1)}
    assert counts == {1, 2, 3}, counts
    assert np.any(golden(50, 1)["count"] < 0)      # and one robot of the long horizon never meets the threshold


def test_golden_oracle_records_are_what_the_live_oracle_computes():
    """a sample: the cold tick and the first warm tick of two robots (one on its reference, one off), delay 1"""
    T, delay, B, seed, max_relin, du_th = ORACLE_SETUPS[1]
    g = golden(T, delay)
    p = LtvParams(T=T, delay_num=delay)
    for tick, b in ((0, 0), (1, 1)):
        out = np.zeros((2, T)) if tick == 0 else g["out"][tick - 1, b].T.copy()
        buff = [np.zeros(2)] if tick == 0 else [g["buff"][tick - 1, b, 0].copy()]
        o, nb, k, hist = converge_oracle(list(g["state"][tick, b]) + [0.0], out, buff, g["xref"][tick, b].T, g["dref"][tick, b].T, p, max_relin, du_th)
        assert k == g["count"][tick, b] and np.allclose(hist, g["hist"][tick, b, :len(hist)], rtol=0, atol=1e-9)
        assert np.allclose(o.T, g["out"][tick, b], rtol=0, atol=1e-9) and np.allclose(nb[0], g["buff"][tick, b, 0], rtol=0, atol=1e-9)
        assert np.allclose(xopt_oracle(list(g["state"][tick, b]) + [0.0], o, p), g["xopt"][tick, b], rtol=0, atol=1e-9)


def engine(p, B):
    from alore_legged_manipulator_amd.ltv_mpc import BatchedLtvMpc, default_config
    return BatchedLtvMpc(B, default_config(predict_steps=p.T, delay_num=p.delay_num))


def against_oracle(T, delay, B, seed, max_relin, du_th):
    g = golden(T, delay)
    check_not_borderline(g, du_th)
    p = LtvParams(T=T, delay_num=delay)
    eng = engine(p, B)
    for tick in range(TICKS):
        eng.set_refs(g["xref"][tick], g["dref"][tick])
        got = eng.get_cmd_converge(g["state"][tick], max_relin=max_relin, du_th=du_th, reset=(tick == 0))
        assert np.all(got["status"] == 0)
        du_o = np.array([h[np.isfinite(h)][-1] for h in g["hist"][tick]])
        err = {"output": np.max(np.abs(got["output"] - g["out"][tick])), "xopt": np.max(np.abs(got["xopt"] - g["xopt"][tick])),
               "du": np.max(np.abs(got["du"] - du_o))}
        print(f"T {T} delay {delay} tick {tick}: counts gpu {got['relin_iters'].tolist()} oracle {g['count'][tick].tolist()}  errors {err}")
        assert got["relin_iters"].tolist() == g["count"][tick].tolist(), (tick, got["relin_iters"], g["count"][tick])
        assert eng.relin_iters is got["relin_iters"] and eng.du is got["du"]
        assert err["output"] < TOL and err["xopt"] < TOL and err["du"] < TOL, (tick, err)
        assert np.max(np.abs(got["cmd"] - g["out"][tick][:, delay])) < TOL
        # the delay buffer a tick leaves is what the next one copies into its first delay_num columns -- covered by `output` of
        # the next tick; the last tick's buffer is read the same way below
    if delay:
        nxt = eng.get_cmd(g["state"][-1], n_relin=1)
        assert np.max(np.abs(nxt["output"][:, :delay] - g["buff"][-1])) < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("delay", [0, 1, 3])
def test_gpu_counts_and_results_match_the_oracle(delay):
    """B = 13: the last wavefront holds one real robot and three padding groups that shadow it."""
    against_oracle(*ORACLE_SETUPS[[0, 1, 3].index(delay)])


@pytest.mark.gpu
def test_gpu_long_horizon_matches_the_oracle():
    """T = 50: the four-stages-per-lane instantiation"""
    against_oracle(*ORACLE_SETUPS[3])


def arc_batch(p, specs):
    refs = [arc(p, v, w, 0.0) for v, w in specs]
    return np.stack([r[0].T for r in refs]), np.stack([r[1].T for r in refs])


@pytest.mark.gpu
def test_gpu_finished_robots_are_frozen_next_to_a_mate_that_goes_on():
    """One wavefront: three robots on their references (warm: the previous output is the reference input), one far off.  The
    three stop early and keep, bit for bit, what alore_ltv_get_cmd with n_relin = their own count computes."""
    p = LtvParams()
    specs = [(1.0, 0.5), (1.5, -0.8), (2.0, 0.4), (1.2, 0.9)]
    xref, dref = arc_batch(p, specs)
    state = np.zeros((4, 3)); state[3] = [0.25, -0.2, 0.5]
    warm = dref.copy()                      # (4, T, 2): v, omega of the arc
    buff = warm[:, :p.delay_num].copy()

    def fresh():
        e = engine(p, 4); e.set_refs(xref, dref); e.set_state(warm, buff)
        return e
    got = fresh().get_cmd_converge(state, max_relin=8, du_th=DU_TH)
    k = got["relin_iters"]
    print("counts", k, "du", got["du"])
    assert np.all(k[:3] >= 1) and np.all(k[:3] <= 2) and abs(k[3]) > max(k[:3]), k
    for n in sorted(set(k[:3].tolist())):
        want = fresh().get_cmd(state, n_relin=n)
        for b in np.nonzero(k[:3] == n)[0]:
            assert np.array_equal(got["output"][b], want["output"][b]) and np.array_equal(got["xopt"][b], want["xopt"][b]), b
            assert got["sweeps"][b] == want["sweeps"][b] and got["status"][b] == want["status"][b]


@pytest.mark.gpu
def test_gpu_threshold_never_met_runs_every_pass():
    """du_th = 0 stops only on an exactly repeated output: off-reference robots run all max_relin = 3 passes, report -3, leave the
    bits of get_cmd(n_relin = 3), and du is the oracle's third-pass value."""
    p = LtvParams()
    B = 4
    rng = np.random.default_rng(5)
    specs = [(rng.uniform(0.5, 2.5), rng.uniform(0.3, 1.5)) for _ in range(B)]
    xref, dref = arc_batch(p, specs)
    state = np.array([[0.3 * math.cos(b), 0.3 * math.sin(b), 0.5 * (-1) ** b] for b in range(B)])
    a = engine(p, B); a.set_refs(xref, dref)
    got = a.get_cmd_converge(state, max_relin=3, du_th=0.0, reset=True)
    b_ = engine(p, B); b_.set_refs(xref, dref)
    want = b_.get_cmd(state, n_relin=3, reset=True)
    assert np.all(got["relin_iters"] == -3), got["relin_iters"]
    for key in ("output", "xopt", "sweeps", "status", "cmd"):
        assert np.array_equal(got[key], want[key]), key
    for b in range(B):
        _, _, count, hist = converge_oracle(list(state[b]) + [0.0], np.zeros((2, p.T)), [np.zeros(2)], xref[b].T, dref[b].T, p, 3, 0.0)
        assert count == -3 and abs(got["du"][b] - hist[2]) < TOL, (b, got["du"][b], hist)


@pytest.mark.gpu
def test_gpu_non_finite_robot_is_finished_from_the_start():
    p = LtvParams()
    B = 7
    rng = np.random.default_rng(8)
    specs = [(rng.uniform(0.5, 2.5), rng.uniform(0.3, 1.5)) for _ in range(B)]
    xref, dref = arc_batch(p, specs)
    state = np.array([[0.1 * math.cos(b), 0.1 * math.sin(b), 0.2 * (-1) ** b] for b in range(B)])

    def run(st):
        e = engine(p, B); e.set_refs(xref, dref)
        return e.get_cmd_converge(st, max_relin=6, du_th=DU_TH, reset=True)
    clean = run(state)
    bad = state.copy(); bad[2, 1] = np.nan
    got = run(bad)
    assert got["status"][2] == 2 and got["relin_iters"][2] == 0 and got["du"][2] == 0.0 and np.all(got["cmd"][2] == 0.0)
    mates = [b for b in range(B) if b != 2]
    assert np.all(got["status"][mates] == 0)
    for key in ("output", "xopt", "relin_iters", "du", "sweeps", "cmd"):
        assert np.array_equal(got[key][mates], clean[key][mates]), key


@pytest.mark.gpu
def test_gpu_tick_converge_returns_what_the_separate_calls_return():
    p = LtvParams()
    B = 9
    rng = np.random.default_rng(9)
    specs = [(rng.uniform(0.5, 2.5), rng.uniform(0.3, 1.5)) for _ in range(B)]
    xref, dref = arc_batch(p, specs)
    state = np.array([[0.2 * math.cos(b), 0.2 * math.sin(b), 0.3 * (-1) ** b] if b % 2 else [0.0, 0.0, 0.0] for b in range(B)])
    a = engine(p, B); a.set_refs(xref, dref)
    t = engine(p, B); t.set_refs(xref, dref)
    for tick in range(2):
        a.get_cmd_converge(state, max_relin=8, du_th=DU_TH, reset=(tick == 0))
        cmd = np.zeros((B, 2)); st = np.zeros(B, np.int32); it = np.zeros(B, np.int32); du = np.zeros(B)
        a._check(a.L.alore_ltv_commands(a.h, B, cmd.ctypes.data_as(DP), st.ctypes.data_as(IP), None))
        a._check(a.L.alore_ltv_relin_info(a.h, B, it.ctypes.data_as(IP), du.ctypes.data_as(DP), None))
        cmd_t, st_t, it_t = t.tick_converge(state, max_relin=8, du_th=DU_TH, reset=(tick == 0))
        assert np.array_equal(cmd_t, cmd) and np.array_equal(st_t, st) and np.array_equal(it_t, it)
        assert np.array_equal(t.relin_iters, it) and np.array_equal(t.du, du) and len(set(it.tolist())) > 1


@pytest.mark.gpu
def test_gpu_bad_arguments_are_refused_with_a_message():
    from alore_legged_manipulator_amd.ltv_mpc import LtvError
    p = LtvParams()
    e = engine(p, 4)
    state = np.zeros((4, 3))
    for kw in ({"max_relin": 0}, {"du_th": -1.0}, {"du_th": float("nan")}):
        for call in (e.get_cmd_converge, e.tick_converge):
            with pytest.raises(LtvError) as err:
                call(state, **kw)
            assert "error -1" in str(err.value) and "converge: " in str(err.value), str(err.value)
        cmd = np.zeros((4, 2))
        args = {"max_relin": 150, "du_th": 0.01, **kw}
        rc = e.L.alore_ltv_tick_converge(e.h, 4, state.ctypes.data_as(DP), args["max_relin"], args["du_th"], 0, cmd.ctypes.data_as(DP), None, None, None)
        assert rc == -1 and len(e.L.alore_ltv_last_error(e.h)) > 0


if __name__ == "__main__":      # regenerate tests/golden/ltv_converge_oracle.npz (minutes: the dense oracle)
    arrays = {}
    for T_, delay_, B_, seed_, max_relin_, du_th_ in ORACLE_SETUPS:
        p_, rec_ = scenario(T_, delay_, B_, seed_, max_relin_, du_th_, TICKS)
        for f_, a_ in pack(p_, rec_, max_relin_).items():
            arrays[f"T{T_}_d{delay_}_{f_}"] = a_
        print(T_, delay_, [row["count"] for row in rec_], flush=True)
    np.savez_compressed(GOLDEN, **arrays)
