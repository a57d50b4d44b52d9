"""Whole-body class on the GPU at horizons N = 1 .. 32 on problems that change from stage to stage (tests/wb_cases.py:
make_varied_problems): every stage has its own A_k, B_k, d_k, gx_k, a non-zero input gradient gu_k = R (u_k - uref_k) and
dx0 = x0 - x_0 != 0, so a stage off by one in the kernels' look-ahead loads, in the stored gains or in the forward sweep,
or a dropped dx0 / gu term, moves the step far past the bounds (the discriminators below show by how much).

Each compared step uses the kernel's own A and B (eng.linearize()) with float64 defects and gradients, as the N = 20 tests
of tests/test_wb_gpu.py do, and the same bounds.  Two conditions on the inputs are asserted beside each comparison; they
use only the references, never the kernel:
  - riccati_f32 (oracle/wb_oracle.py: solve_lq_clamped on float32 arrays, a restatement of the sweep on float32 data; its
    docstring says which of its arithmetic is float32) stays within F32_CAP = 5e-5, half the 1e-4 bound, of the float64
    solve: the inputs are not so ill-conditioned that float32 cannot meet the bound;
  - the discriminators (the float64 reference solved again with A and B rolled by one stage, and with dx0 = 0) differ
    from the reference by at least DISC_MIN = 1e-2, 100 x the bound: the inputs do tell those bugs apart.
A and B are rolled by one stage in the batch's memory order (problem, stage): stage k gets A_{k+1}, the last stage the
first stage of the next problem -- what an index off by one reads -- so the discriminator exists at N = 1 too."""
import math

import numpy as np
import pytest

from oracle.wb_oracle import (contact_penalty, linearize, solve_lq, solve_lq_clamped, solve_lq_contact_rows,
                              solve_lq_inequality, step)
from tests.wb_cases import make_varied_problems, weights

pytestmark = pytest.mark.gpu

B, DT = 3, 0.01                   # three distinct problems
HORIZONS = (1, 2, 3, 7, 32)
SEED, AMP = 26, 0.25              # inputs of every part; the conditions below hold for them (tests/test_wb_oracle.py)
BOUND = 1e-4                      # the N = 20 tests' bound on the float32 sweep against the float64 solve
F32_CAP = 0.5 * BOUND
DISC_MIN = 1e-2
MU = 0.15
RHO = 200.0
# half the arm offset of the N = 20 torque-limit test: still several clamps per stage, and dx0 stays visible in the step
ARM_OFFSET = np.array([0.45, -0.4, 0.45, -0.35, 0.4, -0.45])


@pytest.fixture(scope="module")
def model():
    from oracle.wb_oracle import Model
    return Model()


# ---- reference-only helpers ------------------------------------------------------------------------------------------
def scenario(model, N, kind):
    """(x0, xref, uref, xi, ui, Q, R, QN, stance) of one part.  Every kind starts from the same generator inputs, so the
    iterate and its linearisation are the same; they differ in the reference and the weights:
      plain    -- weights() and the generator's reference
      torque   -- an arm posture far away with stiff weights: more joint torque than the URDF allows (torque limits)
      pyramid  -- the base 25 cm to the side with stiff weights on a slippery floor (friction pyramid, MU)
    stance: problem b lifts foot b from stage ceil(N / 2) on (used by the parts with contacts)."""
    x0, xref, uref, xi, ui = make_varied_problems(model, B, N, seed=SEED, amp=AMP)
    Q, R, QN = weights()
    Q = Q.copy()
    xref = xref.copy()
    if kind == "torque":
        xref[:, :, 18:24] += ARM_OFFSET
        Q[18:24] = 4000.0; QN = 10 * Q
    elif kind == "pyramid":
        xref[:, :, 1] += 0.25
        Q[:3] = 5000.0; QN = 10 * Q
    stance = np.ones((B, N, 4), np.uint8)
    for b in range(B):
        stance[b, math.ceil(N / 2):, b] = 0
    return x0, xref, uref, xi, ui, Q, R, QN, stance


def oracle_lin(model, xi, ui):
    """A, B, next of every (problem, stage) from the oracle's own float64 dynamics and linearisation"""
    nb, N = ui.shape[:2]
    A, Bm, nxt = np.zeros((nb, N, 48, 48)), np.zeros((nb, N, 48, 30)), np.zeros((nb, N, 48))
    for b in range(nb):
        for k in range(N):
            A[b, k], Bm[b, k] = linearize(model, xi[b, k], ui[b, k], DT)
            nxt[b, k] = step(model, xi[b, k], ui[b, k], DT)
    return A, Bm, nxt


def lq_inputs(lin, x0, xref, uref, xi, ui, Q, R, QN, b):
    """the LQ problem of one real-time iteration of problem b from a linearisation (A, B, next) [B][N]: float64 defects
    and gradients; the argument list of solve_lq"""
    A, Bm, nxt = lin
    N = A.shape[1]
    d = [nxt[b, k] - xi[b, k + 1] for k in range(N)]
    gx = [Q * (xi[b, k] - xref[b, k]) for k in range(N)]
    gu = [R * (ui[b, k] - uref[b, k]) for k in range(N)]
    gN = QN * (xi[b, N] - xref[b, N])
    return [list(A[b]), list(Bm[b]), d, np.diag(Q), np.diag(R), np.diag(QN), gx, gu, gN, x0[b] - xi[b, 0]]


def rolled(lin):
    """A and B of every stage replaced by those of the next stage in the batch's memory order (problem, stage)"""
    A, Bm, nxt = lin
    return (np.roll(A.reshape((-1,) + A.shape[2:]), -1, 0).reshape(A.shape),
            np.roll(Bm.reshape((-1,) + Bm.shape[2:]), -1, 0).reshape(Bm.shape), nxt)


def rel_dev(dx, du, rx, ru):
    """the bound's measure: largest deviation of the state and of the input step, each relative to the largest component"""
    return max(np.max(np.abs(dx - rx)) / np.max(np.abs(rx)), np.max(np.abs(du - ru)) / np.max(np.abs(ru)))


def riccati_f32(args, u_cur, effort=None, mu=None, stance=None):
    """solve_lq_clamped on float32 arrays: the stage-wise sweep (with the kernels' one projection per stage) on data
    rounded to float32.  How much of its arithmetic is float32 depends on the clamps, because solve_lq_clamped allocates
    the clamped step, the gain of a clamped stage and dx, du in float64:
      - every product and every solve of the backward sweep is float32 down to the first stage (from the end) that clamps
        an input; that stage's gain is float64, which promotes P, and every earlier stage then runs in float64 on the
        float32-rounded A, B, d and gradients;
      - the forward sweep is float64 in every case, with the gains as the backward sweep left them.
    So part b (no clamp) has a float32 backward sweep throughout, and parts c and d, where nearly every stage clamps,
    only at the last stage: their figure is mostly the effect of rounding the inputs to float32."""
    f = lambda a: np.asarray(a, np.float32)
    A, Bm, d, Q, R, QN, gx, gu, gN, dx0 = args
    dx, du, _ = solve_lq_clamped([f(a) for a in A], [f(a) for a in Bm], [f(a) for a in d], f(Q), f(R), f(QN),
                                 [f(a) for a in gx], [f(a) for a in gu], f(gN), f(dx0), [f(a) for a in u_cur],
                                 None if effort is None else f(effort), tol=np.float32(1e-4),
                                 mu=None if mu is None else np.float32(mu), stance=stance)
    return dx.astype(np.float64), du.astype(np.float64)


def stagewise(args, u_cur, effort=None, mu=None, stance=None):
    """the float64 stage-wise solution (with the kernels' projection where limits are given; without any it equals the
    dense KKT solve of solve_lq, tests/test_wb_oracle.py)"""
    dx, du, _ = solve_lq_clamped(*args, u_cur, effort, mu=mu, stance=stance)
    return dx, du


def check_inputs(lin, prob, b, ref, effort=None, mu=None, stance=None):
    """the two conditions on the inputs of problem b (reference step ref): riccati_f32 within F32_CAP of it, both
    discriminators at least DISC_MIN away from it.  Returns (f32 deviation, rolled deviation, dx0 = 0 deviation)."""
    x0, xref, uref, xi, ui, Q, R, QN = prob
    args = lq_inputs(lin, x0, xref, uref, xi, ui, Q, R, QN, b)
    sb = None if stance is None else stance[b]
    f32 = rel_dev(*riccati_f32(args, list(ui[b]), effort, mu, sb), *ref)
    roll = rel_dev(*stagewise(lq_inputs(rolled(lin), x0, xref, uref, xi, ui, Q, R, QN, b), list(ui[b]), effort, mu, sb), *ref)
    no_dx0 = rel_dev(*stagewise(args[:-1] + [np.zeros(48)], list(ui[b]), effort, mu, sb), *ref)
    assert f32 < F32_CAP, (b, f32)
    assert roll > DISC_MIN and no_dx0 > DISC_MIN, (b, roll, no_dx0)
    return f32, roll, no_dx0


# ---- the kernels -----------------------------------------------------------------------------------------------------
def engine(N, prob, limits=False, mu=None, stance=None):
    from alore_legged_manipulator_amd.whole_body import BatchedWholeBody
    x0, xref, uref, xi, ui, Q, R, QN = prob
    eng = BatchedWholeBody(B, N, DT)
    eng.set_weights(Q, R, QN)
    eng.set_torque_limits(limits)
    if mu is not None:
        eng.set_contact_constraints(True, mu)
    if stance is not None:
        eng.set_contact_schedule(stance)
    eng.set_problem(x0, xref, uref)
    eng.set_iterate(xi, ui)
    return eng


def inside_contact_constraints(u, mu, stance, tol=1e-9):
    mu = float(np.float32(mu))            # the library keeps the coefficient in float32
    f = u[..., 18:30].reshape(u.shape[:-1] + (4, 3))
    return bool(np.all(f[..., 2] >= -tol) and np.all(np.abs(f[..., 0]) <= mu * f[..., 2] + tol) and
                np.all(np.abs(f[..., 1]) <= mu * f[..., 2] + tol) and np.all(np.abs(f[~stance.astype(bool)]) <= tol))


def report(part, N, worst, f32=None, extra=""):
    f32s = "" if f32 is None else f"; riccati_f32 vs float64 {f32:.2e}"
    print(f"wb stages part {part} N={N}: worst deviation {worst:.2e}{f32s}{extra}")


@pytest.mark.parametrize("N", HORIZONS)
def test_a_linearisation_at_every_stage(model, N):
    """next at every (b, k) against oracle.step (1e-10), A and B at k in {0, 1, N // 2, N - 1} against oracle.linearize
    (2e-6 of the block scale)"""
    x0, xref, uref, xi, ui, Q, R, QN, _ = scenario(model, N, "plain")
    eng = engine(N, (x0, xref, uref, xi, ui, Q, R, QN))
    A, Bm, nxt = eng.linearize()
    worst_n = max(np.max(np.abs(nxt[b, k] - step(model, xi[b, k], ui[b, k], DT))) for b in range(B) for k in range(N))
    worst_ab = 0.0
    for k in sorted({0, 1, N // 2, N - 1} & set(range(N))):
        for b in range(B):
            Ao, Bo = linearize(model, xi[b, k], ui[b, k], DT)
            ea = np.max(np.abs(A[b, k] - Ao)) / max(1.0, np.max(np.abs(Ao)))
            eb = np.max(np.abs(Bm[b, k] - Bo)) / max(1.0, np.max(np.abs(Bo)))
            worst_ab = max(worst_ab, ea, eb)
            assert ea < 2e-6 and eb < 2e-6, (b, k, ea, eb)
    report("a", N, worst_n, extra=f" (next, absolute); A, B {worst_ab:.2e} (relative)")
    assert worst_n < 1e-10


@pytest.mark.parametrize("N", HORIZONS)
def test_b_unconstrained_sweep(model, N):
    """torque limits off: the step against the float64 dense KKT solve (solve_lq), 1e-4; the applied iterate is xi + dx"""
    x0, xref, uref, xi, ui, Q, R, QN, _ = scenario(model, N, "plain")
    prob = (x0, xref, uref, xi, ui, Q, R, QN)
    eng = engine(N, prob)
    lin = eng.linearize()
    eng.rti(1)
    assert (eng.status() == 0).all()
    dx, du = eng.last_step()
    x1, u1 = eng.get_iterate()
    worst, f32 = 0.0, 0.0
    for b in range(B):
        rx, ru = solve_lq(*lq_inputs(lin, x0, xref, uref, xi, ui, Q, R, QN, b))
        f32 = max(f32, check_inputs(lin, prob, b, (rx, ru))[0])
        worst = max(worst, rel_dev(dx[b], du[b], rx, ru))
    report("b", N, worst, f32)
    assert worst < BOUND
    assert np.allclose(x1, xi + dx, atol=1e-12)
    applied = ui + du
    applied[:, :, :18] = np.clip(applied[:, :, :18], -model.effort, model.effort)   # the applied torques stay inside the efforts
    assert np.allclose(u1, applied, atol=1e-12)


@pytest.mark.parametrize("N", HORIZONS)
def test_c_torque_limits(model, N):
    """torque limits on: the step against the float64 restatement of the sweep's projection (solve_lq_clamped with the
    efforts), 1e-4; at least one clamped input; the applied torques inside the limits"""
    x0, xref, uref, xi, ui, Q, R, QN, _ = scenario(model, N, "torque")
    prob = (x0, xref, uref, xi, ui, Q, R, QN)
    eng = engine(N, prob, limits=True)
    lin = eng.linearize()
    eng.rti(1)
    assert (eng.status() == 0).all()
    dx, du = eng.last_step()
    _, u1 = eng.get_iterate()
    worst, f32, clamps = 0.0, 0.0, 0
    for b in range(B):
        rx, ru, nc = solve_lq_clamped(*lq_inputs(lin, x0, xref, uref, xi, ui, Q, R, QN, b), list(ui[b]), model.effort)
        clamps += sum(nc)
        f32 = max(f32, check_inputs(lin, prob, b, (rx, ru), effort=model.effort)[0])
        worst = max(worst, rel_dev(dx[b], du[b], rx, ru))
    report("c", N, worst, f32, f"; {clamps} clamped inputs")
    assert clamps > 0
    assert worst < BOUND
    assert np.all(np.abs(u1[:, :, :18]) <= model.effort + 1e-9)


@pytest.mark.parametrize("N", HORIZONS)
def test_d_friction_pyramid_with_a_lifted_foot(model, N):
    """contact constraints on (mu = 0.15), problem b lifts foot b from stage ceil(N / 2): the step against
    solve_lq_clamped with the same mu and schedule, 1e-4; the applied forces inside the pyramids, none on a lifted foot"""
    x0, xref, uref, xi, ui, Q, R, QN, stance = scenario(model, N, "pyramid")
    prob = (x0, xref, uref, xi, ui, Q, R, QN)
    eng = engine(N, prob, mu=MU, stance=stance)
    lin = eng.linearize()
    eng.rti(1)
    assert (eng.status() == 0).all()
    dx, du = eng.last_step()
    _, u1 = eng.get_iterate()
    worst, f32, clamps = 0.0, 0.0, 0
    for b in range(B):
        rx, ru, nc = solve_lq_clamped(*lq_inputs(lin, x0, xref, uref, xi, ui, Q, R, QN, b), list(ui[b]), None, mu=MU,
                                      stance=stance[b])
        clamps += sum(nc)
        f32 = max(f32, check_inputs(lin, prob, b, (rx, ru), mu=MU, stance=stance)[0])
        worst = max(worst, rel_dev(dx[b], du[b], rx, ru))
    report("d", N, worst, f32, f"; {clamps} clamped force components")
    assert clamps > 0
    assert worst < BOUND
    assert inside_contact_constraints(u1, MU, stance)


@pytest.mark.parametrize("N", HORIZONS)
def test_e_contact_rows_with_a_lifted_foot(model, N):
    """hard contact rows with the schedule of part d: the step against solve_lq_contact_rows (the oracle's contact
    Jacobian), 1e-4; the linearised stance-foot speed after the step below 1e-5 m/s; no force on a lifted foot"""
    x0, xref, uref, xi, ui, Q, R, QN, stance = scenario(model, N, "plain")
    eng = engine(N, (x0, xref, uref, xi, ui, Q, R, QN), stance=stance)
    eng.set_contact_rows(True)
    lin = eng.linearize()
    eng.rti(1)
    assert (eng.status() == 0).all()
    dx, du = eng.last_step()
    _, u1 = eng.get_iterate()
    worst, rest = 0.0, 0.0
    A, Bm, nxt = lin
    for b in range(B):
        args = lq_inputs(lin, x0, xref, uref, xi, ui, Q, R, QN, b)
        J = [model.contact_jacobian(xi[b, k, :24]) for k in range(N)]
        vn = [nxt[b, k, 24:] for k in range(N)]
        rx, ru = solve_lq_contact_rows(*args, J, vn, [ui[b, k, 18:30] for k in range(N)], stance[b])
        worst = max(worst, rel_dev(dx[b], du[b], rx, ru))
        for k in range(N):
            w = J[k] @ (vn[k] + (A[b, k] @ dx[b, k] + Bm[b, k] @ du[b, k])[24:])
            rest = max(rest, np.max(np.abs(w * np.repeat(stance[b, k].astype(float), 3))))
    report("e", N, worst, extra=f"; stance-foot speed after the step {rest:.2e} m/s")
    assert worst < BOUND and rest < 1e-5
    f = u1[:, :, 18:30].reshape(B, N, 4, 3)
    assert np.all(f[~stance.astype(bool)] == 0.0)


@pytest.mark.parametrize("N", HORIZONS)
def test_f_contact_penalty_with_refinement(model, N):
    """contact penalty rho = 200 with one step of iterative refinement and the schedule of part d: the step against
    solve_lq with the oracle's penalty terms (contact_penalty) added stage by stage, 1e-4"""
    x0, xref, uref, xi, ui, Q, R, QN, stance = scenario(model, N, "plain")
    eng = engine(N, (x0, xref, uref, xi, ui, Q, R, QN), stance=stance)
    eng.set_refinement(1)
    eng.set_contact_penalty(RHO)
    lin = eng.linearize()
    eng.rti(1)
    assert (eng.status() == 0).all()
    dx, du = eng.last_step()
    worst = 0.0
    for b in range(B):
        A, Bm, d, Qd, Rd, QNd, gx, gu, gN, dx0 = lq_inputs(lin, x0, xref, uref, xi, ui, Q, R, QN, b)
        Ql, gl = [], []
        for k in range(N):
            Qa, ga = contact_penalty(model, xi[b, k], RHO, stance[b, k])
            Ql.append(Qd + Qa); gl.append(gx[k] + ga)
        rx, ru = solve_lq(A, Bm, d, Ql, Rd, QNd, gl, gu, gN, dx0)
        worst = max(worst, rel_dev(dx[b], du[b], rx, ru))
    report("f", N, worst)
    assert worst < BOUND


@pytest.mark.parametrize("case", ["torque", "pyramid"])
@pytest.mark.parametrize("N", (1, 3, 7))
def test_g_exact_working_set_mode(model, N, case):
    """exact working-set mode on the problems of parts c and d: the step against the float64 minimiser of the
    inequality-constrained LQ problem (solve_lq_inequality, its KKT residuals asserted), 1e-4; the working set settled"""
    x0, xref, uref, xi, ui, Q, R, QN, stance = scenario(model, N, case)
    effort = model.effort if case == "torque" else None
    mu = MU if case == "pyramid" else None
    st = stance if case == "pyramid" else None
    if mu is not None:   # a feasible start for the force constraints: the library projects the applied forces, so does the iterate
        f = ui[:, :, 18:30].reshape(B, N, 4, 3).copy()
        f[~st.astype(bool)] = 0.0
        f[..., 2] = np.maximum(f[..., 2], 0.0)
        m32 = float(np.float32(mu))
        f[..., 0] = np.clip(f[..., 0], -m32 * f[..., 2], m32 * f[..., 2]); f[..., 1] = np.clip(f[..., 1], -m32 * f[..., 2], m32 * f[..., 2])
        ui = ui.copy(); ui[:, :, 18:30] = f.reshape(B, N, 12)
    prob = (x0, xref, uref, xi, ui, Q, R, QN)
    eng = engine(N, prob, limits=effort is not None, mu=mu, stance=st)
    eng.set_constraint_mode(True, 1000)
    lin = eng.linearize()
    eng.rti(1)
    assert (eng.status() == 0).all()
    dx, du = eng.last_step()
    sweeps, changed, _, _ = eng.working_set_info(B)
    worst, active = 0.0, 0
    mu_lib = None if mu is None else float(np.float32(mu))
    for b in range(B):
        rx, ru, info = solve_lq_inequality(*lq_inputs(lin, x0, xref, uref, xi, ui, Q, R, QN, b), ui[b], effort, mu_lib,
                                           None if st is None else st[b])
        k = info["kkt"]
        assert k["stationarity"] < 1e-8 * max(1.0, k["scale"]) and k["feasibility"] < 1e-9 and k["dual"] < 1e-9, info
        active += info["active"]
        worst = max(worst, rel_dev(dx[b], du[b], rx, ru))
    report("g", N, worst, extra=f" ({case}; {active} active rows, {sweeps} sweeps)")
    assert active > 0                     # a constrained comparison, as at N = 20
    assert (changed == 0).all(), (sweeps, changed)
    assert worst < BOUND


@pytest.mark.parametrize("N", (1, 2, 32))
def test_h_shift_and_new_initial_state(model, N):
    """receding horizon: shift_iterate is the NumPy rule (drop stage 0, repeat the last) bit for bit; after set_x0 the
    next real-time iteration solves the LQ problem of the shifted iterate from the new initial state (solve_lq, 1e-4)"""
    x0, xref, uref, xi, ui, Q, R, QN, _ = scenario(model, N, "plain")
    eng = engine(N, (x0, xref, uref, xi, ui, Q, R, QN))
    eng.shift_iterate()
    xs, us = eng.get_iterate()
    assert np.array_equal(xs, np.concatenate([xi[:, 1:], xi[:, -1:]], 1))
    assert np.array_equal(us, np.concatenate([ui[:, 1:], ui[:, -1:]], 1))
    x0n = xi[:, 1] + 0.5 * (xi[:, 1] - xi[:, 0])     # somewhere off the shifted iterate's first stage
    eng.set_x0(x0n)
    lin = eng.linearize()
    eng.rti(1)
    assert (eng.status() == 0).all()
    dx, du = eng.last_step()
    worst = 0.0
    for b in range(B):
        rx, ru = solve_lq(*lq_inputs(lin, x0n, xref, uref, xs, us, Q, R, QN, b))
        worst = max(worst, rel_dev(dx[b], du[b], rx, ru))
    report("h", N, worst)
    assert worst < BOUND
