"""Whole-body class, CPU: the float64 oracle (oracle/wb_oracle.py, 6-D spatial algebra) pinned by the physics
identities of SURVEY.md 8(c) -- there is no reference implementation of this class (PARITY UNPINNED): gravity torques
= gradient of the potential energy; CRBA = RNEA columns, symmetric positive definite, total mass on the base block;
ABA o RNEA = identity; forward dynamics by M^-1 = ABA; energy and momentum conservation of passive rollouts."""
import numpy as np
import pytest

from oracle.wb_oracle import Model, linearize, rpy_matrix, solve_lq, step


@pytest.fixture(scope="module")
def model():
    return Model()


def sample(model, rng, vel=0.5):
    q = np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-0.6, 0.6, 3), rng.uniform(model.lower, model.upper)])
    v = rng.normal(0, vel, model.nv)
    return q, v


def test_model_table(model):
    assert model.nb == 19 and model.nv == 24
    assert abs(model.total_mass - 75.6865) < 1e-3          # sum of all URDF link masses
    assert model.parent[1] == 0 and model.parent[13] == 0 and model.parent[18] == 17
    assert np.all(model.lower < model.upper)
    for I in model.I:                                        # physical spatial inertias
        assert np.all(np.linalg.eigvalsh(I) > 0)


def test_gravity_terms_equal_the_potential_gradient(model):
    rng = np.random.default_rng(1)
    for _ in range(5):
        q, _ = sample(model, rng)
        g = model.rnea(q, np.zeros(24), np.zeros(24))
        h = 1e-6
        for j in range(18):
            e = np.zeros(24); e[6 + j] = h
            dU = (model.potential(q + e) - model.potential(q - e)) / (2 * h)
            assert abs(g[6 + j] - dU) < 1e-6 * max(1.0, abs(dU))
        R = rpy_matrix(q[3:6])
        assert np.allclose(g[3:6], R.T @ [0, 0, model.total_mass * model.g], atol=1e-9)


def test_crba_equals_rnea_columns_and_is_spd(model):
    rng = np.random.default_rng(2)
    for _ in range(5):
        q, _ = sample(model, rng)
        M = model.crba(q)
        assert np.max(np.abs(M - M.T)) < 1e-12
        assert np.linalg.eigvalsh(M).min() > 1e-5
        assert np.allclose(M[3:6, 3:6], model.total_mass * np.eye(3), atol=1e-10)
        for j in range(24):
            e = np.zeros(24); e[j] = 1.0
            col = model.rnea(q, np.zeros(24), e, gravity=False)
            assert np.max(np.abs(col - M[:, j])) < 1e-11


def test_aba_inverts_rnea_and_matches_the_mass_matrix_solve(model):
    rng = np.random.default_rng(3)
    for _ in range(8):
        q, v = sample(model, rng)
        a = rng.normal(0, 1.0, 24)
        f = rng.normal(0, 30.0, (4, 3))
        tau_full = model.rnea(q, v, a, f)
        # ABA takes joint torques only: the base rows of RNEA must vanish for a consistent (a, f) -- choose the base
        # acceleration that makes them vanish instead: solve with forward dynamics, then invert
        tau = rng.normal(0, 5.0, 18)
        a1 = model.aba(q, v, tau, f)
        a2 = model.forward_dynamics(q, v, tau, f)
        assert np.max(np.abs(a1 - a2)) < 1e-9 * max(1.0, np.max(np.abs(a1)))
        back = model.rnea(q, v, a1, f)
        assert np.max(np.abs(back[:6])) < 1e-9 and np.max(np.abs(back[6:] - tau)) < 1e-9
        assert np.all(np.isfinite(tau_full))


def rk4(model, q, v, dt, gravity):
    def f(q, v):
        return model.qdot(q, v), model.aba(q, v, np.zeros(18), None, gravity=gravity)
    k1 = f(q, v); k2 = f(q + dt / 2 * k1[0], v + dt / 2 * k1[1]); k3 = f(q + dt / 2 * k2[0], v + dt / 2 * k2[1])
    k4 = f(q + dt * k3[0], v + dt * k3[1])
    return q + dt / 6 * (k1[0] + 2 * k2[0] + 2 * k3[0] + k4[0]), v + dt / 6 * (k1[1] + 2 * k2[1] + 2 * k3[1] + k4[1])


def test_passive_rollout_conserves_energy_and_momentum(model):
    rng = np.random.default_rng(4)
    q, v = sample(model, rng, vel=1.0)
    E0 = model.kinetic(q, v) + model.potential(q)
    qq, vv = q.copy(), v.copy()
    for _ in range(100):                                   # 0.1 s of free fall, torques off
        qq, vv = rk4(model, qq, vv, 1e-3, True)
    E1 = model.kinetic(qq, vv) + model.potential(qq)
    assert abs(E1 - E0) < 1e-7 * abs(E0), (E0, E1)
    h0 = model.world_momentum(q, v)
    qq, vv = q.copy(), v.copy()
    for _ in range(100):                                   # no gravity: spatial momentum is constant
        qq, vv = rk4(model, qq, vv, 1e-3, False)
    h1 = model.world_momentum(qq, vv)
    assert np.max(np.abs(h1 - h0)) < 1e-7 * np.max(np.abs(h0))


def test_static_stance_is_an_equilibrium(model):
    """Standing pose, feet forces = weight / 4 + the torques RNEA asks for: zero acceleration."""
    q = np.zeros(24); q[2] = 0.55
    q[6:18] = np.tile([0.0, 0.8, -1.6], 4)
    q[18:] = [0.0, 1.0, -1.2, 0.2, 0.0, 0.0]
    f = np.tile([0, 0, model.total_mass * model.g / 4], (4, 1))
    need = model.rnea(q, np.zeros(24), np.zeros(24), f)
    # the base rows are the residual wrench the feet cannot balance with equal forces (the centre of mass is not over
    # the centre of the feet): small next to the weight
    assert np.linalg.norm(need[3:6]) < 1e-9 and np.linalg.norm(need[:3]) < 0.2 * model.total_mass * model.g
    a = model.aba(q, np.zeros(24), need[6:], f)
    assert np.max(np.abs(a[6:])) < 50.0 and np.all(np.isfinite(a))


def test_lq_solver_satisfies_its_kkt_conditions(model):
    rng = np.random.default_rng(5)
    N, nx, nu = 4, 6, 3
    A = [np.eye(nx) + 0.1 * rng.normal(size=(nx, nx)) for _ in range(N)]
    B = [rng.normal(size=(nx, nu)) for _ in range(N)]
    d = [0.1 * rng.normal(size=nx) for _ in range(N)]
    Q, R = np.diag(rng.uniform(1, 2, nx)), np.diag(rng.uniform(0.1, 1, nu))
    gx = [rng.normal(size=nx) for _ in range(N)]; gu = [rng.normal(size=nu) for _ in range(N)]; gN = rng.normal(size=nx)
    dx0 = rng.normal(size=nx)
    dx, du = solve_lq(A, B, d, Q, R, Q, gx, gu, gN, dx0)
    assert np.allclose(dx[0], dx0)
    for k in range(N):
        assert np.allclose(dx[k + 1], A[k] @ dx[k] + B[k] @ du[k] + d[k], atol=1e-10)
    # stationarity by the costate recursion
    lam = Q @ dx[N] + gN
    for k in range(N - 1, -1, -1):
        assert np.allclose(R @ du[k] + gu[k] + B[k].T @ lam, 0, atol=1e-9)
        lam = Q @ dx[k] + gx[k] + A[k].T @ lam


def test_discrete_step_and_its_linearisation(model):
    rng = np.random.default_rng(6)
    q, v = sample(model, rng, vel=0.3)
    x = np.concatenate([q, v]); u = np.concatenate([rng.normal(0, 3, 18), rng.normal(0, 50, 12)])
    A, B = linearize(model, x, u, 0.01)
    dxs = 1e-5 * rng.normal(size=48); dus = 1e-3 * rng.normal(size=30)
    lin = step(model, x, u, 0.01) + A @ dxs + B @ dus
    assert np.max(np.abs(step(model, x + dxs, u + dus, 0.01) - lin)) < 1e-7   # second-order remainder
    assert np.allclose(A[:3, :3], np.eye(3)) and np.max(np.abs(A[24:, :3])) < 1e-9   # nothing depends on the position


def test_committed_stance_equilibrium_fixture(model):
    import json, os
    from tests.wb_cases import equilibrium_inputs, make_problems_fast, stand_q
    u = np.array(json.load(open(os.path.join(os.path.dirname(__file__), "golden", "wb_stand_equilibrium.json")))["u_eq"])
    assert np.allclose(u, equilibrium_inputs(model, stand_q()), atol=1e-9)
    a = model.aba(stand_q(), np.zeros(24), u[:18], u[18:].reshape(4, 3))
    assert np.max(np.abs(a)) < 1e-8                       # at rest it stays at rest
    x0, xref, uref, xi, ui = make_problems_fast(5, 4, seed=1)
    assert x0.shape == (5, 48) and xi.shape == (5, 5, 48) and np.allclose(uref[0, 0], u)


def test_clamped_riccati_equals_the_kkt_solve_without_clamps_and_respects_limits(model):
    from oracle.wb_oracle import solve_lq_clamped
    rng = np.random.default_rng(7)
    N, nx, nu = 5, 48, 30
    A = [np.eye(nx) + 0.02 * rng.normal(size=(nx, nx)) for _ in range(N)]
    B = [0.3 * rng.normal(size=(nx, nu)) for _ in range(N)]
    d = [0.01 * rng.normal(size=nx) for _ in range(N)]
    Q, R = np.diag(rng.uniform(1, 3, nx)), np.diag(rng.uniform(0.05, 0.2, nu))
    gx = [0.1 * rng.normal(size=nx) for _ in range(N)]; gu = [0.1 * rng.normal(size=nu) for _ in range(N)]; gN = 0.1 * rng.normal(size=nx)
    dx0 = 0.05 * rng.normal(size=nx)
    u_cur = [np.zeros(nu) for _ in range(N)]
    dx, du = solve_lq(A, B, d, Q, R, Q, gx, gu, gN, dx0)
    big = np.full(18, 1e6)
    dx2, du2, nc = solve_lq_clamped(A, B, d, Q, R, Q, gx, gu, gN, dx0, u_cur, big)
    assert sum(nc) == 0 and np.max(np.abs(dx2 - dx)) < 1e-9 and np.max(np.abs(du2 - du)) < 1e-9
    lim = np.full(18, 0.5 * np.max(np.abs(du[:, :18])))                       # limits that bite
    dx3, du3, nc3 = solve_lq_clamped(A, B, d, Q, R, Q, gx, gu, gN, np.zeros(nx), u_cur, lim)
    assert sum(nc3) > 0
    # with dx0 = 0 the feed-forward steps are the steps of stage 0: inside the limits there
    assert np.all(np.abs(du3[0, :18]) <= lim + 1e-9)


def test_contact_constrained_sweep_restatement():
    """solve_lq_clamped with the contact constraints on a small random LQ problem: without any active bound it is the
    plain LQ solution; with a slippery floor and a swing foot the feed-forward forces of every stage satisfy the bounds
    it states (contact_bounds), and the applied inputs are inside the pyramid."""
    from oracle.wb_oracle import apply_contact_constraints, contact_bounds, solve_lq, solve_lq_clamped
    rng = np.random.default_rng(3)
    N, nx, nu = 6, 8, 30
    A = [np.eye(nx) + 0.05 * rng.normal(size=(nx, nx)) for _ in range(N)]
    Bm = [0.1 * rng.normal(size=(nx, nu)) for _ in range(N)]
    d = [0.01 * rng.normal(size=nx) for _ in range(N)]
    Q, R, QN = np.eye(nx), 0.1 * np.eye(nu), 2 * np.eye(nx)
    gx = [rng.normal(size=nx) for _ in range(N)]; gu = [0.01 * rng.normal(size=nu) for _ in range(N)]
    gN = rng.normal(size=nx); dx0 = 0.1 * rng.normal(size=nx)
    u = [np.concatenate([np.zeros(18), np.tile([0.0, 0.0, 100.0], 4)]) for _ in range(N)]
    dx, du = solve_lq(A, Bm, d, Q, R, QN, gx, gu, gN, dx0)
    cx, cu, nc = solve_lq_clamped(A, Bm, d, Q, R, QN, gx, gu, gN, dx0, u, None, mu=0.9)
    assert sum(nc) == 0 and np.allclose(cx, dx, atol=1e-9) and np.allclose(cu, du, atol=1e-9)
    gu2 = [g.copy() for g in gu]
    for g in gu2:
        g[18] = 30.0; g[21 + 1] = -40.0                     # pushes fx of foot 0 and fy of foot 1 far out
    stance = np.ones((N, 4), int); stance[3:, 2] = 0
    cx, cu, nc = solve_lq_clamped(A, Bm, d, Q, R, QN, gx, gu2, gN, dx0, u, None, mu=0.3, stance=stance)
    assert sum(nc) > 0
    for k in range(N):
        unew = apply_contact_constraints(u[k] + cu[k], 0.3, stance[k])
        f = unew[18:].reshape(4, 3)
        assert np.all(f[:, 2] >= 0) and np.all(np.abs(f[:, :2]) <= 0.3 * f[:, 2:3] + 1e-12)
        if k >= 3:
            assert np.all(f[2] == 0)


def test_contact_jacobian_is_the_velocity_of_the_foot_points(model):
    """J_c from the force route (minus the generalized force of unit foot forces) maps a generalized velocity to the
    world-frame velocity of the four foot points: compared with central differences of foot_positions along qdot(q, v);
    and the penalty terms are its Gauss-Newton Hessian / gradient (swing feet masked out)."""
    from oracle.wb_oracle import contact_penalty
    rng = np.random.default_rng(4)
    q = np.zeros(24); q[2] = 0.45
    q[3:6] = rng.uniform(-0.3, 0.3, 3)
    q[6:] = rng.uniform(-0.5, 0.5, 18)
    v = rng.uniform(-1.0, 1.0, 24)
    J = model.contact_jacobian(q)
    h = 1e-6
    qd = model.qdot(q, v)
    fd = (model.foot_positions(q + h * qd) - model.foot_positions(q - h * qd)).reshape(-1) / (2 * h)
    assert np.max(np.abs(J @ v - fd)) < 1e-6 * max(1.0, np.max(np.abs(fd)))
    x = np.concatenate([q, v])
    Qa, ga = contact_penalty(model, x, 50.0, stance_k=(1, 0, 1, 1))
    Jm = J.copy(); Jm[3:6] = 0.0
    assert np.allclose(Qa[24:, 24:], 50.0 * Jm.T @ Jm) and np.allclose(ga[24:], 50.0 * Jm.T @ (Jm @ v))
    assert not Qa[:24].any() and not Qa[:, :24].any() and not ga[:24].any()


def test_contact_rows_restatement_is_the_limit_of_the_penalty_and_holds_the_rows():
    """solve_lq_contact_rows (hard rows J (v_next + [A dx + B du]_v) = 0, solved with the forces free of cost) on a random LQ
    problem of the whole-body shape (nx 48, nu 30): the rows and the dynamics hold to rounding, a swing foot's force step is
    -f, and the solution is the limit rho -> infinity of the same problem with the penalty 1/2 rho |row|^2 and no force cost."""
    from oracle.wb_oracle import solve_lq_contact_rows
    rng = np.random.default_rng(9)
    N, nx, nu, nv = 3, 48, 30, 24
    A = [np.eye(nx) + 0.05 * rng.normal(size=(nx, nx)) for _ in range(N)]
    B = [0.1 * rng.normal(size=(nx, nu)) for _ in range(N)]
    d = [0.01 * rng.normal(size=nx) for _ in range(N)]
    Q, R, QN = np.diag(rng.uniform(1, 2, nx)), np.diag(rng.uniform(0.1, 1, nu)), np.diag(rng.uniform(1, 2, nx))
    gx = [rng.normal(size=nx) for _ in range(N)]; gu = [rng.normal(size=nu) for _ in range(N)]; gN = rng.normal(size=nx)
    dx0 = 0.1 * rng.normal(size=nx)
    J = [rng.normal(size=(12, nv)) for _ in range(N)]
    vn = [0.1 * rng.normal(size=nv) for _ in range(N)]
    uf = [rng.normal(size=12) for _ in range(N)]
    stance = np.ones((N, 4), int); stance[1:, 2] = 0
    dx, du = solve_lq_contact_rows(A, B, d, Q, R, QN, gx, gu, gN, dx0, J, vn, uf, stance)
    assert np.allclose(dx[0], dx0)
    for k in range(N):
        assert np.allclose(dx[k + 1], A[k] @ dx[k] + B[k] @ du[k] + d[k], atol=1e-9)
        row = J[k] @ (vn[k] + (A[k] @ dx[k] + B[k] @ du[k])[nv:])
        for i in range(4):
            if stance[k, i]:
                assert np.max(np.abs(row[3 * i:3 * i + 3])) < 1e-9
            else:
                assert np.allclose(du[k][18 + 3 * i:21 + 3 * i], -uf[k][3 * i:3 * i + 3], atol=1e-10)
    # the penalty limit: a dense KKT solve with rho (row)^2 in the cost, forces free of cost, swing forces fixed by a stiff term
    def penalised(rho):
        nz = (N + 1) * nx + N * nu
        ox = lambda k: k * (nx + nu); ou = lambda k: k * (nx + nu) + nx
        H = np.zeros((nz, nz)); g = np.zeros(nz)
        Rt = R.copy(); Rt[18:, 18:] = 0.0
        for k in range(N):
            H[ox(k):ox(k) + nx, ox(k):ox(k) + nx] += Q; H[ou(k):ou(k) + nu, ou(k):ou(k) + nu] += Rt
            g[ox(k):ox(k) + nx] += gx[k]; gk = gu[k].copy(); gk[18:] = 0.0; g[ou(k):ou(k) + nu] += gk
            T = np.zeros((12, nz)); t0 = np.zeros(12)
            for i in range(4):
                rs = slice(3 * i, 3 * i + 3)
                if stance[k, i]:
                    T[rs, ox(k):ox(k) + nx] = J[k][rs] @ A[k][nv:]; T[rs, ou(k):ou(k) + nu] = J[k][rs] @ B[k][nv:]; t0[rs] = J[k][rs] @ vn[k]
                else:
                    T[rs, ou(k) + 18 + 3 * i:ou(k) + 21 + 3 * i] = np.eye(3); t0[rs] = uf[k][rs]
            H += rho * T.T @ T; g += rho * T.T @ t0
        H[ox(N):ox(N) + nx, ox(N):ox(N) + nx] += QN; g[ox(N):ox(N) + nx] += gN
        ne = (N + 1) * nx
        C = np.zeros((ne, nz)); c = np.zeros(ne)
        C[:nx, :nx] = np.eye(nx); c[:nx] = dx0
        for k in range(N):
            r = (k + 1) * nx
            C[r:r + nx, ox(k):ox(k) + nx] = -A[k]; C[r:r + nx, ou(k):ou(k) + nu] = -B[k]; C[r:r + nx, ox(k + 1):ox(k + 1) + nx] = np.eye(nx); c[r:r + nx] = d[k]
        z = np.linalg.solve(np.block([[H, C.T], [C, np.zeros((ne, ne))]]), np.concatenate([-g, c]))[:nz]
        return np.array([z[ox(k):ox(k) + nx] for k in range(N + 1)]), np.array([z[ou(k):ou(k) + nu] for k in range(N)])
    e = []
    for rho in (1e4, 1e6):
        px, pu = penalised(rho)
        e.append(max(np.max(np.abs(px - dx)), np.max(np.abs(pu - du))))
    assert e[1] < 0.02 * e[0] and e[1] < 1e-3 * max(np.max(np.abs(dx)), np.max(np.abs(du)))


@pytest.mark.parametrize("N", (1, 2, 3, 5))
def test_stage_varying_problems_suit_float32_and_tell_stage_bugs_apart(model, N):
    """The inputs of tests/test_wb_stages_gpu.py (tests/wb_cases.py: make_varied_problems, its seed and amplitude) with
    the oracle's own linearisation, on the problems of its parts b (unconstrained), c (torque limits) and d (friction
    pyramid with a lifted foot): the float32 restatement of the sweep stays within half the 1e-4 bound of the float64
    solve, and the solve with A, B rolled by one stage or with dx0 = 0 is at least 1e-2 away from it."""
    from tests import test_wb_stages_gpu as S
    from oracle.wb_oracle import solve_lq_clamped
    x0, xref, uref, xi, ui, Q, R, QN, stance = S.scenario(model, N, "plain")
    lin = S.oracle_lin(model, xi, ui)                      # the same iterate in every part
    for kind in ("plain", "torque", "pyramid"):
        x0, xref, uref, xi, ui, Q, R, QN, stance = S.scenario(model, N, kind)
        prob = (x0, xref, uref, xi, ui, Q, R, QN)
        effort = model.effort if kind == "torque" else None
        mu, st = (S.MU, stance) if kind == "pyramid" else (None, None)
        clamps, worst = 0, [0.0, np.inf, np.inf]
        for b in range(S.B):
            args = S.lq_inputs(lin, *prob, b)
            if kind == "plain":
                ref = solve_lq(*args)
            else:
                rx, ru, nc = solve_lq_clamped(*args, list(ui[b]), effort, mu=mu, stance=None if st is None else st[b])
                ref, clamps = (rx, ru), clamps + sum(nc)
            f32, roll, no_dx0 = S.check_inputs(lin, prob, b, ref, effort, mu, st)
            worst = [max(worst[0], f32), min(worst[1], roll), min(worst[2], no_dx0)]
        print(f"N={N} {kind}: riccati_f32 vs float64 {worst[0]:.2e}; discriminators: A, B rolled {worst[1]:.2e}, dx0 = 0 {worst[2]:.2e}; clamps {clamps}")
        assert kind == "plain" or clamps > 0


def test_inequality_constrained_lq_solver_satisfies_its_kkt_conditions():
    """oracle/wb_oracle.py: solve_lq_inequality (the checker of the kernels' exact working-set mode) on a random LQ problem with
    torque boxes, a friction pyramid per stance foot and a foot in the air: stationarity, feasibility and the signs of the
    multipliers to rounding; with nothing active it is solve_lq."""
    from oracle.wb_oracle import solve_lq, solve_lq_inequality
    rng = np.random.default_rng(0)
    N, nx, nu = 4, 48, 30
    A = [np.eye(nx) + 0.05 * rng.standard_normal((nx, nx)) for _ in range(N)]
    B = [0.3 * rng.standard_normal((nx, nu)) for _ in range(N)]
    d = [0.1 * rng.standard_normal(nx) for _ in range(N)]
    Q = np.diag(rng.uniform(1, 5, nx)); R = np.diag(rng.uniform(0.1, 1, nu)); QN = 3 * Q
    gx = [rng.standard_normal(nx) for _ in range(N)]; gu = [rng.standard_normal(nu) for _ in range(N)]; gN = rng.standard_normal(nx)
    dx0 = rng.standard_normal(nx)
    u = np.zeros((N, nu)); u[:, 18:30].reshape(N, 4, 3)[:, :, 2] = 5.0
    stance = np.ones((N, 4), int); stance[2:, 1] = 0
    dx, du, info = solve_lq_inequality(A, B, d, Q, R, QN, gx, gu, gN, dx0, u, np.full(18, 0.5), 0.5, stance)
    k = info["kkt"]
    assert info["active_inequalities"] > 10
    assert k["stationarity"] < 1e-10 * k["scale"] and k["feasibility"] < 1e-12 and k["dual"] < 1e-12
    un = u + du
    f = un[:, 18:30].reshape(N, 4, 3)
    assert np.all(np.abs(un[:, :18]) <= 0.5 + 1e-12) and np.all(np.abs(f[..., :2]) <= 0.5 * f[..., 2:3] + 1e-12) and np.all(np.abs(f[~stance.astype(bool)]) < 1e-12)
    for k_ in range(N):   # the dynamics rows hold
        assert np.max(np.abs(dx[k_ + 1] - (A[k_] @ dx[k_] + B[k_] @ du[k_] + d[k_]))) < 1e-10
    dx2, du2, info2 = solve_lq_inequality(A, B, d, Q, R, QN, gx, gu, gN, dx0, u, np.full(18, 1e9))
    dx3, du3 = solve_lq(A, B, d, Q, R, QN, gx, gu, gN, dx0)
    assert info2["active"] == 0 and np.max(np.abs(du2 - du3)) < 1e-10 and np.max(np.abs(dx2 - dx3)) < 1e-10
