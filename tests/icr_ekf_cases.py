"""The sequential oracle of csrc/icr_ekf.h (the ICR EKF, one robot at a time) and the cases its tests run.

Float64 Python scalars in the header's operation order, math.sin and math.cos: on the CPU the header must give these bits (same
libm on both sides, contraction off); on the device the update must, and the forecast differs by what sincos differs from libm.
Every function follows THE CONTRACT at the top of the header line by line; read them side by side.

Also here: the simulator's Euler plant as tests/test_closed_loop.py: plant_numpy states it (scalars, the same operations), the
ControlPub message (simulator.h:342-347) and the open-loop rollouts that show what the filter is for."""
import math

import numpy as np

OK, MASKED, E_DEGENERATE, E_NONFINITE, E_SINGULAR, E_MEAS = 0, 1, -1, -2, -3, -4
PI = math.pi
MAX_TURNS = 64.0
DEFAULT = {"q": [0.5, 0.5, 1.14, 0.1, 0.1, 0.1], "r": [0.1, 0.1, 0.1], "standard": [-0.3, 0.3, 0.2]}   # planner_sim.launch:41-43, 189-198
INIT_ICR = [-0.25, 0.25, 0.1]                                                                           # (yr, yl, xv), :200-202


def finite_all(v):
    return all(math.isfinite(a) for a in v)


class Filter:
    """state of one robot: x[6], P[36] row-major, u = [vl, vr], the flag counters"""

    def __init__(self, x, P=None, u=None):
        self.x = [float(a) for a in x]
        self.P = [float(a) for a in (P if P is not None else [0.0] * 36)]
        self.u = [float(a) for a in (u if u is not None else [0.0, 0.0])]
        self.run, self.conv, self.conv_step, self.steps = [0, 0, 0], [0, 0, 0], [-1, -1, -1], 0

    def copy(self):
        f = Filter(self.x, self.P, self.u)
        f.run, f.conv, f.conv_step, f.steps = list(self.run), list(self.conv), list(self.conv_step), self.steps
        return f

    def key(self):
        return (self.x, self.P, self.u, self.run, self.conv, self.conv_step, self.steps)


def forecast(prm, x, P, u, dt):
    X, Y, psi, yr, yl, xv = x
    vl, vr = u
    D = yl - yr
    if not (finite_all(x) and finite_all(P) and finite_all(u) and math.isfinite(dt)) or D == 0.0:
        return E_DEGENERATE, None, None
    sn, cs = math.sin(psi), math.cos(psi)
    dv = vr - vl
    n = vr * yl - vl * yr
    m = dv * xv
    a = n / D
    b = m / D
    wdt = (dt * dv) / D
    ex = a * cs + b * sn
    ey = a * sn - b * cs
    gx = ((n * cs + m * sn) / D) / D
    gy = ((n * sn - m * cs) / D) / D
    G = [[dt * ((-a) * sn + b * cs), dt * ((-vl) * cs / D + gx), dt * (vr * cs / D - gx), wdt * sn],
         [dt * ex, dt * ((-vl) * sn / D + gy), dt * (vr * sn / D - gy), (-wdt) * cs]]
    G23 = wdt / D
    G24 = -G23
    M = [0.0] * 36
    for j in range(6):
        for i in range(2):
            M[i * 6 + j] = P[i * 6 + j] + (((G[i][0] * P[12 + j] + G[i][1] * P[18 + j]) + G[i][2] * P[24 + j]) + G[i][3] * P[30 + j])
        M[12 + j] = P[12 + j] + (G23 * P[18 + j] + G24 * P[24 + j])
        for i in range(3, 6):
            M[i * 6 + j] = P[i * 6 + j]
    N = [0.0] * 36
    for i in range(6):
        Mi = M[i * 6:i * 6 + 6]
        for j in range(2):
            N[i * 6 + j] = Mi[j] + (((Mi[2] * G[j][0] + Mi[3] * G[j][1]) + Mi[4] * G[j][2]) + Mi[5] * G[j][3])
        N[i * 6 + 2] = Mi[2] + (Mi[3] * G23 + Mi[4] * G24)
        for j in range(3, 6):
            N[i * 6 + j] = Mi[j]
        N[i * 6 + i] = N[i * 6 + i] + (dt * (prm["q"][i] * prm["q"][i])) * dt
    x3 = [X + dt * ex, Y + dt * ey, psi + wdt]
    if not (finite_all(x3) and finite_all(N)):
        return E_NONFINITE, None, None
    return OK, x3 + [yr, yl, xv], N


def update(prm, x, P, z):
    if not (finite_all(x) and finite_all(P)):
        return E_DEGENERATE, None, None
    psi = x[2]
    if not finite_all(z) or not (abs(z[2] - psi) <= MAX_TURNS * (2 * PI)):
        return E_MEAS, None, None
    z2 = z[2]
    while z2 - psi > PI:
        z2 -= 2 * PI
    while z2 - psi < -PI:
        z2 += 2 * PI
    r = prm["r"]
    S00, S01, S02 = P[0] + r[0] * r[0], P[1], P[2]
    S10, S11, S12 = P[6], P[7] + r[1] * r[1], P[8]
    S20, S21, S22 = P[12], P[13], P[14] + r[2] * r[2]
    A = [[S11 * S22 - S12 * S21, S02 * S21 - S01 * S22, S01 * S12 - S02 * S11],
         [S12 * S20 - S10 * S22, S00 * S22 - S02 * S20, S02 * S10 - S00 * S12],
         [S10 * S21 - S11 * S20, S01 * S20 - S00 * S21, S00 * S11 - S01 * S10]]
    det = (S00 * A[0][0] + S01 * A[1][0]) + S02 * A[2][0]
    if not (math.isfinite(det) and det > 0.0):
        return E_SINGULAR, None, None
    Si = [[A[i][j] / det for j in range(3)] for i in range(3)]
    y = [z[0] - x[0], z[1] - x[1], z2 - psi]
    xn, Pn = [0.0] * 6, [0.0] * 36
    for i in range(6):
        K = [(P[i * 6] * Si[0][j] + P[i * 6 + 1] * Si[1][j]) + P[i * 6 + 2] * Si[2][j] for j in range(3)]
        xn[i] = x[i] + ((K[0] * y[0] + K[1] * y[1]) + K[2] * y[2])
        for j in range(6):
            Pn[i * 6 + j] = P[i * 6 + j] - ((K[0] * P[j] + K[1] * P[6 + j]) + K[2] * P[12 + j])
    if not (finite_all(xn) and finite_all(Pn)):
        return E_NONFINITE, None, None
    return OK, xn, Pn


def flags(prm, f):
    for k in range(3):
        s = prm["standard"][k]
        # fabs(x - s) / fabs(s) < 0.01 as IEEE evaluates it: with s == 0 the quotient is inf or nan, never below 0.01
        passed = (abs(f.x[3 + k] - s) / abs(s) < 0.01) if s != 0.0 else False
        if not f.conv[k] and passed:
            before = f.run[k]
            f.run[k] += 1
            if before > 10:
                f.conv[k], f.conv_step[k] = 1, f.steps
        else:
            f.run[k] = 0


def step(prm, f, wheel, dt, z=None, mask=None):
    """one step in place; returns the status; a negative status (and MASKED) leaves f exactly as it was"""
    if mask is not None and not mask:
        return MASKED
    if not finite_all(wheel):
        return E_DEGENERATE
    st, x1, P1 = forecast(prm, f.x, f.P, f.u, dt)
    if st != OK:
        return st
    if z is not None:
        st, x1, P1 = update(prm, x1, P1, z)
        if st != OK:
            return st
    f.x, f.P, f.u = x1, P1, [float(wheel[0]), float(wheel[1])]
    flags(prm, f)
    f.steps += 1
    return OK


# ---- the simulator's plant (tests/test_closed_loop.py: plant_numpy, simulator.h:234-275) and its ControlPub message -------------
def plant(pose, vw, cmd, icr, max_a=2.0, max_dw=4.0, ppr=0.01, spr=0.002, substeps=5):
    """cmd = (right, left), icr = (xv, yr, yl) -> pose', vw'"""
    right, left = float(cmd[0]), float(cmd[1])
    xv, yr, yl = icr
    dv = (left + right) / 2.0 - (right - left) / (yl - yr) * (yl + yr) / 2.0
    vy = -(right - left) / (yl - yr) * xv
    dw = (right - left) / (yl - yr)
    x, y, th = pose
    v, w = vw
    for _ in range(substeps):
        if abs(v - dv) >= ppr * max_a: v += ppr * max_a * (dv - v) / abs(dv - v)
        else: v = dv
        if abs(w - dw) >= ppr * max_dw: w += ppr * max_dw * (dw - w) / abs(dw - w)
        else: w = dw
        x += v * spr * math.cos(th); y += v * spr * math.sin(th); th += w * spr
        x -= vy * spr * math.sin(th); y += vy * spr * math.cos(th)
    return [x, y, th], [v, w]


def control_pub(vw, icr):
    """(left, right) = (v - omega yl, v - omega yr), simulator.h:345-346"""
    xv, yr, yl = icr
    return [vw[0] - vw[1] * yl, vw[0] - vw[1] * yr]


# ---- the open-loop rollouts: what the filter is for -------------------------------------------------------------------------
TRUE_ICRS = [(-0.3, 0.3, 0.2), (-0.35, 0.35, 0.3), (-0.2, 0.2, 0.0)]      # (yr, yl, xv)
ROLLOUT_STEPS, ROLLOUT_DT = 3000, 0.01
_rollouts = {}


def rollout_inputs(k):
    """wheel messages [steps][2] and poses [steps][3] of the plant with true ICR k, driven open loop at v = 1, omega = sin(pi t / 2)"""
    if ("in", k) not in _rollouts:
        yr, yl, xv = TRUE_ICRS[k]
        icr = (xv, yr, yl)
        pose, vw, wheels, poses = [0.0, 0.0, 0.0], [0.0, 0.0], [], []
        for t in range(ROLLOUT_STEPS):
            v, w = 1.0, math.sin(PI * (t * ROLLOUT_DT) / 2.0)
            left = v + w * (yl + yr) / 2.0 - w * (yl - yr) / 2.0      # the command that ControlSubCallback decodes to (v, omega)
            right = left + w * (yl - yr)
            pose, vw = plant(pose, vw, (right, left), icr)
            wheels.append(control_pub(vw, icr))
            poses.append(list(pose))
        _rollouts[("in", k)] = (wheels, poses)
    return _rollouts[("in", k)]


def rollout(k, odom_every):
    """the filter from INIT_ICR along rollout k, a pose update on every odom_every-th step -> the final Filter"""
    if (k, odom_every) not in _rollouts:
        wheels, poses = rollout_inputs(k)
        f = Filter([0.0, 0.0, 0.0] + INIT_ICR)
        prm = dict(DEFAULT, standard=list(TRUE_ICRS[k]))
        for t in range(ROLLOUT_STEPS):
            z = poses[t] if (t + 1) % odom_every == 0 else None
            assert step(prm, f, wheels[t], ROLLOUT_DT, z) == OK
        _rollouts[(k, odom_every)] = f
    return _rollouts[(k, odom_every)].copy()


def icr_error_ratios(f, k):
    """|estimate - truth| over |INIT_ICR - truth| for yr, yl, xv"""
    return [abs(f.x[3 + i] - TRUE_ICRS[k][i]) / abs(INIT_ICR[i] - TRUE_ICRS[k][i]) for i in range(3)]


# ---- the cases: groups of steps on one robot --------------------------------------------------------------------------------
def _st(wheel, dt, z=None, mask=None):
    return {"wheel": [float(a) for a in wheel], "dt": float(dt), "z": None if z is None else [float(a) for a in z], "mask": mask}


def _random_state(rng):
    yr = -rng.uniform(0.1, 0.6)
    x = [rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-7, 7), yr, yr + rng.uniform(0.2, 1.0), rng.uniform(-0.3, 0.3)]
    A = rng.normal(0, 0.2, (6, 6))
    P = A @ A.T + rng.normal(0, 0.01, (6, 6))          # not symmetric
    return x, P.reshape(-1).tolist(), rng.uniform(-3, 3, 2).tolist()


def build_groups():
    rng = np.random.default_rng(20260)
    G = []

    def add(name, x, P, u, steps, prm=None):
        G.append({"name": name, "prm": prm or DEFAULT, "init": Filter(x, P, u), "steps": steps})

    for k in range(24):                                 # random states, non-symmetric P, both dt, with and without a pose
        x, P, u = _random_state(rng)
        steps = []
        for s in range(3):
            dt = (0.01, 0.1)[(k + s) % 2]
            z = None if (k + s) % 3 == 0 else [x[0] + rng.normal(0, 0.3), x[1] + rng.normal(0, 0.3), x[2] + rng.normal(0, 0.3)]
            steps.append(_st(rng.uniform(-3, 3, 2), dt, z))
        add("random%d" % k, x, P, u, steps)
    for k in range(6):                                  # update only: the held wheel speeds are zero, nothing depends on sin / cos
        x, P, _ = _random_state(rng)
        add("update_only%d" % k, x, P, [0.0, 0.0],
            [_st([0.0, 0.0], (0.01, 0.1)[k % 2], [x[0] + rng.normal(0, 0.3), x[1] + rng.normal(0, 0.3), x[2] + rng.normal(0, 0.3)]) for _ in range(2)])
    for k in range(4):                                  # P = 0 after a reset
        x, _, _ = _random_state(rng)
        add("reset%d" % k, x, None, None, [_st(rng.uniform(-3, 3, 2), 0.01, x[:3] if s % 2 else None) for s in range(4)])
    for turns in (1, -1, 2, -2, 3, -3):                 # measurements whole turns away
        x, P, _ = _random_state(rng)
        add("turns%+d" % turns, x, P, [0.0, 0.0], [_st([0.0, 0.0], 0.01, [x[0] + 0.1, x[1] - 0.1, x[2] + 0.2 + turns * 2 * PI])])
    x, P, u = _random_state(rng)
    good = _st([1.0, 1.5], 0.01, [x[0], x[1], x[2]])
    add("fail_D", x[:3] + [0.25, 0.25, 0.1], P, u, [good, _st([1.0, 1.0], 0.01)])
    add("fail_nan_state", [x[0], float("nan")] + x[2:], P, u, [good])
    add("fail_inf_P", x, [float("inf")] + P[1:], u, [good])
    add("fail_nan_wheel", x, P, u, [_st([float("nan"), 1.0], 0.01), good])
    add("fail_inf_dt", x, P, u, [_st([1.0, 1.0], float("inf")), good])
    big = list(P); big[14] = 1e308
    add("fail_nonfinite_forecast", x, big, [3.0, -3.0], [_st([1.0, 1.0], 100.0), _st([1.0, 1.0], 0.01)])
    neg = list(P); neg[0] = -1.0
    add("fail_singular_negative", x, neg, [0.0, 0.0], [_st([1.0, 1.5], 0.0, x[:3]), _st([1.0, 1.0], 0.01)])
    add("fail_singular_zero", x, None, None, [_st([1.0, 1.5], 0.0, x[:3]), _st([1.0, 1.0], 0.01)], dict(DEFAULT, r=[0.0, 0.1, 0.1]))
    add("fail_meas_nan", x, P, u, [_st([1.0, 1.5], 0.01, [x[0], float("nan"), x[2]]), good])
    add("fail_meas_far", x, P, [0.0, 0.0], [_st([0.0, 0.0], 0.01, [x[0], x[1], x[2] + 64.5 * 2 * PI]), _st([0.0, 0.0], 0.01, [x[0], x[1], x[2] + 63.5 * 2 * PI])])
    cross = list(P); cross[18] = 1e300
    add("fail_nonfinite_update", x, cross, [0.0, 0.0], [_st([1.0, 1.5], 0.01, [x[0] + 1e10, x[1], x[2]]), good])
    add("masks", x, P, u, [_st([1.0, 1.5], 0.01, x[:3], mask=0), _st([2.0, 1.0], 0.01, None, mask=1), _st([0.5, 0.5], 0.1, x[:3], mask=0),
                           _st([0.5, 0.5], 0.1, x[:3], mask=1)])
    # the flag counter: x stays where it is (wheel speeds zero, no pose): yr and yl sit on their standard, xv does not
    on = [0.0, 0.0, 0.0, -0.3, 0.3, 0.25]
    still = _st([0.0, 0.0], 0.01)
    for n in (10, 11, 12, 15):
        add("flags_run%d" % n, on, None, None, [still] * n)
    # ... a run of 8, then a pose that pulls yr away through P[3][0]: the run is broken and does not come back
    Pb = [0.0] * 36; Pb[0] = 0.01; Pb[18] = 0.05; Pb[3] = 0.05
    add("flags_broken", on, Pb, None, [still] * 8 + [_st([0.0, 0.0], 0.01, [0.1, 0.0, 0.0])] + [still] * 14)
    add("flags_standard_zero", [0.0, 0.0, 0.0, -0.3, 0.3, 0.0], None, None, [still] * 14, dict(DEFAULT, standard=[-0.3, 0.3, 0.0]))
    return G


GROUPS = build_groups()
NAMES = [g["name"] for g in GROUPS]
_expected = {}


def group(name):
    return GROUPS[NAMES.index(name)]


def expected(name):
    """[(status, Filter after the step)] for every step of the group, by the oracle"""
    if name not in _expected:
        g = group(name)
        f, out = g["init"].copy(), []
        for s in g["steps"]:
            st = step(g["prm"], f, s["wheel"], s["dt"], s["z"], s["mask"])
            out.append((st, f.copy()))
        _expected[name] = out
    return _expected[name]
