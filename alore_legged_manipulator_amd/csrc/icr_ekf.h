// icr_ekf.h -- the extended Kalman filter that estimates pose and ICR parameters of a robot, the arithmetic once (internal).
// Plain C++17: __host__ __device__ under hipcc, no HIP dependency otherwise.  An own restatement of the reference's `icrekf` node
// (planning_ddr_opt/icrekf/src/icrekf.cpp: get_forecast_x :99-208, get_update_x :210-222, PoseOdomSubCallback :64-72,
// ControlSubCallback :76-96, state_pub_timer_callback :272-303; include/icrekf/icrekf.h:142-181 for Q_, R_, L_, H_, M_ and the
// initial state), stated so that a step has exactly one answer.  The small functions are what the kernels of icr_ekf.hip run per
// thread; step_one() strings them together serially and is what tests/harness/icr_ekf_check.cpp and tools/icr_ekf.py run on the CPU.
// The oracle is tests/icr_ekf_cases.py (float64 Python scalars in the order written here).
//
// THE CONTRACT
//   state    x = (X, Y, psi, yr, yl, xv); P 6 x 6 row-major, stored in full (the reference never symmetrises it, neither do we);
//            the held control u = (vl, vr); q[6], r[3] standard deviations: Qd = diag(q q), Rd = diag(r r).
//   forecast over dt with the held u (get_forecast_x).  sn = sin(psi), cs = cos(psi), evaluated ONCE (libm on the host, sincos on
//            the device: the only place where the two differ).  Every product and sum below is one rounded double operation,
//            contraction off, in the order the parentheses give:
//              D = yl - yr;  dv = vr - vl;  n = vr yl - vl yr;  m = dv xv;  a = n / D;  b = m / D;  wdt = (dt dv) / D
//              ex = a cs + b sn;  ey = a sn - b cs;  gx = ((n cs + m sn) / D) / D;  gy = ((n sn - m cs) / D) / D
//              X' = X + dt ex;   Y' = Y + dt ey;   psi' = psi + wdt
//            G = J - I, J = df/dx, has rows 0-2 and columns 2-5 only (F of the reference is J transposed, :118-159):
//              G02 = dt ((-a) sn + b cs)   G03 = dt ((-vl) cs / D + gx)   G04 = dt (vr cs / D - gx)   G05 = wdt sn
//              G12 = dt ex                 G13 = dt ((-vl) sn / D + gy)   G14 = dt (vr sn / D - gy)   G15 = (-wdt) cs
//              G22 = 0                     G23 = wdt / D                  G24 = -G23                  G25 = 0
//            P' = J P J^T + dt^2 Qd (the reference's F^T P F, :205, with L_ = I), the zeros of G left out -- THIS is the order:
//              M = J P:    M[i][j] = P[i][j] + (((G[i][2] P[2][j] + G[i][3] P[3][j]) + G[i][4] P[4][j]) + G[i][5] P[5][j])   i = 0, 1
//                          M[2][j] = P[2][j] + (G23 P[3][j] + G24 P[4][j]);   M[i][j] = P[i][j]   i = 3, 4, 5
//              N = M J^T:  N[i][j] = M[i][j] + (((M[i][2] G[j][2] + M[i][3] G[j][3]) + M[i][4] G[j][4]) + M[i][5] G[j][5])   j = 0, 1
//                          N[i][2] = M[i][2] + (M[i][3] G23 + M[i][4] G24);   N[i][j] = M[i][j]   j = 3, 4, 5
//              P'[i][i] = N[i][i] + (dt (q[i] q[i])) dt;   P'[i][j] = N[i][j] elsewhere.
//   latch    u <- the new wheel message (left, right) after the forecast (ControlSubCallback :89-93).
//   update   with a pose z (PoseOdomSubCallback :64-72, get_update_x).  No trigonometry: the device gives the oracle's bits.
//              z2 = z[2];  while (z2 - psi > PI) z2 -= 2 PI;  while (z2 - psi < -PI) z2 += 2 PI      (:68-69)
//              S[i][j] = P[i][j] (+ r[i] r[i] on the diagonal), i, j < 3
//              the adjugate A of S and det S by cofactors along row 0:
//                A00 = S11 S22 - S12 S21   A01 = S02 S21 - S01 S22   A02 = S01 S12 - S02 S11
//                A10 = S12 S20 - S10 S22   A11 = S00 S22 - S02 S20   A12 = S02 S10 - S00 S12
//                A20 = S10 S21 - S11 S20   A21 = S01 S20 - S00 S21   A22 = S00 S11 - S01 S10
//                det = (S00 A00 + S01 A10) + S02 A20;   Si[i][j] = A[i][j] / det   (nine divisions, no reciprocal)
//              K[i][j] = (P[i][0] Si[0][j] + P[i][1] Si[1][j]) + P[i][2] Si[2][j]        i < 6, j < 3
//              y = (z[0] - X, z[1] - Y, z2 - psi);   x'[i] = x[i] + ((K[i][0] y0 + K[i][1] y1) + K[i][2] y2)
//              P'[i][j] = P[i][j] - ((K[i][0] P[0][j] + K[i][1] P[1][j]) + K[i][2] P[2][j])   (from the P before the update)
//   flags    once per step, after forecast and update (state_pub_timer_callback :272-303, at the rate of the control messages),
//            for k = yr, yl, xv with s = standard[k]:  pass = fabs(x[3 + k] - s) / fabs(s) < 0.01, evaluated as written (with
//            s == 0 it is never true).  As :272-281 has it: `if (!conv[k] && pass) { if (run[k]++ > 10) set } else run[k] = 0`.
//            The counter is compared BEFORE it is incremented, so the flag is set by the pass that follows a run of more than 10
//            (11) passes, i.e. by the 12th consecutive pass; conv_step[k] is the number of that step (steps are counted from 0
//            since the reset), -1 before.  Once set, a flag stays.
//   status   OK 0; MASKED 1 (mask given and 0: status 1 is written and nothing else);
//            E_DEGENERATE -1: D == 0, or something of x, P, u, the new wheel message or dt is not finite;
//            E_MEAS -4: z is not finite, or fabs(z[2] - psi') > 64 * 2 PI (this bounds the unwrap loops: the reference would spin);
//            E_SINGULAR -3: det S is not a finite number > 0;
//            E_NONFINITE -2: something of the x or P that the forecast or the update would write is not finite.
//            Tested in that order along the step (forecast: -1, -2; update: -4, -3, -2).  A step is all or nothing: when the
//            forecast or the update fails, x, P, u, the flag counters and the step count of that robot stay exactly as they were
//            and only the status is written.
// DEVIATIONS from the reference, each with a case in tests/icr_ekf_cases.py:
//   the inverse of S is adjugate over determinant in the order above (Eigen's dynamic .inverse() is a pivoted LU), and P' is
//   P - K P[0:3, :] (the reference forms (I - K H) P as dense products: the same numbers up to rounding);
//   the status, and the state left alone on failure (the reference would carry NaN on, or divide by zero);
//   the unwrap is bounded at 64 turns;
//   the flags run once per filter step, not on a timer of their own.
// LEFT OUT: the Simple_EKF_ICR first-order filter (:305-328) and the eigenvalue topics (:262-270: they publish the diagonal of P,
//   which is readable here).
#ifndef ALORE_ICR_EKF_H
#define ALORE_ICR_EKF_H

#include <cmath>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define IE_HD __host__ __device__ inline
#else
#define IE_HD inline
#endif
#if defined(__clang__)
#define IE_UNROLL _Pragma("unroll")
#else
#define IE_UNROLL
#endif

namespace icrekf {

constexpr int OK = 0, MASKED = 1, E_DEGENERATE = -1, E_NONFINITE = -2, E_SINGULAR = -3, E_MEAS = -4;
constexpr double PI = 3.14159265358979323846; // M_PI
constexpr double MAX_TURNS = 64.0;

struct Params {
    double q[6], r[3];  // standard deviations (Q_x .. Q_xv, R_x .. R_psi of the launch file)
    double standard[3]; // (yr, yl, xv) that the convergence flags compare with
};

struct Flags {        // per robot, all zero / -1 after a reset
    int run[3];       // index_*_standard_
    int conv[3];      // if_*_conver_
    int conv_step[3]; // step at which conv[k] was set, -1 before
    int steps;        // committed steps since the reset
};

IE_HD bool finite_all(const double* v, int n)
{
    bool ok = true;
    IE_UNROLL for (int i = 0; i < n; ++i) ok = ok && std::isfinite(v[i]);
    return ok;
}

IE_HD void sin_cos(double a, double& sn, double& cs)
{
#if defined(__HIP_DEVICE_COMPILE__)
    sincos(a, &sn, &cs);
#else
    sn = std::sin(a);
    cs = std::cos(a);
#endif
}

// get_forecast_x: x, P in; xo, Po out (written only on OK; they may not alias the inputs)
IE_HD int forecast(const Params& p, const double* x, const double* P, const double* u, double dt, double* xo, double* Po)
{
    const double X = x[0], Y = x[1], psi = x[2], yr = x[3], yl = x[4], xv = x[5], vl = u[0], vr = u[1];
    const double D = yl - yr;
    if (!finite_all(x, 6) || !finite_all(P, 36) || !finite_all(u, 2) || !std::isfinite(dt) || D == 0.0) return E_DEGENERATE;
    double sn, cs;
    sin_cos(psi, sn, cs);
    const double dv = vr - vl, n = vr * yl - vl * yr, m = dv * xv, a = n / D, b = m / D, wdt = (dt * dv) / D;
    const double ex = a * cs + b * sn, ey = a * sn - b * cs;
    const double gx = ((n * cs + m * sn) / D) / D, gy = ((n * sn - m * cs) / D) / D;
    double G[2][4]; // rows 0, 1 of J - I, columns 2 .. 5
    G[0][0] = dt * ((-a) * sn + b * cs); G[0][1] = dt * ((-vl) * cs / D + gx); G[0][2] = dt * (vr * cs / D - gx); G[0][3] = wdt * sn;
    G[1][0] = dt * ex;                   G[1][1] = dt * ((-vl) * sn / D + gy); G[1][2] = dt * (vr * sn / D - gy); G[1][3] = (-wdt) * cs;
    const double G23 = wdt / D, G24 = -G23;
    double M[36];
    IE_UNROLL for (int j = 0; j < 6; ++j) {
        IE_UNROLL for (int i = 0; i < 2; ++i)
            M[i * 6 + j] = P[i * 6 + j] + (((G[i][0] * P[12 + j] + G[i][1] * P[18 + j]) + G[i][2] * P[24 + j]) + G[i][3] * P[30 + j]);
        M[12 + j] = P[12 + j] + (G23 * P[18 + j] + G24 * P[24 + j]);
        IE_UNROLL for (int i = 3; i < 6; ++i) M[i * 6 + j] = P[i * 6 + j];
    }
    double N[36];
    IE_UNROLL for (int i = 0; i < 6; ++i) {
        const double* Mi = M + i * 6;
        IE_UNROLL for (int j = 0; j < 2; ++j) N[i * 6 + j] = Mi[j] + (((Mi[2] * G[j][0] + Mi[3] * G[j][1]) + Mi[4] * G[j][2]) + Mi[5] * G[j][3]);
        N[i * 6 + 2] = Mi[2] + (Mi[3] * G23 + Mi[4] * G24);
        IE_UNROLL for (int j = 3; j < 6; ++j) N[i * 6 + j] = Mi[j];
        N[i * 6 + i] = N[i * 6 + i] + (dt * (p.q[i] * p.q[i])) * dt;
    }
    const double x3[3] = {X + dt * ex, Y + dt * ey, psi + wdt};
    if (!finite_all(x3, 3) || !finite_all(N, 36)) return E_NONFINITE;
    xo[0] = x3[0]; xo[1] = x3[1]; xo[2] = x3[2]; xo[3] = yr; xo[4] = yl; xo[5] = xv;
    IE_UNROLL for (int i = 0; i < 36; ++i) Po[i] = N[i];
    return OK;
}

// PoseOdomSubCallback's unwrap + get_update_x: x, P in; xo, Po out (written only on OK; they may not alias the inputs)
IE_HD int update(const Params& p, const double* x, const double* P, const double* z, double* xo, double* Po)
{
    if (!finite_all(x, 6) || !finite_all(P, 36)) return E_DEGENERATE;
    const double psi = x[2];
    if (!finite_all(z, 3) || !(std::fabs(z[2] - psi) <= MAX_TURNS * (2 * PI))) return E_MEAS;
    double z2 = z[2];
    while (z2 - psi > PI) z2 -= 2 * PI;
    while (z2 - psi < -PI) z2 += 2 * PI;
    const double S00 = P[0] + p.r[0] * p.r[0], S01 = P[1], S02 = P[2];
    const double S10 = P[6], S11 = P[7] + p.r[1] * p.r[1], S12 = P[8];
    const double S20 = P[12], S21 = P[13], S22 = P[14] + p.r[2] * p.r[2];
    double A[3][3];
    A[0][0] = S11 * S22 - S12 * S21; A[0][1] = S02 * S21 - S01 * S22; A[0][2] = S01 * S12 - S02 * S11;
    A[1][0] = S12 * S20 - S10 * S22; A[1][1] = S00 * S22 - S02 * S20; A[1][2] = S02 * S10 - S00 * S12;
    A[2][0] = S10 * S21 - S11 * S20; A[2][1] = S01 * S20 - S00 * S21; A[2][2] = S00 * S11 - S01 * S10;
    const double det = (S00 * A[0][0] + S01 * A[1][0]) + S02 * A[2][0];
    if (!(std::isfinite(det) && det > 0.0)) return E_SINGULAR;
    double Si[3][3];
    IE_UNROLL for (int i = 0; i < 3; ++i)
        IE_UNROLL for (int j = 0; j < 3; ++j) Si[i][j] = A[i][j] / det;
    const double y[3] = {z[0] - x[0], z[1] - x[1], z2 - psi};
    double xn[6], Pn[36];
    IE_UNROLL for (int i = 0; i < 6; ++i) {
        double K[3];
        IE_UNROLL for (int j = 0; j < 3; ++j) K[j] = (P[i * 6] * Si[0][j] + P[i * 6 + 1] * Si[1][j]) + P[i * 6 + 2] * Si[2][j];
        xn[i] = x[i] + ((K[0] * y[0] + K[1] * y[1]) + K[2] * y[2]);
        IE_UNROLL for (int j = 0; j < 6; ++j) Pn[i * 6 + j] = P[i * 6 + j] - ((K[0] * P[j] + K[1] * P[6 + j]) + K[2] * P[12 + j]);
    }
    if (!finite_all(xn, 6) || !finite_all(Pn, 36)) return E_NONFINITE;
    IE_UNROLL for (int i = 0; i < 6; ++i) xo[i] = xn[i];
    IE_UNROLL for (int i = 0; i < 36; ++i) Po[i] = Pn[i];
    return OK;
}

// state_pub_timer_callback :272-303, for the step number f.steps (the caller increments it afterwards)
IE_HD void flags(const Params& p, const double* x, Flags& f)
{
    IE_UNROLL for (int k = 0; k < 3; ++k) {
        const double s = p.standard[k];
        if (!f.conv[k] && std::fabs(x[3 + k] - s) / std::fabs(s) < 0.01) {
            if (f.run[k]++ > 10) { f.conv[k] = 1; f.conv_step[k] = f.steps; }
        } else {
            f.run[k] = 0;
        }
    }
}

IE_HD void reset_flags(Flags& f)
{
    IE_UNROLL for (int k = 0; k < 3; ++k) { f.run[k] = 0; f.conv[k] = 0; f.conv_step[k] = -1; }
    f.steps = 0;
}

// One step of the filter for one robot, in place: forecast with the held u over dt, u <- wheel = (left, right), the update when
// has_z says so (z is not read otherwise), the flags.  mask: nullptr, or a pointer to this robot's flag.  Returns the status; on a
// negative status nothing was written.
IE_HD int step_one(const Params& p, double* x, double* P, double* u, Flags& f, const double* wheel, double dt, const double* z,
                   bool has_z, const unsigned char* mask)
{
    if (mask && !*mask) return MASKED;
    if (!finite_all(wheel, 2)) return E_DEGENERATE;
    double x1[6], P1[36];
    int st = forecast(p, x, P, u, dt, x1, P1);
    if (st != OK) return st;
    if (has_z) {
        double x2[6], P2[36];
        st = update(p, x1, P1, z, x2, P2);
        if (st != OK) return st;
        IE_UNROLL for (int i = 0; i < 6; ++i) x[i] = x2[i];
        IE_UNROLL for (int i = 0; i < 36; ++i) P[i] = P2[i];
    } else {
        IE_UNROLL for (int i = 0; i < 6; ++i) x[i] = x1[i];
        IE_UNROLL for (int i = 0; i < 36; ++i) P[i] = P1[i];
    }
    u[0] = wheel[0]; u[1] = wheel[1];
    flags(p, x, f);
    f.steps += 1;
    return OK;
}

} // namespace icrekf
#endif
