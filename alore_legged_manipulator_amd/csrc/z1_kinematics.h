// z1_kinematics.h -- the Z1 arm's grasp kinematics and the FSM's grasp step for one robot, the arithmetic once (internal).
// Plain C++17, float64: __host__ __device__ under hipcc, no HIP dependency otherwise.  Restates the reference's only use of
// Pinocchio (Simulation/isaac_b2_controller/b2z1/b2z1_object_fsm.py: the setup :136-151, object_grasp :643-749, to_se3 and
// get_grasp_pose :848-873; Deployment/object_arrangement_fsm.py:142, 740-755 is the same code).  The functions are what one lane
// of the kernels of arm_ik.hip computes for its problem; tests/harness/arm_ik_check.cpp runs them one by one on the CPU, and
// tests/arm_ik_cases.py is their oracle.
//
// THE CHAIN, in the arm's base frame link00.  Six revolute joints with translation-only origins: joint1 at joint1_xyz =
// (0, 0, 0.0585) in link00, joint2..6 at b2z1::ORIGIN of bodies 14..18, axes z y y y z x (b2z1::AXIS of bodies 13..18); the tool
// frame gripperStator rigidly at tool_xyz = (0.051, 0, 0) in link06 (z1_original.urdf:56-66, 224-229, 262-266).  A joint vector
// has 7 entries as in the FSM; entry 6 is jointGripper, which does not move the tool frame: it passes through the IK untouched.
//
//   fk         the tool placement (R row-major, p)
//   jac_local  the 6 x 6 frame Jacobian in the LOCAL frame, linear rows first (pin.computeFrameJacobian(..., LOCAL)); the
//              seventh column of Pinocchio's 6 x 7 matrix is zero and is left out: J J^T and v[0:6] are the same without it
//   log6       (v, w) of a placement.  theta = atan2(|s|, c) with s = (R32 - R23, R13 - R31, R21 - R12) / 2 and c = (tr R - 1) / 2,
//              w = (theta / |s|) s, v = alpha p - w x p / 2 + beta (w . p) w with alpha = (theta / 2) cot(theta / 2) and
//              beta = (1 - alpha) / theta^2
//   jlog6      Pinocchio's Jlog6: [[A, C A], [0, A]], A = beta w w^T + alpha I + [w]x / 2,
//              C = u w^T + beta w p^T + beta (w . p) I + [p]x / 2, u = b (w . p) w - (theta^2 b + 2 beta) p, b = beta' / theta
//   SMALL ANGLES.  Below theta = 1e-2 (SMALL_ANGLE) the closed forms give way to their series: theta / sin theta =
//              1 + t2 / 6 + 7 t2^2 / 360 + 31 t2^3 / 15120; alpha = 1 - t2 / 12 - t2^2 / 720 - t2^3 / 30240; beta = 1 / 12 +
//              t2 / 720 + t2^2 / 30240; b = 1 / 360 + t2 / 7560 (t2 = theta^2).  At the switch the series are exact to below 1e-16; the
//              closed forms lose digits there by cancellation (beta to 1e-12, b to 2e-8, alpha none), which is why it is not lower.
//   ROTATION ANGLES ABOVE 3.0 rad are outside the tested contract: |s| goes to 0 near a half turn and theta / |s| loses its
//              digits; the reference (Pinocchio) has a branch of its own there, this header has none.
//   ik_solve   the loop of :710-726.  err = log6(oMf^-1 oMdes); stop when |err| < eps (status 0); Je = -Jlog6(iMd^-1) J;
//              v = -Je^T (Je Je^T + damp I)^-1 err by LDL^T without pivoting in a fixed order (column by column, sums in index
//              order); q[0:6] += v dt.  err_norm is the last norm that was EVALUATED: as in the reference it is not evaluated
//              again after the last step.  status: 0 below eps, 1 iteration limit, 2 a pivot that is not positive and finite (q
//              as it stood, the iteration count of the completed steps), -1 an input that is not finite (q = q_init, err_norm
//              NaN, 0 iterations).  |err| is sqrt of the six squares summed in index order.
//   NO JOINT LIMITS: the reference's IK has none, nor has this one; q leaves b2z1::Q_LOWER / Q_UPPER where the target asks for it.
//   grasp_pose get_grasp_pose: (x - dx cos yaw, y - dx sin yaw, z + dz) and Rz(yaw) Ry(pitch) as the quaternion x, y, z, w =
//              (-sy sp, cy sp, sy cp, cy cp) of the half angles (tf's quaternion_from_euler(0, pitch, yaw, 'sxyz')); pitch in degrees
//   base_target :672-696: T_base^-1 T_target, quaternions read x, y, z, w and NORMALISED as scipy's from_quat does (to_se3), then in
//              the base frame: box z -= k / 2.2; table x += k / 1.5, z -= 0.01; every other class x += k, z += 0.03
//   grasp_step one call of object_grasp on one robot's state, in the reference's order (the numbered lines in the function).
//
// THE QUIRKS of object_grasp, kept:
//   d_gripper      is 0 before the first grasp and stays 0.01 after the first finished one (:739): every later grasp closes the
//                  gripper and moves k from its first tick after the wait, whatever err_norm says;
//   early returns  the return of :664 (grasp_time < 100) writes neither robot_vel_cmd nor joint_cmd, the `done` return of :746
//                  does not write joint_cmd: both keep what an earlier tick left;
//   err_norm       counts stability BEFORE this tick's IK: it is the norm of the previous tick (1000 after a reset);
//   grasp_time     runs from the first call, the approach included: a robot that needs more than 100 ticks to get into the band
//                  does not wait, one that needs more than 700 closes its gripper at once;
//   default pose   for the table class the arm joints of the command become arm_default_pose from gripper_ang >= -0.4 on, the
//                  IK still runs and err_norm is that of its target.
// DEVIATIONS: the state also carries what the last tick's IK reported (ik_iterations, ik_status; IK_NOT_RUN on a tick without
//   one); joint_cmd starts as joint_default, robot_vel_cmd as 0; inputs that are not finite give IK status -1, q = the measured
//   joints and err_norm NaN (NaN < 0.1 is false: the stability count restarts), where the reference would raise.
//
// CONTRACTION is off (the pragma below; g++ does not contract in ISO mode and the harness is built with -ffp-contract=off).
#ifndef ALORE_Z1_KINEMATICS_H
#define ALORE_Z1_KINEMATICS_H

#include <cmath>

#include "b2z1_model.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define Z1_HD __host__ __device__ inline
#else
#define Z1_HD inline
#endif

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

namespace z1 {

constexpr int NQ = 7, NA = 6;
constexpr double SMALL_ANGLE = 1e-2;
constexpr int CATEGORY_OTHER = 0, CATEGORY_TABLE = 1, CATEGORY_BOX = 2; // ALORE_ARM_CATEGORY_*
constexpr int IK_OK = 0, IK_LIMIT = 1, IK_PIVOT = 2, IK_NOT_RUN = 3, IK_NOT_FINITE = -1;
// the constants of object_grasp (:652-739)
constexpr double REACH_BAND = 0.02, APPROACH_SPEED = 0.15, ERR_STABLE = 0.1, D_GRIPPER = 0.01, K_MAX = 0.25;
constexpr double GRIPPER_OPEN = -1.5, GRIPPER_CLOSED = -0.1, GRIPPER_TABLE = -0.4, ERR_RESET = 1000.0;
constexpr int WAIT_TICKS = 100, STABLE_TICKS = 20, TIMEOUT_TICKS = 700;

// alore_arm_params, field for field
struct Params {
    double eps, damp, dt;
    int max_iter, reserved;
    double joint1_xyz[3], tool_xyz[3], joint_default[7];
};
inline void default_params(Params* p)
{
    p->eps = 1e-3;  // :705-708
    p->damp = 1e-12;
    p->dt = 3e-3;
    p->max_iter = 200;
    p->reserved = 0;
    p->joint1_xyz[0] = 0.0; p->joint1_xyz[1] = 0.0; p->joint1_xyz[2] = 0.0585;
    p->tool_xyz[0] = 0.051; p->tool_xyz[1] = 0.0; p->tool_xyz[2] = 0.0;
    const double jd[7] = {0.0, 1.48, -0.63, -0.84, 0.0, 1.57, 0.0}; // :148
    for (int i = 0; i < 7; ++i) p->joint_default[i] = jd[i];
}
// alore_arm_class, field for field
struct Class {
    int category, reserved;
    double grasp_cfg[3], plan_cfg[3], arm_default_pose[7];
};

Z1_HD bool finite(double v) { return v - v == 0.0; }
Z1_HD bool finite_n(const double* v, int n)
{
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = ok && finite(v[i]);
    return ok;
}

// R <- R Rot(AX, a), R row-major
template <int AX> Z1_HD void rotate(double* R, double a)
{
    constexpr int i = (AX + 1) % 3, j = (AX + 2) % 3;
    const double s = std::sin(a), c = std::cos(a);
    for (int r = 0; r < 3; ++r) {
        const double u = R[3 * r + i], v = R[3 * r + j];
        R[3 * r + i] = c * u + s * v;
        R[3 * r + j] = c * v - s * u;
    }
}

// the tool placement and, per joint, its axis and its origin in link00
struct Chain {
    double R[9], p[3], axis[NA][3], at[NA][3];
};
template <int AX> Z1_HD void joint(Chain& c, int i, double ox, double oy, double oz, double a)
{
    for (int r = 0; r < 3; ++r) c.p[r] = c.p[r] + (c.R[3 * r] * ox + c.R[3 * r + 1] * oy + c.R[3 * r + 2] * oz);
    rotate<AX>(c.R, a);
    for (int r = 0; r < 3; ++r) {
        c.axis[i][r] = c.R[3 * r + AX];
        c.at[i][r] = c.p[r];
    }
}
Z1_HD void chain(const Params& P, const double* q, Chain& c)
{
    using b2z1::ORIGIN;
    static_assert(b2z1::AXIS[13] == 2 && b2z1::AXIS[14] == 1 && b2z1::AXIS[15] == 1 && b2z1::AXIS[16] == 1 && b2z1::AXIS[17] == 2 &&
                      b2z1::AXIS[18] == 0, "the Z1 axes are z y y y z x");
    for (int k = 0; k < 9; ++k) c.R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    c.p[0] = c.p[1] = c.p[2] = 0.0;
    joint<2>(c, 0, P.joint1_xyz[0], P.joint1_xyz[1], P.joint1_xyz[2], q[0]);
    joint<1>(c, 1, ORIGIN[42], ORIGIN[43], ORIGIN[44], q[1]);
    joint<1>(c, 2, ORIGIN[45], ORIGIN[46], ORIGIN[47], q[2]);
    joint<1>(c, 3, ORIGIN[48], ORIGIN[49], ORIGIN[50], q[3]);
    joint<2>(c, 4, ORIGIN[51], ORIGIN[52], ORIGIN[53], q[4]);
    joint<0>(c, 5, ORIGIN[54], ORIGIN[55], ORIGIN[56], q[5]);
    for (int r = 0; r < 3; ++r) c.p[r] = c.p[r] + (c.R[3 * r] * P.tool_xyz[0] + c.R[3 * r + 1] * P.tool_xyz[1] + c.R[3 * r + 2] * P.tool_xyz[2]);
}

// out = R^T v
Z1_HD void rt_mul(const double* R, const double* v, double* out)
{
    for (int k = 0; k < 3; ++k) out[k] = R[k] * v[0] + R[3 + k] * v[1] + R[6 + k] * v[2];
}

Z1_HD void fk(const Params& P, const double* q, double* R, double* p)
{
    Chain c;
    chain(P, q, c);
    for (int k = 0; k < 9; ++k) R[k] = c.R[k];
    for (int k = 0; k < 3; ++k) p[k] = c.p[k];
}

// J[6][6] row-major: rows 0..2 linear, 3..5 angular, column i for joint i
Z1_HD void jac_of_chain(const Chain& c, double* J)
{
    for (int i = 0; i < NA; ++i) {
        const double* a = c.axis[i];
        const double r[3] = {c.p[0] - c.at[i][0], c.p[1] - c.at[i][1], c.p[2] - c.at[i][2]};
        const double x[3] = {a[1] * r[2] - a[2] * r[1], a[2] * r[0] - a[0] * r[2], a[0] * r[1] - a[1] * r[0]};
        double lin[3], ang[3];
        rt_mul(c.R, x, lin);
        rt_mul(c.R, a, ang);
        for (int k = 0; k < 3; ++k) {
            J[6 * k + i] = lin[k];
            J[6 * (k + 3) + i] = ang[k];
        }
    }
}
Z1_HD void jac_local(const Params& P, const double* q, double* J)
{
    Chain c;
    chain(P, q, c);
    jac_of_chain(c, J);
}

// w[3] and the angle
Z1_HD double log3(const double* R, double* w)
{
    const double s[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
    const double sn = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    const double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    const double theta = std::atan2(sn, c);
    double f;
    if (theta < SMALL_ANGLE) {
        const double t2 = theta * theta;
        f = 1.0 + t2 * (1.0 / 6.0 + t2 * (7.0 / 360.0 + t2 * (31.0 / 15120.0)));
    } else
        f = theta / sn;
    for (int k = 0; k < 3; ++k) w[k] = f * s[k];
    return theta;
}

// alpha = (t / 2) cot(t / 2), beta = (1 - alpha) / t^2, bdot = beta' / t
Z1_HD void alpha_beta(double t, double& alpha, double& beta, double& bdot)
{
    const double t2 = t * t;
    if (t < SMALL_ANGLE) {
        alpha = 1.0 - t2 * (1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0)));
        beta = 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0));
        bdot = 1.0 / 360.0 + t2 * (1.0 / 7560.0);
    } else {
        const double h = 0.5 * t, sh = std::sin(h), ch = std::cos(h);
        alpha = h * ch / sh;
        beta = (1.0 - alpha) / t2;
        bdot = (-2.0 / t2 + (1.0 + 2.0 * sh * ch / t) / (4.0 * sh * sh)) / t2;
    }
}

// out[6] = (v, w)
Z1_HD void log6(const double* R, const double* p, double* out)
{
    double w[3], alpha, beta, bdot;
    const double t = log3(R, w);
    alpha_beta(t, alpha, beta, bdot);
    const double wp = w[0] * p[0] + w[1] * p[1] + w[2] * p[2];
    const double x[3] = {w[1] * p[2] - w[2] * p[1], w[2] * p[0] - w[0] * p[2], w[0] * p[1] - w[1] * p[0]};
    for (int k = 0; k < 3; ++k) {
        out[k] = alpha * p[k] - 0.5 * x[k] + (beta * wp) * w[k];
        out[3 + k] = w[k];
    }
}

// A[9] and B[9] = C A of Jlog6 = [[A, B], [0, A]]
Z1_HD void jlog6_blocks(const double* R, const double* p, double* A, double* B)
{
    double w[3], alpha, beta, bdot, Cm[9];
    const double t = log3(R, w);
    alpha_beta(t, alpha, beta, bdot);
    const double wp = w[0] * p[0] + w[1] * p[1] + w[2] * p[2];
    double u[3];
    for (int k = 0; k < 3; ++k) u[k] = (bdot * wp) * w[k] - (t * t * bdot + 2.0 * beta) * p[k];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            A[3 * r + c] = beta * (w[r] * w[c]) + (r == c ? alpha : 0.0);
            Cm[3 * r + c] = u[r] * w[c] + beta * (w[r] * p[c]) + (r == c ? wp * beta : 0.0);
        }
    // + [w]x / 2 and + [p]x / 2
    A[1] -= 0.5 * w[2]; A[2] += 0.5 * w[1]; A[3] += 0.5 * w[2]; A[5] -= 0.5 * w[0]; A[6] -= 0.5 * w[1]; A[7] += 0.5 * w[0];
    Cm[1] -= 0.5 * p[2]; Cm[2] += 0.5 * p[1]; Cm[3] += 0.5 * p[2]; Cm[5] -= 0.5 * p[0]; Cm[6] -= 0.5 * p[1]; Cm[7] += 0.5 * p[0];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) B[3 * r + c] = Cm[3 * r] * A[c] + Cm[3 * r + 1] * A[3 + c] + Cm[3 * r + 2] * A[6 + c];
}
// the full 6 x 6, row-major (inspection and the harness)
Z1_HD void jlog6(const double* R, const double* p, double* out)
{
    double A[9], B[9];
    jlog6_blocks(R, p, A, B);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            out[6 * r + c] = A[3 * r + c];
            out[6 * r + 3 + c] = B[3 * r + c];
            out[6 * (r + 3) + c] = 0.0;
            out[6 * (r + 3) + 3 + c] = A[3 * r + c];
        }
}

// A x = b for the symmetric 6 x 6 A (the lower triangle is read), LDL^T without pivoting, column by column; b is overwritten
// with x.  false at the first pivot that is not positive and finite
Z1_HD bool ldlt_solve(const double* A, double* b)
{
    double L[36], d[6];
    for (int j = 0; j < 6; ++j) {
        double s = A[6 * j + j];
        for (int k = 0; k < j; ++k) s -= L[6 * j + k] * L[6 * j + k] * d[k];
        if (!(s > 0.0 && s < INFINITY)) return false;
        d[j] = s;
        for (int i = j + 1; i < 6; ++i) {
            double r = A[6 * i + j];
            for (int k = 0; k < j; ++k) r -= L[6 * i + k] * L[6 * j + k] * d[k];
            L[6 * i + j] = r / d[j];
        }
    }
    for (int i = 0; i < 6; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s -= L[6 * i + k] * b[k];
        b[i] = s;
    }
    for (int i = 0; i < 6; ++i) b[i] = b[i] / d[i];
    for (int i = 5; i >= 0; --i) {
        double s = b[i];
        for (int k = i + 1; k < 6; ++k) s -= L[6 * k + i] * b[k];
        b[i] = s;
    }
    return true;
}

Z1_HD double norm6(const double* e) { return std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3] + e[4] * e[4] + e[5] * e[5]); }

// err[6] = log6(oMf^-1 oMdes) of a chain; Ri, pi: iMd
Z1_HD void error_of_chain(const Chain& c, const double* Rd, const double* pd, double* err, double* Ri, double* pi)
{
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) Ri[3 * r + k] = c.R[r] * Rd[k] + c.R[3 + r] * Rd[3 + k] + c.R[6 + r] * Rd[6 + k];
    const double dp[3] = {pd[0] - c.p[0], pd[1] - c.p[1], pd[2] - c.p[2]};
    rt_mul(c.R, dp, pi);
    log6(Ri, pi, err);
}

struct IkResult {
    double err_norm;
    int iterations, status;
};

// target: R row-major [9], then p [3].  q[7] receives the result; q_init may be q
Z1_HD IkResult ik_solve(const Params& P, const double* q_init, const double* target, double* q)
{
    IkResult out;
    for (int i = 0; i < NQ; ++i) q[i] = q_init[i];
    out.iterations = 0;
    if (!(finite_n(q, NQ) && finite_n(target, 12))) {
        out.err_norm = NAN;
        out.status = IK_NOT_FINITE;
        return out;
    }
    out.err_norm = NAN;
    out.status = IK_LIMIT;
    for (int it = 0; it < P.max_iter; ++it) {
        Chain c;
        double err[6], Ri[9], pi[3];
        chain(P, q, c);
        error_of_chain(c, target, target + 9, err, Ri, pi);
        out.err_norm = norm6(err);
        if (out.err_norm < P.eps) {
            out.status = IK_OK;
            break;
        }
        double J[36], Je[36], A[9], B[9], Rt[9], pt[3];
        jac_of_chain(c, J);
        // iMd^-1 = (Ri^T, -Ri^T pi)
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) Rt[3 * r + k] = Ri[3 * k + r];
        rt_mul(Ri, pi, pt);
        for (int k = 0; k < 3; ++k) pt[k] = -pt[k];
        jlog6_blocks(Rt, pt, A, B);
        // Je = -[[A, B], [0, A]] J
        for (int r = 0; r < 3; ++r)
            for (int i = 0; i < NA; ++i) {
                const double top = (A[3 * r] * J[i] + A[3 * r + 1] * J[6 + i] + A[3 * r + 2] * J[12 + i]) +
                                   (B[3 * r] * J[18 + i] + B[3 * r + 1] * J[24 + i] + B[3 * r + 2] * J[30 + i]);
                const double bot = A[3 * r] * J[18 + i] + A[3 * r + 1] * J[24 + i] + A[3 * r + 2] * J[30 + i];
                Je[6 * r + i] = -top;
                Je[6 * (r + 3) + i] = -bot;
            }
        // M = Je Je^T + damp I: the lower triangle
        double M[36];
        for (int r = 0; r < 6; ++r)
            for (int k = 0; k <= r; ++k) {
                double s = 0.0;
                for (int i = 0; i < NA; ++i) s += Je[6 * r + i] * Je[6 * k + i];
                M[6 * r + k] = (r == k) ? s + P.damp : s;
            }
        if (!ldlt_solve(M, err)) {
            out.status = IK_PIVOT;
            break;
        }
        for (int i = 0; i < NA; ++i) {
            double s = 0.0;
            for (int r = 0; r < 6; ++r) s += Je[6 * r + i] * err[r];
            q[i] = q[i] + (-s) * P.dt;
        }
        out.iterations = it + 1;
    }
    return out;
}

// pose[7]: x, y, z, then the quaternion x, y, z, w
Z1_HD void grasp_pose(const double* obj, const double* cfg, double* pose)
{
    const double yaw = obj[3], hp = 0.5 * (cfg[2] * (M_PI / 180.0)), hy = 0.5 * yaw;
    const double sp = std::sin(hp), cp = std::cos(hp), sy = std::sin(hy), cy = std::cos(hy);
    pose[0] = obj[0] - cfg[0] * std::cos(yaw);
    pose[1] = obj[1] - cfg[0] * std::sin(yaw);
    pose[2] = obj[2] + cfg[1];
    pose[3] = -sy * sp;
    pose[4] = cy * sp;
    pose[5] = sy * cp;
    pose[6] = cy * cp;
}

// scipy's Rotation.from_quat(x, y, z, w).as_matrix(): normalised first
Z1_HD void quat_to_rot(const double* qq, double* R)
{
    const double n = std::sqrt(qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2] + qq[3] * qq[3]);
    const double x = qq[0] / n, y = qq[1] / n, z = qq[2] / n, w = qq[3] / n;
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - z * w); R[2] = 2.0 * (x * z + y * w);
    R[3] = 2.0 * (x * y + z * w); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - x * w);
    R[6] = 2.0 * (x * z - y * w); R[7] = 2.0 * (y * z + x * w); R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// target[12] = T_base^-1 T_target with the class's adjustment
Z1_HD void base_target(const double* base_pose, const double* target_pose, int category, double k, double* target)
{
    double Rb[9], Rt[9];
    quat_to_rot(base_pose + 3, Rb);
    quat_to_rot(target_pose + 3, Rt);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) target[3 * r + c] = Rb[r] * Rt[c] + Rb[3 + r] * Rt[3 + c] + Rb[6 + r] * Rt[6 + c];
    const double dp[3] = {target_pose[0] - base_pose[0], target_pose[1] - base_pose[1], target_pose[2] - base_pose[2]};
    rt_mul(Rb, dp, target + 9);
    if (category == CATEGORY_BOX)
        target[11] -= k / 2.2;
    else if (category == CATEGORY_TABLE) {
        target[9] += k / 1.5;
        target[11] -= 0.01;
    } else {
        target[9] += k;
        target[11] += 0.03;
    }
}

// one robot's resident state: the attributes of :143-151 and what the FSM publishes
struct Grasp {
    double k, d_gripper, gripper_ang, err_norm;
    int grasp_time, flag, stable, done, ik_iterations, ik_status;
    double joint_cmd[7], robot_vel_cmd[3];
};
// :143-151; d_gripper 0: before the first grasp
Z1_HD void grasp_reset(Grasp& g)
{
    g.k = 0.0;
    g.d_gripper = 0.0;
    g.gripper_ang = GRIPPER_OPEN;
    g.err_norm = ERR_RESET;
    g.grasp_time = 0;
    g.flag = 0;
    g.stable = 0;
}
Z1_HD void grasp_initial(const Params& P, Grasp& g)
{
    grasp_reset(g);
    g.done = 0;
    g.ik_iterations = 0;
    g.ik_status = IK_NOT_RUN;
    for (int i = 0; i < 7; ++i) g.joint_cmd[i] = P.joint_default[i];
    g.robot_vel_cmd[0] = g.robot_vel_cmd[1] = g.robot_vel_cmd[2] = 0.0;
}
Z1_HD void set_vel(Grasp& g, double vx)
{
    g.robot_vel_cmd[0] = vx;
    g.robot_vel_cmd[1] = 0.0;
    g.robot_vel_cmd[2] = 0.0;
}

// object_grasp, :643-749.  robot_xy[2], object_pose[4] (x, y, z, yaw), arm_base_pose[7], joint_positions[7] (the measured arm
// joints: entries 8 and 13..18 of the reference's joint vector).  Returns done
Z1_HD int grasp_step(const Params& P, const Class& c, Grasp& g, const double* robot_xy, const double* object_pose, const double* arm_base_pose,
                     const double* joint_positions)
{
    g.ik_iterations = 0;
    g.ik_status = IK_NOT_RUN;
    g.done = 0;
    g.grasp_time += 1; // 1
    const double dx = robot_xy[0] - object_pose[0], dy = robot_xy[1] - object_pose[1];
    const double gap = std::sqrt(dx * dx + dy * dy) - c.plan_cfg[0]; // 2
    if (!g.flag) {                                                   // 3
        for (int i = 0; i < 7; ++i) g.joint_cmd[i] = P.joint_default[i];
        if (gap > REACH_BAND)
            set_vel(g, APPROACH_SPEED);
        else if (gap < -REACH_BAND)
            set_vel(g, -APPROACH_SPEED);
        else {
            set_vel(g, 0.0);
            g.flag = 1;
        }
        return 0;
    }
    if (g.grasp_time < WAIT_TICKS) return 0; // 4
    g.stable = (g.err_norm < ERR_STABLE) ? g.stable + 1 : 0; // 5
    if (g.stable > STABLE_TICKS || g.grasp_time > TIMEOUT_TICKS) g.d_gripper = D_GRIPPER;
    g.k = g.k + g.d_gripper;
    g.k = g.k < K_MAX ? g.k : K_MAX;
    double pose[7], target[12], q[7];
    grasp_pose(object_pose, c.grasp_cfg, pose);
    base_target(arm_base_pose, pose, c.category, g.k, target);
    const IkResult r = ik_solve(P, joint_positions, target, q); // 6
    g.err_norm = r.err_norm;
    g.ik_iterations = r.iterations;
    g.ik_status = r.status;
    g.gripper_ang += g.d_gripper; // 7
    g.gripper_ang = g.gripper_ang < GRIPPER_CLOSED ? g.gripper_ang : GRIPPER_CLOSED;
    g.gripper_ang = g.gripper_ang > GRIPPER_OPEN ? g.gripper_ang : GRIPPER_OPEN;
    q[6] = g.gripper_ang;
    if (c.category == CATEGORY_TABLE && g.gripper_ang >= GRIPPER_TABLE)
        for (int i = 0; i < 6; ++i) q[i] = c.arm_default_pose[i];
    if (g.gripper_ang >= GRIPPER_CLOSED) { // 8
        g.d_gripper = D_GRIPPER;
        g.k = 0.0;
        g.gripper_ang = GRIPPER_OPEN;
        g.err_norm = ERR_RESET;
        g.stable = 0;
        g.flag = 0;
        g.grasp_time = 0;
        g.done = 1;
        return 1;
    }
    for (int i = 0; i < 7; ++i) g.joint_cmd[i] = q[i]; // 9
    return 0;
}

} // namespace z1
#endif
