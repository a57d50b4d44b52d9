// plant_substeps.h -- the propagation steps of the simulator's plant and its wheel-speed command decode, the arithmetic once
// (internal).  Plain C++17: __host__ __device__ under hipcc, no HIP dependency otherwise.  Read by the NMPC closed loops
// (nmpc::plant_kernel, nmpc::plant_ahead_one, icrekf::plant_ekf_kernel: wheel_plant_step, through nmpc_kernels.h) and by the plant
// of the `mpc` node (ltv_plant.h: plant_substeps).
#ifndef ALORE_PLANT_SUBSTEPS_H
#define ALORE_PLANT_SUBSTEPS_H

#include <cmath>

#if defined(__HIPCC__)
#define PLANT_HD __host__ __device__ __forceinline__
#else
#define PLANT_HD inline
#endif

namespace nmpc {

struct PlantParams { // simulator.h: max_a_, max_domega_, Pose_pub_rate_ (a period), State_Propa_rate_ (a period)
    double max_a, max_domega, pose_pub_period, propa_period;
    int substeps; // StatePropaCallback calls per control tick
};

// The substeps of one control tick (StatePropaCallback, simulator.h:234-275).  The heading changes once per substep and its sine /
// cosine after the update are those the next substep starts with: one evaluation per tick, then a rotation by the substep's angle
// w * period -- a few milliradians, whose sine and cosine are short series (next terms d^9 / 9! and d^8 / 8!: below the last bit
// for |d| < 0.03); a larger angle takes the full evaluation.  The reference calls cos and sin four times per substep; the rotation
// differs from them by rounding (1e-16 per substep, nothing carried over to the next tick).
PLANT_HD void plant_substeps(const PlantParams& p, double desired_v, double desired_w, double vy, double& x, double& y, double& th,
                             double& v, double& w)
{
    double sn, cs;
    sincos(th, &sn, &cs);
    for (int k = 0; k < p.substeps; ++k) {
        if (fabs(v - desired_v) >= p.pose_pub_period * p.max_a) v += p.pose_pub_period * p.max_a * (desired_v - v) / fabs(desired_v - v);
        else v = desired_v;
        if (fabs(w - desired_w) >= p.pose_pub_period * p.max_domega) w += p.pose_pub_period * p.max_domega * (desired_w - w) / fabs(desired_w - w);
        else w = desired_w;
        x += v * p.propa_period * cs;
        y += v * p.propa_period * sn;
        const double d = w * p.propa_period;
        th += d;
        if (fabs(d) < 0.03) {
            const double d2 = d * d;
            const double sd = d * (1.0 - d2 * (1.0 / 6.0) * (1.0 - d2 * (1.0 / 20.0) * (1.0 - d2 * (1.0 / 42.0))));
            const double cd = 1.0 - d2 * 0.5 * (1.0 - d2 * (1.0 / 12.0) * (1.0 - d2 * (1.0 / 30.0)));
            const double c1 = cs * cd - sn * sd, s1 = sn * cd + cs * sd;
            cs = c1; sn = s1;
        } else {
            sincos(th, &sn, &cs);
        }
        x -= vy * p.propa_period * sn;
        y += vy * p.propa_period * cs;
    }
}

// One control tick of one robot's plant under a wheel-speed command (right, left): ControlSubCallback (simulator.h:234-242) turns
// it into (v, vy, omega) through the robot's ICR (xv, yr, yl), then the substeps above.  Pose and velocities in and out in the
// caller's registers.  The decode is compiled without contraction wherever it is read, so that it is the same instructions in
// every kernel.
PLANT_HD void wheel_plant_step(const PlantParams& p, double right, double left, double xv, double yr, double yl, double& x, double& y,
                               double& th, double& v, double& w)
{
    double desired_v, vy, desired_w;
    {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        desired_v = (left + right) / 2.0 - (right - left) / (yl - yr) * (yl + yr) / 2.0;
        vy = -(right - left) / (yl - yr) * xv;
        desired_w = (right - left) / (yl - yr);
    }
    plant_substeps(p, desired_v, desired_w, vy, x, y, th, v, w);
}

} // namespace nmpc
#endif
