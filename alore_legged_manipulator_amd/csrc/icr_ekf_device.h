// icr_ekf_device.h -- what the kernels that run the ICR EKF share (internal): the filter's device arrays, one robot's
// load -> icrekf::step_one -> store, and the view of an NMPC handle's filter that the LTV-MPC closed loop takes.
// Read by icr_ekf.hip and ltv_ekf_loop.hip.  Include it LAST: icr_ekf.h switches contraction off for what follows it.
#ifndef ALORE_ICR_EKF_DEVICE_H
#define ALORE_ICR_EKF_DEVICE_H

#include <hip/hip_runtime.h>

#include "icr_ekf.h"

namespace icrekf {

struct Dev { // the filter's device arrays, [capacity] robots each
    double *x, *P, *u, *est_pose, *est_icr;
    Flags* f;
    int* status;
};

// load -> step_one -> store for robot r; wheel and z (read when has_z) in registers of the caller
__device__ __forceinline__ void step_robot(const Dev& d, const Params& p, int r, const double* wheel, double dt, const double* z, bool has_z)
{
    double x[6], P[36], u[2];
    const double2* gx = reinterpret_cast<const double2*>(d.x + (size_t)r * 6);   // 48-, 288- and 16-byte records: 16-byte aligned
    const double2* gP = reinterpret_cast<const double2*>(d.P + (size_t)r * 36);
    IE_UNROLL for (int i = 0; i < 3; ++i) { const double2 v = gx[i]; x[2 * i] = v.x; x[2 * i + 1] = v.y; }
    IE_UNROLL for (int i = 0; i < 18; ++i) { const double2 v = gP[i]; P[2 * i] = v.x; P[2 * i + 1] = v.y; }
    { const double2 v = *reinterpret_cast<const double2*>(d.u + (size_t)r * 2); u[0] = v.x; u[1] = v.y; }
    Flags f = d.f[r];
    const int st = step_one(p, x, P, u, f, wheel, dt, z, has_z, nullptr);
    d.status[r] = st;
    if (st != OK) return; // x, P, u, flags and the published estimate stay exactly as they were
    double2* sx = reinterpret_cast<double2*>(d.x + (size_t)r * 6);
    double2* sP = reinterpret_cast<double2*>(d.P + (size_t)r * 36);
    IE_UNROLL for (int i = 0; i < 3; ++i) sx[i] = make_double2(x[2 * i], x[2 * i + 1]);
    IE_UNROLL for (int i = 0; i < 18; ++i) sP[i] = make_double2(P[2 * i], P[2 * i + 1]);
    *reinterpret_cast<double2*>(d.u + (size_t)r * 2) = make_double2(u[0], u[1]);
    d.f[r] = f;
    d.est_pose[(size_t)r * 3] = x[0]; d.est_pose[(size_t)r * 3 + 1] = x[1]; d.est_pose[(size_t)r * 3 + 2] = x[2];
    d.est_icr[(size_t)r * 3] = x[5]; d.est_icr[(size_t)r * 3 + 1] = x[3]; d.est_icr[(size_t)r * 3 + 2] = x[4]; // (xv, yr, yl)
}

// alore_nmpc_internal_ekf: the filter of an NMPC handle as another library part drives it -- the arrays themselves (no copy), the
// parameters, and the handle's count of closed-loop ticks since the reset, which the caller advances
struct Access {
    Dev d;
    Params p;
    int odom_every;
    long* ticks;
    int capacity, device;
};

} // namespace icrekf

// internal (not in the public header), beside alore_nmpc_internal_refstore; nonzero: no handle or no alore_nmpc_ekf_init
extern "C" int alore_nmpc_internal_ekf(void* nmpc_handle, icrekf::Access* out);

#endif
