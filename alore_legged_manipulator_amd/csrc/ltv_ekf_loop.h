// ltv_ekf_loop.h -- what ltv_mpc_capi.hip (the C ABI) needs of ltv_ekf_loop.hip (the kernels of the LTV-MPC closed loop on the
// ICR EKF's estimate) (internal).  No filter type appears here on purpose: icr_ekf.h switches contraction off for the rest of a
// translation unit, and the kernels of ltv_mpc_capi.hip keep the code they have.
#ifndef ALORE_LTV_EKF_LOOP_H
#define ALORE_LTV_EKF_LOOP_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/alore_ltv_mpc.h"

namespace ltv {

// the filter of an NMPC handle as the C ABI sees it (alore_nmpc_internal_ekf behind it); false: no handle or no alore_nmpc_ekf_init
struct EkfInfo {
    int capacity, device, odom_every;
    long* ticks;            // the handle's closed-loop ticks since alore_nmpc_ekf_reset
    const double* est_pose; // [capacity][3]
};
bool ekf_info(void* nmpc, EkfInfo* out);

struct PlantEkf {
    alore_ltv_plant_params p;
    const double* meta;   // RefStore::meta of the last sampling, or null: every robot counts as having a trajectory
    int B, stride;        // robots of the launch; robots the plant's slabs and the trace records are laid out for
    const int* goal;      // [B] at-goal flags of the sampling the last solve used
    double* pose;         // the plant, one slab: pose [stride][3], then vw [stride][2], then desired [stride][2]
    const double* cmd;    // [B][2] of the last solve
    const int* status;    // [B]
    const double* icr;    // [stride][3] the true (xv, yr, yl)
    double* tr_pose;      // the trace record, or null: pose [stride][3], then cmd [stride][2]
    int* tr_status;       // status [stride], then at_goal [stride]
    double* tr_est;       // est [stride][3]
    int* tr_ekf_status;   // [stride]
    double dt;            // the filter's step
    int do_update;        // a pose update on this step
    double noise_stddev, meas_stddev[3];
    uint64_t seed, event;
};
// plant + ControlPub + filter step + trace record of a.B robots on the filter of `nmpc` (checked by the caller with ekf_info)
hipError_t launch_plant_ekf(const PlantEkf& a, void* nmpc, hipStream_t s);
// out DEVICE [n_events][B][2]: sim_noise::normal2(seed, robot, event0 + e, noise_stream)
hipError_t launch_noise_draws(uint64_t seed, int B, uint64_t event0, int n_events, int noise_stream, double* out, hipStream_t s);

} // namespace ltv
#endif
