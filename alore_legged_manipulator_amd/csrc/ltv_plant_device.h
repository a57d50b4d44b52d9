// ltv_plant_device.h -- the plant step of one robot of the LTV-MPC closed loops as the kernels run it (internal): load, the step of
// ltv_plant.h, store, and the plant's part of the trace record.  Read by ltv::plant_step_kernel and ltv::pre_tick_kernel
// (ltv_mpc_capi.hip) and by ltv::plant_ekf_kernel (ltv_ekf_loop.hip).  It reads no filter header; where icr_ekf_device.h is read
// too, this one comes first (icr_ekf.h switches contraction off for what follows it).
#ifndef ALORE_LTV_PLANT_DEVICE_H
#define ALORE_LTV_PLANT_DEVICE_H

#include <hip/hip_runtime.h>

#include "ltv_plant.h"

namespace ltv {

// The plant step of robot r and its trace record.  Args: the kernel-argument struct (PreTick, PlantEkf), of which p, pose, stride,
// cmd, status, tr_pose and tr_status are read.  has / goal: the robot has a trajectory / the at-goal flag of the tick.  nz.stddev ==
// 0: no noise.  Every calling lane computes, `writer` lanes store.  st: the state after the step.
template <class Args>
__device__ __forceinline__ void plant_robot(const Args& a, int r, bool has, int goal, const ltv_plant::Noise& nz, bool writer, ltv_plant::State& st)
{
    double* const vwp = a.pose + (size_t)a.stride * 3;
    double* const desp = a.pose + (size_t)a.stride * 5;
    st.x = a.pose[(size_t)r * 3]; st.y = a.pose[(size_t)r * 3 + 1]; st.th = a.pose[(size_t)r * 3 + 2];
    st.v = vwp[(size_t)r * 2]; st.w = vwp[(size_t)r * 2 + 1];
    st.dv = desp[(size_t)r * 2]; st.dw = desp[(size_t)r * 2 + 1];
    const double cv = a.cmd[(size_t)r * 2], cw = a.cmd[(size_t)r * 2 + 1];
    const int status = a.status[r];
    ltv_plant::step_noisy(a.p, has, goal != 0, cv, cw, nz, st);
    if (!writer) return;
    a.pose[(size_t)r * 3] = st.x; a.pose[(size_t)r * 3 + 1] = st.y; a.pose[(size_t)r * 3 + 2] = st.th;
    vwp[(size_t)r * 2] = st.v; vwp[(size_t)r * 2 + 1] = st.w;
    desp[(size_t)r * 2] = st.dv; desp[(size_t)r * 2 + 1] = st.dw;
    if (a.tr_pose) {
        a.tr_pose[(size_t)r * 3] = st.x; a.tr_pose[(size_t)r * 3 + 1] = st.y; a.tr_pose[(size_t)r * 3 + 2] = st.th;
        double* const tc = a.tr_pose + (size_t)a.stride * 3;
        tc[(size_t)r * 2] = (has && goal) ? 0.0 : cv; tc[(size_t)r * 2 + 1] = (has && goal) ? 0.0 : cw;
        a.tr_status[r] = status; a.tr_status[(size_t)a.stride + r] = goal;
    }
}

} // namespace ltv
#endif
