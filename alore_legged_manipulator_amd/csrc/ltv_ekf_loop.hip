// ltv_ekf_loop.hip -- the third launch of the LTV-MPC closed loop on the ICR EKF's estimate (include/alore_ltv_mpc.h:
// alore_ltv_plant_ekf_step, alore_ltv_ekf_closed_loop_run): the `mpc` node's plant on the TRUE state with the simulator's noise
// (ltv_plant::step_noisy), the simulator's ControlPub message, the filter step on the NMPC handle's filter (icrekf::step_robot),
// the trace record.  One thread per robot: the covariance lives in that thread's registers from the load to the store; no LDS, no
// scratch (registers: profiles/ltv_ekf_loop.txt).  Sampling and the solve of that loop are the kernels of ltv_mpc_capi.hip and
// ltv_mpc.hip, handed est_pose where they take the plant's pose.
// Three launches per tick on purpose: see DESIGN 7c.
#include "ltv_ekf_loop.h"
#include "ltv_plant_device.h" // ltv::plant_robot: load -> ltv_plant::step_noisy -> store and trace record for one robot
#include "icr_ekf_device.h" // last: icr_ekf.h switches contraction off for what follows it

namespace ltv {

__global__ void __launch_bounds__(64) plant_ekf_kernel(PlantEkf a, icrekf::Dev d, icrekf::Params ep)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.B) return;
    const bool has = a.meta ? a.meta[(size_t)r * 8 + 6] != 0.0 : true;
    // 1. the plant step on the true state, PoseSub with the noise (and 5., the plant's part of the trace record, as
    // plant_step_kernel writes it: here, so that its pointers are not held in scalar registers across the filter step)
    ltv_plant::Noise nz;
    nz.stddev = a.noise_stddev; nz.seed = a.seed; nz.event = a.event; nz.robot = (uint32_t)r;
    ltv_plant::State st;
    plant_robot(a, r, has, a.goal[r], nz, true, st);
    // 2. ControlPub from the true ICR and the velocities after the step: (left, right)
    const double yr = a.icr[(size_t)r * 3 + 1], yl = a.icr[(size_t)r * 3 + 2];
    const double wheel[2] = {st.v - st.w * yl, st.v - st.w * yr};
    // 3., 4. the filter step, with the pose update where this tick has one
    double z[3] = {st.x, st.y, st.th};
    if (a.do_update && (a.meas_stddev[0] > 0.0 || a.meas_stddev[1] > 0.0 || a.meas_stddev[2] > 0.0)) {
        double n0, n1, n2, unused;
        sim_noise::normal2(a.seed, (uint32_t)r, a.event, sim_noise::STREAM_MEAS_XY, n0, n1);
        sim_noise::normal2(a.seed, (uint32_t)r, a.event, sim_noise::STREAM_MEAS_TH, n2, unused);
        z[0] = st.x + a.meas_stddev[0] * n0; z[1] = st.y + a.meas_stddev[1] * n1; z[2] = st.th + a.meas_stddev[2] * n2;
    }
    icrekf::step_robot(d, ep, r, wheel, a.dt, z, a.do_update != 0);
    // 5. the trace record: the estimate as the filter step has left it (where the step failed, what it was), and the status
    if (a.tr_est) {
        a.tr_est[(size_t)r * 3] = d.est_pose[(size_t)r * 3]; a.tr_est[(size_t)r * 3 + 1] = d.est_pose[(size_t)r * 3 + 1];
        a.tr_est[(size_t)r * 3 + 2] = d.est_pose[(size_t)r * 3 + 2];
        a.tr_ekf_status[r] = d.status[r];
    }
}

// thread = (event, robot)
__global__ void noise_draws_kernel(uint64_t seed, int B, uint64_t event0, int n_events, int noise_stream, double* out)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)n_events * B) return;
    const int e = (int)(t / B), r = (int)(t % B);
    double z0, z1;
    sim_noise::normal2(seed, (uint32_t)r, event0 + (uint64_t)e, (uint32_t)noise_stream, z0, z1);
    out[(size_t)t * 2] = z0; out[(size_t)t * 2 + 1] = z1;
}

bool ekf_info(void* nmpc, EkfInfo* out)
{
    icrekf::Access acc;
    if (!nmpc || alore_nmpc_internal_ekf(nmpc, &acc) != 0) return false;
    out->capacity = acc.capacity; out->device = acc.device; out->odom_every = acc.odom_every; out->ticks = acc.ticks;
    out->est_pose = acc.d.est_pose;
    return true;
}

hipError_t launch_plant_ekf(const PlantEkf& a, void* nmpc, hipStream_t s)
{
    icrekf::Access acc;
    if (alore_nmpc_internal_ekf(nmpc, &acc) != 0 || a.B > acc.capacity) return hipErrorInvalidValue;
    hipLaunchKernelGGL(plant_ekf_kernel, dim3((a.B + 63) / 64), dim3(64), 0, s, a, acc.d, acc.p);
    return hipGetLastError();
}

hipError_t launch_noise_draws(uint64_t seed, int B, uint64_t event0, int n_events, int noise_stream, double* out, hipStream_t s)
{
    const long total = (long)n_events * B;
    hipLaunchKernelGGL(noise_draws_kernel, dim3((unsigned)((total + 127) / 128)), dim3(128), 0, s, seed, B, event0, n_events, noise_stream, out);
    return hipGetLastError();
}

} // namespace ltv
