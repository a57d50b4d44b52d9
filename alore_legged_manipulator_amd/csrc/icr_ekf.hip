// icr_ekf.hip -- the ICR EKF of csrc/icr_ekf.h for B robots on the device, and the part of the C ABI of include/alore_nmpc.h that
// drives it (alore_nmpc_ekf_*): the stand-alone filter step, and the closed loop of the NMPC on the filter's estimate.
// One thread per robot: the 6 x 6 covariance, the state and the flags of a robot live in that thread's registers from the load to
// the store; no LDS, no scratch (registers: profiles/icr_ekf.txt).  The arithmetic is the header's, nothing is restated here.
#include "ltv_host_plan.h" // the update schedule, shared with the LTV-MPC loop on this filter
#include "nmpc_solver.h" // (before icr_ekf.h: that header switches contraction off for what follows it)
#include "icr_ekf_device.h" // icr_ekf.h, icrekf::Dev and step_robot: load -> step_one -> store for one robot

using namespace nmpc_capi;

namespace icrekf {

// forecast with the held u over dt, u <- wheel, update where meas is given, flags
__global__ void __launch_bounds__(64) step_kernel(Dev d, Params p, int B, const double* wheel, double dt, const double* meas,
                                                  const unsigned char* mask)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B) return;
    if (mask && !mask[r]) { d.status[r] = MASKED; return; }
    const double w[2] = {wheel[(size_t)r * 2], wheel[(size_t)r * 2 + 1]};
    double z[3] = {0.0, 0.0, 0.0};
    if (meas) { z[0] = meas[(size_t)r * 3]; z[1] = meas[(size_t)r * 3 + 1]; z[2] = meas[(size_t)r * 3 + 2]; }
    step_robot(d, p, r, w, dt, z, meas != nullptr);
}

// The third launch of the EKF closed loop: the simulator's plant on the TRUE state (nmpc::wheel_plant_step, as nmpc::plant_kernel
// runs it), its ControlPub message (simulator.h:342-347), the filter step.
__global__ void __launch_bounds__(64) plant_ekf_kernel(alore_nmpc_batch b, int B, int N, int node, const double* icr, const int* at_goal,
                                                       double* pose, double* vw, nmpc::PlantParams pp, Dev d, Params p, double dt,
                                                       int do_update, const double* noise)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B) return;
    double right = (double)b.u[((size_t)r * N + node) * 2], left = (double)b.u[((size_t)r * N + node) * 2 + 1];
    if (at_goal && at_goal[r]) { right = 0.0; left = 0.0; }
    const double xv = icr[(size_t)r * 3], yr = icr[(size_t)r * 3 + 1], yl = icr[(size_t)r * 3 + 2];
    double x = pose[(size_t)r * 3], y = pose[(size_t)r * 3 + 1], th = pose[(size_t)r * 3 + 2];
    double v = vw[(size_t)r * 2], w = vw[(size_t)r * 2 + 1];
    nmpc::wheel_plant_step(pp, right, left, xv, yr, yl, x, y, th, v, w);
    pose[(size_t)r * 3] = x; pose[(size_t)r * 3 + 1] = y; pose[(size_t)r * 3 + 2] = th;
    vw[(size_t)r * 2] = v; vw[(size_t)r * 2 + 1] = w;
    const double wheel[2] = {v - w * yl, v - w * yr}; // (left, right)
    double z[3] = {x, y, th};
    if (do_update && noise) { z[0] = x + noise[(size_t)r * 3]; z[1] = y + noise[(size_t)r * 3 + 1]; z[2] = th + noise[(size_t)r * 3 + 2]; }
    step_robot(d, p, r, wheel, dt, z, do_update != 0);
}

// alore_nmpc_ekf_reset: pose_in / icr_in are device copies of the caller's arrays or nullptr (the plant's pose / init_icr)
__global__ void reset_kernel(Dev d, int B, const double* pose_in, const double* icr_in, const unsigned char* mask,
                             const double* plant_pose, double yr0, double yl0, double xv0)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B || (mask && !mask[r])) return;
    const double* ps = (pose_in ? pose_in : plant_pose) + (size_t)r * 3;
    double x[6] = {ps[0], ps[1], ps[2], yr0, yl0, xv0};
    if (icr_in) { x[3] = icr_in[(size_t)r * 3]; x[4] = icr_in[(size_t)r * 3 + 1]; x[5] = icr_in[(size_t)r * 3 + 2]; }
    for (int i = 0; i < 6; ++i) d.x[(size_t)r * 6 + i] = x[i];
    for (int i = 0; i < 36; ++i) d.P[(size_t)r * 36 + i] = 0.0;
    d.u[(size_t)r * 2] = 0.0; d.u[(size_t)r * 2 + 1] = 0.0;
    Flags f;
    reset_flags(f);
    d.f[r] = f;
    d.status[r] = OK;
    d.est_pose[(size_t)r * 3] = x[0]; d.est_pose[(size_t)r * 3 + 1] = x[1]; d.est_pose[(size_t)r * 3 + 2] = x[2];
    d.est_icr[(size_t)r * 3] = x[5]; d.est_icr[(size_t)r * 3 + 1] = x[3]; d.est_icr[(size_t)r * 3 + 2] = x[4];
}

} // namespace icrekf

namespace {
// the one allocation of alore_nmpc_ekf_init, cut up: doubles first, then ints, then bytes
struct Layout {
    icrekf::Dev d;
    double *in_pose, *in_icr; // staging of alore_nmpc_ekf_reset's host arrays
    unsigned char* in_mask;
};
size_t ekf_bytes(int Bc) { return sizeof(double) * Bc * (6 + 36 + 2 + 3 + 3 + 3 + 3) + sizeof(icrekf::Flags) * Bc + sizeof(int) * Bc + (size_t)Bc; }
Layout ekf_layout(char* base, int Bc)
{
    Layout L;
    double* p = reinterpret_cast<double*>(base);
    L.d.P = p; p += (size_t)Bc * 36;
    L.d.x = p; p += (size_t)Bc * 6;
    L.d.u = p; p += (size_t)Bc * 2;
    L.d.est_pose = p; p += (size_t)Bc * 3;
    L.d.est_icr = p; p += (size_t)Bc * 3;
    L.in_pose = p; p += (size_t)Bc * 3;
    L.in_icr = p; p += (size_t)Bc * 3;
    L.d.f = reinterpret_cast<icrekf::Flags*>(p);
    L.d.status = reinterpret_cast<int*>(L.d.f + Bc);
    L.in_mask = reinterpret_cast<unsigned char*>(L.d.status + Bc);
    return L;
}
icrekf::Params ekf_params(const alore_ekf_params& a)
{
    icrekf::Params p;
    for (int i = 0; i < 6; ++i) p.q[i] = a.q[i];
    for (int i = 0; i < 3; ++i) { p.r[i] = a.r[i]; p.standard[i] = a.standard[i]; }
    return p;
}
bool ekf_ready(alore_nmpc_handle h, int B) { return h && h->ekf.d_block && B > 0 && B <= h->ekf.B; }

// one tick of the EKF closed loop, arguments checked by the callers
int ekf_tick(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, double now, double dt_tick, int delay_num, const double* d_noise,
             void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int N = h->cfg.N;
    const Layout L = ekf_layout(h->ekf.d_block, h->ekf.B);
    if (int rc = nmpc_capi::promote_if_due(h, now, s)) return rc; // a pending trajectory whose start time has passed (mpc.cpp:177-182)
    // CmdCallback on the estimate: ~odom = EKF_XYTheta, od = EKF_ICR
    HIP_TRY(h, nmpc::launch_ref_sample(h->refs.store, *dev, B, N, (double)h->cfg.dt, now, L.d.est_pose, L.d.est_icr, h->refs.d_goal, h->refs.d_psi, 1, s));
    const int rc = alore_nmpc_rti(h, dev, B, 1, stream);
    if (rc != ALORE_NMPC_OK) return rc;
    if (h->handoff.d_stopped) // alore_nmpc_refs_stop: the zero command holds while the robot has no trajectory
        HIP_TRY(h, nmpc::launch_stop_hold(dev->u, h->refs.store.meta, h->handoff.d_stopped, B, N, delay_num < N ? delay_num : N - 1, s));
    h->ekf.ticks += 1;
    const int do_update = ltv_plan::is_update_tick(h->ekf.ticks, h->ekf.params.odom_every) ? 1 : 0;
    hipLaunchKernelGGL(icrekf::plant_ekf_kernel, dim3((B + 63) / 64), dim3(64), 0, s, *dev, B, N, delay_num < N ? delay_num : N - 1,
                       h->refs.d_icr, h->refs.d_goal, h->refs.d_est, h->refs.d_vw, h->refs.plant, L.d, ekf_params(h->ekf.params), dt_tick,
                       do_update, d_noise);
    HIP_TRY(h, hipGetLastError());
    return ALORE_NMPC_OK;
}
} // namespace

extern "C" {

void alore_nmpc_ekf_default_params(alore_ekf_params* p)
{
    if (!p) return;
    const alore_ekf_params d = {{0.5, 0.5, 1.14, 0.1, 0.1, 0.1}, {0.1, 0.1, 0.1}, {-0.25, 0.25, 0.1}, {-0.3, 0.3, 0.2}, 10};
    *p = d;
}

int alore_nmpc_ekf_init(alore_nmpc_handle h, const alore_ekf_params* params)
{
    if (!h || !h->refs.store.dur || !params || params->odom_every < 1 || h->ekf.d_block)
        return fail(h, ALORE_NMPC_E_INVALID, "ekf_init: needs refs_init first, odom_every >= 1, and is called once");
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(params->q[i])) return fail(h, ALORE_NMPC_E_INVALID, "ekf_init: q is not finite");
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(params->r[i]) || !std::isfinite(params->init_icr[i]) || !std::isfinite(params->standard[i]))
            return fail(h, ALORE_NMPC_E_INVALID, "ekf_init: r, init_icr or standard is not finite");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int Bc = h->refs.B;
    hipError_t e = hipMalloc((void**)&h->ekf.d_block, ekf_bytes(Bc));
    if (e == hipSuccess) e = hipMemset(h->ekf.d_block, 0, ekf_bytes(Bc));
    if (e != hipSuccess) {
        if (h->ekf.d_block) (void)hipFree(h->ekf.d_block);
        h->ekf.d_block = nullptr;
        return fail(h, ALORE_NMPC_E_NOMEM, "ekf_init: hipMalloc", e);
    }
    h->ekf.B = Bc;
    h->ekf.params = *params;
    h->ekf.ticks = 0;
    return ALORE_NMPC_OK;
}

int alore_nmpc_ekf_reset(alore_nmpc_handle h, int B, const double* pose, const double* icr0, const unsigned char* mask, void* stream)
{
    if (!ekf_ready(h, B) || (!pose && !h->refs.has_plant)) return fail(h, ALORE_NMPC_E_INVALID, "ekf_reset: bad argument (pose NULL needs the plant)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    const Layout L = ekf_layout(h->ekf.d_block, h->ekf.B);
    if (pose) HIP_TRY(h, hipMemcpyAsync(L.in_pose, pose, sizeof(double) * B * 3, hipMemcpyHostToDevice, s));
    if (icr0) HIP_TRY(h, hipMemcpyAsync(L.in_icr, icr0, sizeof(double) * B * 3, hipMemcpyHostToDevice, s));
    if (mask) HIP_TRY(h, hipMemcpyAsync(L.in_mask, mask, (size_t)B, hipMemcpyHostToDevice, s));
    if (pose || icr0 || mask) HIP_TRY(h, hipStreamSynchronize(s)); // the host buffers may go away after return
    const double* ic = h->ekf.params.init_icr;
    hipLaunchKernelGGL(icrekf::reset_kernel, dim3((B + 63) / 64), dim3(64), 0, s, L.d, B, pose ? L.in_pose : nullptr, icr0 ? L.in_icr : nullptr,
                       mask ? L.in_mask : nullptr, h->refs.d_est, ic[0], ic[1], ic[2]);
    HIP_TRY(h, hipGetLastError());
    h->ekf.ticks = 0;
    return ALORE_NMPC_OK;
}

int alore_nmpc_ekf_set_state(alore_nmpc_handle h, int B, const double* x, const double* P, const double* u, void* stream)
{
    if (!ekf_ready(h, B)) return fail(h, ALORE_NMPC_E_INVALID, "ekf_set_state: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    const Layout L = ekf_layout(h->ekf.d_block, h->ekf.B);
    if (x) HIP_TRY(h, hipMemcpyAsync(L.d.x, x, sizeof(double) * B * 6, hipMemcpyHostToDevice, s));
    if (P) HIP_TRY(h, hipMemcpyAsync(L.d.P, P, sizeof(double) * B * 36, hipMemcpyHostToDevice, s));
    if (u) HIP_TRY(h, hipMemcpyAsync(L.d.u, u, sizeof(double) * B * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return ALORE_NMPC_OK;
}

int alore_nmpc_ekf_step(alore_nmpc_handle h, int B, const double* d_wheel, double dt, const double* d_meas, const unsigned char* d_mask,
                        void* stream)
{
    if (!ekf_ready(h, B) || !d_wheel) return fail(h, ALORE_NMPC_E_INVALID, "ekf_step: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const Layout L = ekf_layout(h->ekf.d_block, h->ekf.B);
    hipLaunchKernelGGL(icrekf::step_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, L.d, ekf_params(h->ekf.params), B, d_wheel, dt,
                       d_meas, d_mask);
    HIP_TRY(h, hipGetLastError());
    return ALORE_NMPC_OK;
}

int alore_nmpc_ekf_get(alore_nmpc_handle h, int B, double* x, double* P, int* status, int* conv_step)
{
    if (!ekf_ready(h, B)) return fail(h, ALORE_NMPC_E_INVALID, "ekf_get: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipDeviceSynchronize());
    const Layout L = ekf_layout(h->ekf.d_block, h->ekf.B);
    if (x) HIP_TRY(h, hipMemcpy(x, L.d.x, sizeof(double) * B * 6, hipMemcpyDeviceToHost));
    if (P) HIP_TRY(h, hipMemcpy(P, L.d.P, sizeof(double) * B * 36, hipMemcpyDeviceToHost));
    if (status) HIP_TRY(h, hipMemcpy(status, L.d.status, sizeof(int) * B, hipMemcpyDeviceToHost));
    if (conv_step) {
        std::vector<icrekf::Flags> f(B);
        HIP_TRY(h, hipMemcpy(f.data(), L.d.f, sizeof(icrekf::Flags) * B, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < 3; ++k) conv_step[b * 3 + k] = f[b].conv_step[k];
    }
    return ALORE_NMPC_OK;
}

int alore_nmpc_ekf_device(alore_nmpc_handle h, alore_ekf_view* out)
{
    if (!h || !h->ekf.d_block || !out) return fail(h, ALORE_NMPC_E_INVALID, "ekf_device: bad argument");
    const Layout L = ekf_layout(h->ekf.d_block, h->ekf.B);
    out->x = L.d.x; out->P = L.d.P; out->est_pose = L.d.est_pose; out->est_icr = L.d.est_icr; out->status = L.d.status;
    return ALORE_NMPC_OK;
}

int alore_nmpc_ekf_closed_loop_tick(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, double now, double dt_tick, int delay_num,
                                    const double* d_noise, void* stream)
{
    if (!ekf_ready(h, B) || !h->refs.has_plant || !dev || B > h->refs.B || delay_num < 0 || !(dt_tick > 0.0))
        return fail(h, ALORE_NMPC_E_INVALID, "ekf_closed_loop_tick: bad argument (needs plant_init and ekf_init)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return ekf_tick(h, dev, B, now, dt_tick, delay_num, d_noise, stream);
}

int alore_nmpc_ekf_closed_loop_run(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, double t0, double dt_tick, int n_ticks,
                                   int delay_num, const double* d_noise, void* stream)
{
    if (!ekf_ready(h, B) || !h->refs.has_plant || !dev || B > h->refs.B || delay_num < 0 || !(dt_tick > 0.0) || n_ticks < 0)
        return fail(h, ALORE_NMPC_E_INVALID, "ekf_closed_loop_run: bad argument (needs plant_init and ekf_init)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const long first = h->ekf.ticks; // ekf_tick counts on; update number k of the run reads d_noise [k]
    for (int t = 0; t < n_ticks; ++t) {
        const size_t updates = (size_t)ltv_plan::updates_within(first, h->ekf.ticks, h->ekf.params.odom_every);
        const int rc = ekf_tick(h, dev, B, t0 + dt_tick * t, dt_tick, delay_num, d_noise ? d_noise + updates * (size_t)B * 3 : nullptr, stream);
        if (rc != ALORE_NMPC_OK) return rc;
    }
    return ALORE_NMPC_OK;
}

// internal (not in the public header): the filter of a handle, for the LTV-MPC closed loop on its estimate (ltv_mpc_capi.hip)
int alore_nmpc_internal_ekf(void* nmpc_handle, icrekf::Access* out)
{
    alore_nmpc_handle h = static_cast<alore_nmpc_handle>(nmpc_handle);
    if (!h || !h->ekf.d_block || !out) return -1;
    out->d = ekf_layout(h->ekf.d_block, h->ekf.B).d;
    out->p = ekf_params(h->ekf.params);
    out->odom_every = h->ekf.params.odom_every;
    out->ticks = &h->ekf.ticks;
    out->capacity = h->ekf.B;
    out->device = h->cfg.device;
    return 0;
}

} // extern "C"
