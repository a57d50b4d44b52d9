// ltv_mpc_capi.hip -- C ABI of the batched LTV-MPC (include/alore_ltv_mpc.h) and the kernels that sample its references
// from the trajectory store (getRefPoints / smooth_yaw of the `mpc` node, mpc_controller/src/mpc.cpp:634-690, 538-567).
// Built with default floating-point semantics: the argument checks and the heading-unwrap loops must see NaN / Inf as
// what they are (ltv_mpc.hip, the solver kernels, is built without them -- see ltv_mpc.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ltv_ekf_loop.h"
#include "ltv_host_plan.h"
#include "ltv_mpc.h"
#include "ltv_plant_device.h"
#include "minco_spline.h"
#include "nmpc_kernels.h"
#include "traj_handoff.h"

namespace ltv {

// node i of robot r, getRefPoints of the `mpc` node on the trajectory store (m: the robot's meta record, valid): the reference
// pose with the heading normalised to (-pi, pi], the reference inputs, and getRefPoints' at-goal test
struct RefNode { double X, Y, psi, v, w; };
__device__ __forceinline__ void ltv_ref_node(const nmpc::RefStore& s, const double* m, int r, int i, double dt, double now, RefNode& o, int& goal)
{
    const double duration = m[1], xv = m[2], res = m[3];
    const int np = (int)m[4], nc = (int)m[5];
    const double* dur = s.dur + (size_t)r * s.P;
    const double* coef = s.coef + (size_t)r * s.P * 12;
    const double t_cur = now - m[0];
    double temp_t = t_cur + dt;
    for (int k = 0; k < i; ++k) temp_t += dt;
    const double tq = (temp_t <= duration) ? temp_t : duration;
    int index = (int)floor(tq / res);
    if (index > nc - 1) index = nc - 1;
    if (index < 0) index = 0;
    const double floor_t = index * res, diff_t = tq - floor_t;
    double p1[2], p2[2], p3[2], v1[2], v2[2], v3[2];
    constexpr int PRE = 16; // piece durations fetched up front (independent loads), as in nmpc::ref_sample_node
    double dreg[PRE];
#pragma unroll
    for (int k = 0; k < PRE; ++k) dreg[k] = dur[min(k, np - 1)];
    minco::eval_pv_pre<PRE>(dreg, dur, coef, np, floor_t, p1, v1);
    minco::eval_pv_pre<PRE>(dreg, dur, coef, np, floor_t + diff_t / 2.0, p2, v2);
    minco::eval_pv_pre<PRE>(dreg, dur, coef, np, tq, p3, v3);
    const double* ck = s.ckpt + ((size_t)r * s.C + index) * 2;
    double xd1, yd1, xd2, yd2, xd3, yd3; // one sincos per Simpson node
    minco::xydot(p1, v1, xv, xd1, yd1); minco::xydot(p2, v2, xv, xd2, yd2); minco::xydot(p3, v3, xv, xd3, yd3);
    o.X = ck[0] + diff_t / 6.0 * (xd1 + 4.0 * xd2 + xd3);
    o.Y = ck[1] + diff_t / 6.0 * (yd1 + 4.0 * yd2 + yd3);
    double psi = p3[0];
    if (std::isfinite(psi)) { // a non-finite sample is handed on as it is: get_cmd flags the robot (status 2)
        while (psi > M_PI) psi -= 2 * M_PI;
        while (psi < -M_PI) psi += 2 * M_PI;
    }
    o.psi = psi;
    o.v = v3[1];
    o.w = v3[0];
    goal = (t_cur > duration + 1.0) ? 1 : 0;
}
// one step of smooth_yaw: `cur` moved by whole turns until it is within a quarter turn of `prev`
__device__ __forceinline__ void ltv_unwrap_step(double& cur, double prev)
{
    double dy = cur - prev;
    while (dy >= M_PI / 2) { cur -= 2 * M_PI; dy = cur - prev; }
    while (dy <= -M_PI / 2) { cur += 2 * M_PI; dy = cur - prev; }
}
// node i of robot r as the solve reads it: xref [B][T][3] with the heading `psi` (normalised or unwrapped), dref [B][T][2]
__device__ __forceinline__ void ltv_store_node(double* xref, double* dref, int T, int r, int i, const RefNode& n, double psi)
{
    double* xo = xref + ((size_t)r * T + i) * 3;
    xo[0] = n.X; xo[1] = n.Y; xo[2] = psi;
    dref[((size_t)r * T + i) * 2] = n.v;
    dref[((size_t)r * T + i) * 2 + 1] = n.w;
}

// getRefPoints of the `mpc` node on the trajectory store: thread = (robot, i), then smooth_yaw per robot
__global__ void ltv_refs_kernel(nmpc::RefStore s, int B, int T, double dt, double now, double* xref, double* dref, int* at_goal)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)B * T) return;
    const int r = (int)(t / T), i = (int)(t % T);
    const double* m = s.meta + (size_t)r * 8;
    if (m[6] == 0.0) { if (i == 0 && at_goal) at_goal[r] = 0; return; }
    RefNode n;
    int goal;
    ltv_ref_node(s, m, r, i, dt, now, n, goal);
    ltv_store_node(xref, dref, T, r, i, n, n.psi);
    if (i == 0 && at_goal) at_goal[r] = goal;
}
__global__ void ltv_unwrap_kernel(nmpc::RefStore s, int B, int T, const double* est, double* xref)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B || s.meta[(size_t)r * 8 + 6] == 0.0) return;
    double* x = xref + (size_t)r * T * 3;
    const double th = est[(size_t)r * 3 + 2];
    if (!std::isfinite(th) || !std::isfinite(x[2])) return; // an Inf heading would never leave the loops below; get_cmd flags the robot (status 2)
    // the walk in registers (the headings were read, changed and read again in memory: several dependent round trips per node)
    double prev = x[2];
    ltv_unwrap_step(prev, th);
    x[2] = prev;
    for (int i = 0; i + 1 < T; ++i) {
        double cur = x[3 * (i + 1) + 2];
        if (!std::isfinite(cur)) return;
        ltv_unwrap_step(cur, prev);
        x[3 * (i + 1) + 2] = cur;
        prev = cur;
    }
}

// ---- the closed loop on the device (alore_ltv_closed_loop_run and its pieces)
struct PreTick {
    nmpc::RefStore s;       // pre_tick_kernel only
    alore_ltv_plant_params p;
    const double* meta;     // RefStore::meta of the last sampling, or null: every robot counts as having a trajectory
    int B, T;
    double dt, now;
    double *xref, *dref;    // [B][T][3], [B][T][2]
    int* goal;              // [B] at-goal flags: in, of the sampling the last solve used; out (pre_tick_kernel), of this tick's
    double* pose;           // the plant, one slab: pose [stride][3], then vw [stride][2], then desired [stride][2]
    int stride;             // robots the slabs are laid out for (max_robots)
    const double* cmd;      // [B][2] of the last solve
    const int* status;      // [B]
    double* tr_pose;        // the trace record of the plant step, or null: pose [stride][3], then cmd [stride][2]
    int* tr_status;         // status [stride], then at_goal [stride]
    int do_plant;           // pre_tick_kernel: 0 on the first tick of a run
};

// alore_ltv_plant_step: thread = robot (plant_robot: ltv_plant_device.h)
__global__ void plant_step_kernel(PreTick a)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.B) return;
    const bool has = a.meta ? a.meta[(size_t)r * 8 + 6] != 0.0 : true;
    ltv_plant::State st;
    plant_robot(a, r, has, a.goal[r], ltv_plant::noise_off(), true, st);
}

// One launch in front of the solve of tick t: the plant step and trace record of tick t - 1, getRefPoints of tick t and smooth_yaw
// against the pose that plant step has just produced.  Wavefront = robot, lane i = node i (T <= 64).  The plant's dependent
// substeps run on every lane alike (uniform, no broadcast needed) while the sampling loads of the lane are in flight; the heading
// walk hands the unwrapped value from lane to lane by a wavefront shift, as nmpc::ref_sample_smooth_body does, instead of T
// dependent round trips through memory.  The arithmetic is that of plant_step_kernel, ltv_refs_kernel and ltv_unwrap_kernel
// (the same device functions): the same bits.
__global__ __launch_bounds__(64) void pre_tick_kernel(PreTick a)
{
    const int r = blockIdx.x, i = threadIdx.x;
    const double* m = a.s.meta + (size_t)r * 8;
    const bool has = m[6] != 0.0;
    double th;
    if (a.do_plant) {
        // the flag of tick t - 1: read and (below) overwritten by lane 0, handed to the others in registers
        const int gp = __shfl((i == 0) ? a.goal[r] : 0, 0);
        ltv_plant::State st;
        plant_robot(a, r, has, gp, ltv_plant::noise_off(), i == 0, st);
        th = st.th;
    } else {
        th = a.pose[(size_t)r * 3 + 2];
    }
    if (!has) { if (i == 0) a.goal[r] = 0; return; }
    const bool in = i < a.T;
    RefNode n{0.0, 0.0, 0.0, 0.0, 0.0};
    int goal = 0;
    if (in) ltv_ref_node(a.s, m, r, i, a.dt, a.now, n, goal);
    // smooth_yaw: node 0 against the pose, node k against the unwrapped node k - 1; the walk stops at the first heading that is
    // not finite (ltv_unwrap_kernel returns there) -- a stopped lane hands on NaN, which stops every lane after it
    double cur = n.psi, prev = th;
    for (int k = 0; k < a.T; ++k) { // wavefront-uniform
        double pass = cur;
        if (i == k) {
            if (std::isfinite(prev) && std::isfinite(cur)) { ltv_unwrap_step(cur, prev); pass = cur; }
            else pass = __builtin_nan("");
        }
        const int clo = __builtin_amdgcn_update_dpp(0, __double2loint(pass), 0x138, 0xF, 0xF, false); // wave_shr:1
        const int chi = __builtin_amdgcn_update_dpp(0, __double2hiint(pass), 0x138, 0xF, 0xF, false);
        if (i == k + 1) prev = __hiloint2double(chi, clo);
    }
    if (!in) return;
    ltv_store_node(a.xref, a.dref, a.T, r, i, n, cur);
    if (i == 0) a.goal[r] = goal;
}

} // namespace ltv

// internal accessor of the NMPC handle's trajectory store (nmpc_capi.hip)
extern "C" int alore_nmpc_internal_refstore(void* nmpc_handle, nmpc::RefStore* out, int* capacity, int* device);
// ... and of its pending trajectories (nmpc_refs_capi.hip; traj_handoff.h): every sampler of the store below has the promotion for its
// `now` in front, enqueued only while the NMPC handle has a pending start time outstanding
extern "C" int alore_nmpc_internal_promote_if_due(void* nmpc_handle, double now, void* stream);
extern "C" int alore_nmpc_internal_pending_times(void* nmpc_handle, const double** starts, size_t* n);
#define LTV_PROMOTE(h, nmpc, now, stream)                                                                              \
    do {                                                                                                               \
        if (alore_nmpc_internal_promote_if_due(nmpc, now, stream) != 0)                                                \
            return lfail(h, ALORE_LTV_E_HIP, "promotion of the pending trajectories (alore_nmpc_refs_promote) failed"); \
    } while (0)

struct alore_ltv_solver {
    alore_ltv_config cfg;
    int device = 0, B = 0;
    std::string err;
    double *d_now = nullptr, *d_xref = nullptr, *d_dref = nullptr, *d_out = nullptr, *d_buff = nullptr, *d_xopt = nullptr, *d_ws = nullptr,
           *d_est = nullptr, *d_cmd = nullptr;
    int *d_st = nullptr, *d_sweeps = nullptr, *d_status = nullptr, *d_goal = nullptr, *d_relin = nullptr;
    double* d_du = nullptr;
    long long* d_stamps = nullptr;
    char* h_stage = nullptr; // pinned
    size_t stage_bytes = 0;
    // the plant of the closed loop (alore_ltv_plant_init)
    bool plant_ready = false;
    alore_ltv_plant_params plant{};
    double* d_pose = nullptr; // one slab: pose [B][3], then vw [B][2] (d_vw), then desired [B][2] (d_des)
    double *d_vw = nullptr, *d_des = nullptr;
    const double* plant_meta = nullptr; // RefStore::meta of the last device sampling
    int trace_cap = 0;                  // ticks the ring holds
    long long trace_total = 0;          // plant steps recorded since the trace was emptied
    double* d_tr_pose = nullptr;        // per tick of the ring: pose [B][3], then cmd [B][2]
    int* d_tr_status = nullptr;         // per tick of the ring: status [B], then at_goal [B]
    // the loop on the ICR EKF's estimate (alore_ltv_ekf_closed_loop_run and its pieces, kernels in ltv_ekf_loop.hip)
    double* d_icr = nullptr;            // [B][3] the true (xv, yr, yl), for the ControlPub message
    double noise_stddev = 0.0, meas_stddev[3] = {0.0, 0.0, 0.0};
    unsigned long long noise_seed = 0;
    unsigned long long noise_event = 0; // plant + filter steps since alore_ltv_plant_set_noise / _set_state
    double* d_tr_est = nullptr;         // per tick of the ring: est [B][3]
    int* d_tr_ekf = nullptr;            // per tick of the ring: the filter's status [B]
};

namespace {
int lfail(alore_ltv_handle h, int code, const char* what, hipError_t e = hipSuccess)
{
    if (h) { h->err = what; if (e != hipSuccess) { h->err += ": "; h->err += hipGetErrorString(e); } }
    return code;
}
#define LTV_TRY(h, call)                                                  \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) return lfail(h, ALORE_LTV_E_HIP, #call, e_); \
    } while (0)
// after the carves of an entry point (ltv_plan::StageCursor over the pinned slab): one that did not fit is refused
#define LTV_STAGE(h, who, cursor)                                                                                 \
    do {                                                                                                          \
        if (!(cursor).ok()) return lfail(h, ALORE_LTV_E_INVALID, who ": the staging slab of the handle is too small"); \
    } while (0)
template <class T>
hipError_t zalloc(T** p, size_t n)
{
    hipError_t e = hipMalloc((void**)p, sizeof(T) * (n ? n : 1));
    if (e == hipSuccess) e = hipMemset(*p, 0, sizeof(T) * (n ? n : 1));
    return e;
}
void plant_free(alore_ltv_handle h)
{
    void* ptrs[] = {h->d_pose, h->d_tr_pose, h->d_tr_status, h->d_icr, h->d_tr_est, h->d_tr_ekf};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    h->d_pose = h->d_vw = h->d_des = h->d_tr_pose = h->d_icr = h->d_tr_est = nullptr;
    h->d_tr_status = h->d_tr_ekf = nullptr;
    h->plant_ready = false; h->trace_cap = 0; h->trace_total = 0; h->plant_meta = nullptr;
    h->noise_stddev = 0.0; h->meas_stddev[0] = h->meas_stddev[1] = h->meas_stddev[2] = 0.0; h->noise_seed = 0; h->noise_event = 0;
}
void lfree(alore_ltv_handle h)
{
    plant_free(h);
    void* ptrs[] = {h->d_now, h->d_xref, h->d_dref, h->d_out, h->d_buff, h->d_xopt, h->d_ws, h->d_est, h->d_st, h->d_sweeps, h->d_status, h->d_goal, h->d_cmd, h->d_relin, h->d_du};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (h->h_stage) (void)hipHostFree(h->h_stage);
}
} // namespace

extern "C" {

void alore_ltv_default_config(alore_ltv_config* c)
{
    std::memset(c, 0, sizeof(*c));
    c->dt = 0.01; c->predict_steps = 30; c->delay_num = 1;
    c->matrix_q[0] = 15.0; c->matrix_q[1] = 15.0; c->matrix_q[2] = 0.0; c->matrix_q[3] = 1.0;
    c->matrix_r[0] = 0.0; c->matrix_r[1] = 0.0;
    c->matrix_rd[0] = 1.0; c->matrix_rd[1] = 0.05;
    c->max_vel = 3.0; c->min_vel = 0.0; c->max_omega = 3.0; c->max_acc = 2.0; c->max_domega = 4.0;
    c->max_sweeps = 64;
}

int alore_ltv_create(const alore_ltv_config* cfg, int device, int max_robots, alore_ltv_handle* out)
{
    if (!cfg || !out || max_robots < 1) return ALORE_LTV_E_INVALID;
    *out = nullptr;
    if (cfg->predict_steps < 2 || cfg->predict_steps > ltv::MAXT || cfg->delay_num < 0 || cfg->delay_num >= cfg->predict_steps - 1 ||
        !(cfg->dt > 0.0) || !std::isfinite(cfg->dt))
        return ALORE_LTV_E_INVALID;
    {
        const double vals[] = {cfg->matrix_q[0], cfg->matrix_q[1], cfg->matrix_q[2], cfg->matrix_q[3], cfg->matrix_r[0], cfg->matrix_r[1],
                               cfg->matrix_rd[0], cfg->matrix_rd[1], cfg->max_vel, cfg->min_vel, cfg->max_omega, cfg->max_acc, cfg->max_domega};
        for (double v : vals)
            if (!std::isfinite(v)) return ALORE_LTV_E_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ALORE_LTV_E_NO_DEVICE;
    if (device < 0 || device >= ndev) return ALORE_LTV_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return ALORE_LTV_E_NO_DEVICE;
    alore_ltv_solver* h = new (std::nothrow) alore_ltv_solver;
    if (!h) return ALORE_LTV_E_NOMEM;
    h->cfg = *cfg;
    if (h->cfg.max_sweeps <= 0) h->cfg.max_sweeps = 64;
    h->device = device;
    h->B = max_robots;
    const size_t B = max_robots, T = cfg->predict_steps, dl = cfg->delay_num > 0 ? cfg->delay_num : 1;
    hipError_t e = hipSuccess;
    auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    A(zalloc(&h->d_now, B * 3)); A(zalloc(&h->d_xref, B * T * 3)); A(zalloc(&h->d_dref, B * T * 2)); A(zalloc(&h->d_out, B * T * 2));
    A(zalloc(&h->d_buff, B * dl * 2)); A(zalloc(&h->d_xopt, B * (T + 1) * 3)); A(zalloc(&h->d_ws, T * ltv::NF * B)); A(zalloc(&h->d_est, B * 3));
    if (std::getenv("ALORE_LTV_STAMPS")) A(zalloc(&h->d_stamps, (size_t)8));
    A(zalloc(&h->d_st, T * 2 * B)); A(zalloc(&h->d_sweeps, B)); A(zalloc(&h->d_status, B)); A(zalloc(&h->d_goal, B)); A(zalloc(&h->d_cmd, B * 2));
    A(zalloc(&h->d_relin, B)); A(zalloc(&h->d_du, B));
    h->stage_bytes = ltv_plan::stage_bytes(B, T);
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_stage, h->stage_bytes, hipHostMallocDefault);
    if (e != hipSuccess) { lfree(h); delete h; return e == hipErrorOutOfMemory ? ALORE_LTV_E_NOMEM : ALORE_LTV_E_HIP; }
    *out = h;
    return ALORE_LTV_OK;
}

int alore_ltv_destroy(alore_ltv_handle h)
{
    if (!h) return ALORE_LTV_E_INVALID;
    (void)hipSetDevice(h->device);
    if (h->d_stamps) {
        long long st[8];
        if (hipMemcpy(st, h->d_stamps, sizeof(st), hipMemcpyDeviceToHost) == hipSuccess)
            std::fprintf(stderr, "[alore_ltv stamps] robot 0, cycles: rollout %lld, backward %lld, forward %lld, rest %lld\n", st[0], st[1], st[2], st[3]);
        (void)hipFree(h->d_stamps);
    }
    lfree(h);
    delete h;
    return ALORE_LTV_OK;
}
const char* alore_ltv_last_error(alore_ltv_handle h) { return h ? h->err.c_str() : "null handle"; }

int alore_ltv_set_refs(alore_ltv_handle h, int B, const double* xref, const double* dref, void* stream)
{
    if (!h || B < 1 || B > h->B || !xref || !dref) return lfail(h, ALORE_LTV_E_INVALID, "set_refs: bad argument");
    LTV_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t T = h->cfg.predict_steps;
    ltv_plan::StageCursor stage(h->h_stage, h->stage_bytes);
    double* hx = stage.take<double>((size_t)B * T * 3);
    double* hd = stage.take<double>((size_t)B * T * 2);
    LTV_STAGE(h, "set_refs", stage);
    std::memcpy(hx, xref, sizeof(double) * B * T * 3);
    std::memcpy(hd, dref, sizeof(double) * B * T * 2);
    LTV_TRY(h, hipMemcpyAsync(h->d_xref, hx, sizeof(double) * B * T * 3, hipMemcpyHostToDevice, s));
    LTV_TRY(h, hipMemcpyAsync(h->d_dref, hd, sizeof(double) * B * T * 2, hipMemcpyHostToDevice, s));
    LTV_TRY(h, hipStreamSynchronize(s)); // the slab is reused
    return ALORE_LTV_OK;
}

int alore_ltv_refs_from_store(alore_ltv_handle h, void* nmpc, int B, double now, const double* est, int* at_goal, void* stream)
{
    if (!h || !nmpc || B < 1 || B > h->B || !est || !std::isfinite(now)) return lfail(h, ALORE_LTV_E_INVALID, "refs_from_store: bad argument");
    nmpc::RefStore rs;
    int cap = 0, dev = -1;
    if (alore_nmpc_internal_refstore(nmpc, &rs, &cap, &dev) != 0 || cap < B || dev != h->device)
        return lfail(h, ALORE_LTV_E_INVALID, "refs_from_store: the NMPC handle has no trajectory store for B robots on this device");
    LTV_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int T = h->cfg.predict_steps;
    ltv_plan::StageCursor stage(h->h_stage, h->stage_bytes);
    double* he = stage.take<double>((size_t)B * 3);
    LTV_STAGE(h, "refs_from_store", stage);
    std::memcpy(he, est, sizeof(double) * B * 3);
    LTV_TRY(h, hipMemcpyAsync(h->d_est, he, sizeof(double) * B * 3, hipMemcpyHostToDevice, s));
    LTV_PROMOTE(h, nmpc, now, stream);
    const long total = (long)B * T;
    hipLaunchKernelGGL(ltv::ltv_refs_kernel, dim3((unsigned)((total + 127) / 128)), dim3(128), 0, s, rs, B, T, h->cfg.dt, now, h->d_xref, h->d_dref,
                       h->d_goal);
    hipLaunchKernelGGL(ltv::ltv_unwrap_kernel, dim3((B + 63) / 64), dim3(64), 0, s, rs, B, T, h->d_est, h->d_xref);
    LTV_TRY(h, hipGetLastError());
    if (at_goal) LTV_TRY(h, hipMemcpyAsync(at_goal, h->d_goal, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    LTV_TRY(h, hipStreamSynchronize(s));
    return ALORE_LTV_OK;
}

// What every solve launch takes of the handle.  now: the states [B][3] as the device reads them.  du_th < 0: the fixed count of
// n_relin passes; else the converged build (n_relin is its cap), which is always the lanes kernel.
static ltv::DevConv solve_args(alore_ltv_handle h, int B, const double* now, int n_relin, double du_th, int reset)
{
    ltv::DevConv d{};
    d.c = h->cfg; d.B = B; d.stride = h->B;
    d.now = now;
    d.xref = h->d_xref; d.dref = h->d_dref; d.output = h->d_out; d.buff = h->d_buff; d.xopt = h->d_xopt;
    d.ws = h->d_ws; d.st = h->d_st; d.sweeps = h->d_sweeps; d.status = h->d_status; d.cmd = h->d_cmd;
    d.n_relin = n_relin; d.reset = reset;
    d.stamps = h->d_stamps;
    if (du_th < 0.0) return d;
    d.du_th = std::isinf(du_th) ? 1.7976931348623157e308 : du_th; // "always met": the kernel compares finite numbers only
    d.relin_iters = h->d_relin; d.du = h->d_du;
    return d;
}
static hipError_t launch_solve(const ltv::DevConv& d, double du_th, bool thread_kernel, hipStream_t s)
{
    return du_th < 0.0 ? ltv::launch_get_cmd(d, thread_kernel, s) : ltv::launch_get_cmd_converge(d, s);
}

// the host regions of the pinned slab that the kernel of a tick writes straight into (device alias of the host pointer), behind
// the states: commands [B][2], status [B], pass counts [B]
struct TickOut { double* cmd; int *status, *iters; };

// a solve on host states (du_th: see solve_args); tick: the kernel also writes what a tick returns into the slab
static int ltv_enqueue(alore_ltv_handle h, int B, const double* now_state, int n_relin, double du_th, int reset, hipStream_t s, TickOut* tick = nullptr)
{
    ltv_plan::StageCursor stage(h->h_stage, h->stage_bytes);
    double* hn = stage.take<double>((size_t)B * 3);
    if (tick) { tick->cmd = stage.take<double>((size_t)B * 2); tick->status = stage.take<int>(B); tick->iters = stage.take<int>(B); }
    LTV_STAGE(h, "solve", stage);
    std::memcpy(hn, now_state, sizeof(double) * B * 3);
    // 16 lanes per robot (stages in registers, sweeps lane by lane) unless ALORE_LTV_KERNEL=thread asks for the
    // one-thread-per-robot kernel (diagnostic A/B)
    static const char* which = std::getenv("ALORE_LTV_KERNEL");
    const bool thread_kernel = du_th < 0.0 && which && which[0] == 't';
    void* dn = h->d_now;
    if (tick && !thread_kernel) // tick path: the lanes kernel reads the states once, straight from the pinned slab
        LTV_TRY(h, hipHostGetDevicePointer(&dn, hn, 0));
    else
        LTV_TRY(h, hipMemcpyAsync(h->d_now, hn, sizeof(double) * B * 3, hipMemcpyHostToDevice, s));
    ltv::DevConv d = solve_args(h, B, (const double*)dn, n_relin, du_th, reset);
    if (tick) {
        LTV_TRY(h, hipHostGetDevicePointer((void**)&d.cmd_host, tick->cmd, 0));
        LTV_TRY(h, hipHostGetDevicePointer((void**)&d.status_host, tick->status, 0));
        if (du_th >= 0.0) LTV_TRY(h, hipHostGetDevicePointer((void**)&d.iters_host, tick->iters, 0));
    }
    LTV_TRY(h, launch_solve(d, du_th, thread_kernel, s));
    return ALORE_LTV_OK;
}

int alore_ltv_get_cmd(alore_ltv_handle h, int B, const double* now_state, int n_relin, int reset, void* stream)
{
    if (!h || B < 1 || B > h->B || !now_state || n_relin < 1) return lfail(h, ALORE_LTV_E_INVALID, "get_cmd: bad argument");
    LTV_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int rc = ltv_enqueue(h, B, now_state, n_relin, -1.0, reset, s);
    if (rc != ALORE_LTV_OK) return rc;
    LTV_TRY(h, hipStreamSynchronize(s)); // the staging slab is reused by the next call
    return ALORE_LTV_OK;
}

// one control tick: states in, getCmd, commands (and status) out -- one upload, one launch, one download, one wait
int alore_ltv_tick(alore_ltv_handle h, int B, const double* now_state, int n_relin, int reset, double* cmd, int* status, void* stream)
{
    if (!h || B < 1 || B > h->B || !now_state || n_relin < 1 || !cmd) return lfail(h, ALORE_LTV_E_INVALID, "tick: bad argument");
    LTV_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    // the kernel writes the 20 bytes per robot a tick returns straight into the pinned slab: two copy commands and their
    // completion signals less on the critical path of the tick
    TickOut t;
    const int rc = ltv_enqueue(h, B, now_state, n_relin, -1.0, reset, s, &t);
    if (rc != ALORE_LTV_OK) return rc;
    LTV_TRY(h, hipStreamSynchronize(s));
    std::memcpy(cmd, t.cmd, sizeof(double) * B * 2);
    if (status) std::memcpy(status, t.status, sizeof(int) * B);
    return ALORE_LTV_OK;
}

// The stopping rule's arguments.  Here, not in the kernel: ltv_mpc.hip is built without NaN / Inf semantics.
static const char* converge_args_bad(int max_relin, double du_th)
{
    if (max_relin < 1) return "max_relin must be at least 1";
    if (std::isnan(du_th)) return "du_th is NaN";
    if (du_th < 0.0) return "du_th must not be negative";
    return nullptr;
}

int alore_ltv_get_cmd_converge(alore_ltv_handle h, int B, const double* now_state, int max_relin, double du_th, int reset, void* stream)
{
    if (!h || B < 1 || B > h->B || !now_state) return lfail(h, ALORE_LTV_E_INVALID, "get_cmd_converge: bad argument");
    if (const char* why = converge_args_bad(max_relin, du_th)) return lfail(h, ALORE_LTV_E_INVALID, (std::string("get_cmd_converge: ") + why).c_str());
    LTV_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int rc = ltv_enqueue(h, B, now_state, max_relin, du_th, reset, s);
    if (rc != ALORE_LTV_OK) return rc;
    LTV_TRY(h, hipStreamSynchronize(s)); // the staging slab is reused by the next call
    return ALORE_LTV_OK;
}

int alore_ltv_tick_converge(alore_ltv_handle h, int B, const double* now_state, int max_relin, double du_th, int reset, double* cmd, int* status,
                            int* relin_iters, void* stream)
{
    if (!h || B < 1 || B > h->B || !now_state || !cmd) return lfail(h, ALORE_LTV_E_INVALID, "tick_converge: bad argument");
    if (const char* why = converge_args_bad(max_relin, du_th)) return lfail(h, ALORE_LTV_E_INVALID, (std::string("tick_converge: ") + why).c_str());
    LTV_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    TickOut t; // as alore_ltv_tick, and the pass counts
    const int rc = ltv_enqueue(h, B, now_state, max_relin, du_th, reset, s, &t);
    if (rc != ALORE_LTV_OK) return rc;
    LTV_TRY(h, hipStreamSynchronize(s));
    std::memcpy(cmd, t.cmd, sizeof(double) * B * 2);
    if (status) std::memcpy(status, t.status, sizeof(int) * B);
    if (relin_iters) std::memcpy(relin_iters, t.iters, sizeof(int) * B);
    return ALORE_LTV_OK;
}

int alore_ltv_relin_info(alore_ltv_handle h, int B, int* relin_iters, double* du, void* stream)
{
    if (!h || B < 1 || B > h->B) return lfail(h, ALORE_LTV_E_INVALID, "relin_info: bad argument");
    LTV_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    ltv_plan::StageCursor stage(h->h_stage, h->stage_bytes);
    double* sd = stage.take<double>(B);
    int* si = stage.take<int>(B);
    LTV_STAGE(h, "relin_info", stage);
    if (du) LTV_TRY(h, hipMemcpyAsync(sd, h->d_du, sizeof(double) * B, hipMemcpyDeviceToHost, s));
    if (relin_iters) LTV_TRY(h, hipMemcpyAsync(si, h->d_relin, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    LTV_TRY(h, hipStreamSynchronize(s));
    if (du) std::memcpy(du, sd, sizeof(double) * B);
    if (relin_iters) std::memcpy(relin_iters, si, sizeof(int) * B);
    return ALORE_LTV_OK;
}

int alore_ltv_results(alore_ltv_handle h, int B, double* output, double* xopt, int* sweeps, int* status, void* stream)
{
    if (!h || B < 1 || B > h->B) return lfail(h, ALORE_LTV_E_INVALID, "results: bad argument");
    LTV_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t T = h->cfg.predict_steps;
    // through the pinned slab of the handle (a device-to-pageable copy is staged by the runtime in small pieces with a host
    // wait per piece): layout  output | xopt | sweeps | status
    ltv_plan::StageCursor stage(h->h_stage, h->stage_bytes);
    double* so = stage.take<double>((size_t)B * T * 2);
    double* sx = stage.take<double>((size_t)B * (T + 1) * 3);
    int* ss = stage.take<int>(B);
    int* st = stage.take<int>(B);
    LTV_STAGE(h, "results", stage);
    if (output) LTV_TRY(h, hipMemcpyAsync(so, h->d_out, sizeof(double) * B * T * 2, hipMemcpyDeviceToHost, s));
    if (xopt) LTV_TRY(h, hipMemcpyAsync(sx, h->d_xopt, sizeof(double) * B * (T + 1) * 3, hipMemcpyDeviceToHost, s));
    if (sweeps) LTV_TRY(h, hipMemcpyAsync(ss, h->d_sweeps, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    if (status) LTV_TRY(h, hipMemcpyAsync(st, h->d_status, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    LTV_TRY(h, hipStreamSynchronize(s));
    if (output) std::memcpy(output, so, sizeof(double) * B * T * 2);
    if (xopt) std::memcpy(xopt, sx, sizeof(double) * B * (T + 1) * 3);
    if (sweeps) std::memcpy(sweeps, ss, sizeof(int) * B);
    if (status) std::memcpy(status, st, sizeof(int) * B);
    return ALORE_LTV_OK;
}

int alore_ltv_commands(alore_ltv_handle h, int B, double* cmd, int* status, void* stream)
{
    if (!h || B < 1 || B > h->B || !cmd) return lfail(h, ALORE_LTV_E_INVALID, "commands: bad argument");
    LTV_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    ltv_plan::StageCursor stage(h->h_stage, h->stage_bytes);
    double* sc = stage.take<double>((size_t)B * 2);
    int* st = stage.take<int>(B);
    LTV_STAGE(h, "commands", stage);
    // column delay_num of every robot's output, packed by the kernel (16 bytes per robot)
    LTV_TRY(h, hipMemcpyAsync(sc, h->d_cmd, sizeof(double) * B * 2, hipMemcpyDeviceToHost, s));
    if (status) LTV_TRY(h, hipMemcpyAsync(st, h->d_status, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    LTV_TRY(h, hipStreamSynchronize(s));
    std::memcpy(cmd, sc, sizeof(double) * B * 2);
    if (status) std::memcpy(status, st, sizeof(int) * B);
    return ALORE_LTV_OK;
}

int alore_ltv_set_state(alore_ltv_handle h, int B, const double* output, const double* buff, void* stream)
{
    if (!h || B < 1 || B > h->B) return lfail(h, ALORE_LTV_E_INVALID, "set_state: bad argument");
    LTV_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t T = h->cfg.predict_steps, dl = h->cfg.delay_num;
    if (output) LTV_TRY(h, hipMemcpyAsync(h->d_out, output, sizeof(double) * B * T * 2, hipMemcpyHostToDevice, s));
    if (buff && dl > 0) LTV_TRY(h, hipMemcpyAsync(h->d_buff, buff, sizeof(double) * B * dl * 2, hipMemcpyHostToDevice, s));
    LTV_TRY(h, hipStreamSynchronize(s));
    return ALORE_LTV_OK;
}

// ---- the closed loop on the device

void alore_ltv_plant_default_params(alore_ltv_plant_params* p)
{
    std::memset(p, 0, sizeof(*p));
    p->max_acc = 2.0; p->max_domega = 4.0; p->pose_pub_period = 0.01; p->state_propa_period = 0.002;
    p->substeps = 5; p->follow = 0;
}

int alore_ltv_plant_init(alore_ltv_handle h, const alore_ltv_plant_params* p, int max_trace_ticks)
{
    if (!h) return ALORE_LTV_E_INVALID;
    if (!p || max_trace_ticks < 0) return lfail(h, ALORE_LTV_E_INVALID, "plant_init: bad argument");
    if (!ltv_plant::valid(*p)) return lfail(h, ALORE_LTV_E_INVALID, "plant_init: the plant parameters must be finite and positive, substeps at least 1");
    LTV_TRY(h, hipSetDevice(h->device));
    LTV_TRY(h, hipDeviceSynchronize()); // a run still in flight reads what is freed below
    plant_free(h);
    const size_t B = h->B, M = max_trace_ticks;
    hipError_t e = hipSuccess;
    auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    A(zalloc(&h->d_pose, B * 7));
    if (M > 0) { A(zalloc(&h->d_tr_pose, M * B * 5)); A(zalloc(&h->d_tr_status, M * B * 2)); }
    A(zalloc(&h->d_icr, B * 3));
    if (M > 0) { A(zalloc(&h->d_tr_est, M * B * 3)); A(zalloc(&h->d_tr_ekf, M * B)); }
    if (e == hipSuccess) { // the true ICR of planner_sim.launch:41-43 as (xv, yr, yl)
        std::vector<double> icr(B * 3);
        for (size_t b = 0; b < B; ++b) { icr[b * 3] = 0.2; icr[b * 3 + 1] = -0.3; icr[b * 3 + 2] = 0.3; }
        e = hipMemcpy(h->d_icr, icr.data(), sizeof(double) * B * 3, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) { h->d_vw = h->d_pose + B * 3; h->d_des = h->d_pose + B * 5; }
    if (e != hipSuccess) { plant_free(h); return lfail(h, e == hipErrorOutOfMemory ? ALORE_LTV_E_NOMEM : ALORE_LTV_E_HIP, "plant_init: allocation", e); }
    h->plant = *p;
    h->plant.follow = p->follow ? 1 : 0;
    h->trace_cap = max_trace_ticks;
    h->plant_ready = true;
    return ALORE_LTV_OK;
}

// the checks every device call starts with; null: fine
static const char* plant_args_bad(alore_ltv_handle h, int B)
{
    if (!h->plant_ready) return "alore_ltv_plant_init has not been called";
    if (B < 1 || B > h->B) return "B out of range";
    return nullptr;
}
static const char* store_bad(alore_ltv_handle h, void* nmpc, int B, nmpc::RefStore* rs)
{
    int cap = 0, dev = -1;
    if (!nmpc || alore_nmpc_internal_refstore(nmpc, rs, &cap, &dev) != 0 || cap < B || dev != h->device)
        return "the NMPC handle has no trajectory store for B robots on this device";
    return nullptr;
}
// n_relin / du_th of the device solve (du_th < 0: the fixed count)
static const char* solve_args_bad(int n_relin, double du_th)
{
    if (n_relin < 1) return "n_relin must be at least 1";
    if (std::isnan(du_th)) return "du_th is NaN";
    return nullptr;
}
// n_ticks, t0, dt_tick and the solve's arguments of a run; dt_positive: dt_tick is the filter's step too
static const char* run_args_bad(int n_ticks, double t0, double dt_tick, bool dt_positive, int n_relin, double du_th)
{
    if (n_ticks < 1) return "n_ticks must be at least 1";
    const bool finite = std::isfinite(t0) && std::isfinite(dt_tick);
    if (!dt_positive && !finite) return "t0 and dt_tick must be finite";
    if (dt_positive && (!finite || !(dt_tick > 0.0))) return "t0 must be finite, dt_tick finite and positive";
    return solve_args_bad(n_relin, du_th);
}
#define LTV_ARGS(h, who, expr)                                                                          \
    do {                                                                                                \
        if (const char* why_ = (expr)) return lfail(h, ALORE_LTV_E_INVALID, (std::string(who ": ") + why_).c_str()); \
    } while (0)

int alore_ltv_plant_set_state(alore_ltv_handle h, int B, const double* pose, const double* vw, const double* desired, void* stream)
{
    if (!h) return ALORE_LTV_E_INVALID;
    LTV_ARGS(h, "plant_set_state", plant_args_bad(h, B));
    if (!pose) return lfail(h, ALORE_LTV_E_INVALID, "plant_set_state: pose is null");
    LTV_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    ltv_plan::StageCursor stage(h->h_stage, h->stage_bytes);
    double* sp = stage.take<double>((size_t)B * 3);
    double* sv = stage.take<double>((size_t)B * 2);
    double* sd = stage.take<double>((size_t)B * 2);
    LTV_STAGE(h, "plant_set_state", stage);
    std::memcpy(sp, pose, sizeof(double) * B * 3);
    if (vw) std::memcpy(sv, vw, sizeof(double) * B * 2); else std::memset(sv, 0, sizeof(double) * B * 2);
    if (desired) std::memcpy(sd, desired, sizeof(double) * B * 2); else std::memset(sd, 0, sizeof(double) * B * 2);
    LTV_TRY(h, hipMemcpyAsync(h->d_pose, sp, sizeof(double) * B * 3, hipMemcpyHostToDevice, s));
    LTV_TRY(h, hipMemcpyAsync(h->d_vw, sv, sizeof(double) * B * 2, hipMemcpyHostToDevice, s));
    LTV_TRY(h, hipMemcpyAsync(h->d_des, sd, sizeof(double) * B * 2, hipMemcpyHostToDevice, s));
    LTV_TRY(h, hipStreamSynchronize(s)); // the slab is reused
    h->trace_total = 0;
    h->noise_event = 0;
    return ALORE_LTV_OK;
}

int alore_ltv_plant_stop(alore_ltv_handle h, int B, const int* d_mask, int mask_stride_bytes, void* stream)
{
    if (!h) return ALORE_LTV_E_INVALID;
    LTV_ARGS(h, "plant_stop", plant_args_bad(h, B));
    if (d_mask && (mask_stride_bytes < (int)sizeof(int) || mask_stride_bytes % (int)sizeof(int)))
        return lfail(h, ALORE_LTV_E_INVALID, "plant_stop: the mask stride must be a positive multiple of sizeof(int)");
    LTV_TRY(h, hipSetDevice(h->device));
    LTV_TRY(h, nmpc::launch_plant_stop(h->d_vw, h->d_des, 2, d_mask, d_mask ? mask_stride_bytes : 0, B, (hipStream_t)stream));
    return ALORE_LTV_OK;
}

int alore_ltv_plant_get_state(alore_ltv_handle h, int B, double* pose, double* vw, int* at_goal, void* stream)
{
    if (!h) return ALORE_LTV_E_INVALID;
    LTV_ARGS(h, "plant_get_state", plant_args_bad(h, B));
    LTV_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    ltv_plan::StageCursor stage(h->h_stage, h->stage_bytes);
    double* sp = stage.take<double>((size_t)B * 3);
    double* sv = stage.take<double>((size_t)B * 2);
    int* sg = stage.take<int>(B);
    LTV_STAGE(h, "plant_get_state", stage);
    if (pose) LTV_TRY(h, hipMemcpyAsync(sp, h->d_pose, sizeof(double) * B * 3, hipMemcpyDeviceToHost, s));
    if (vw) LTV_TRY(h, hipMemcpyAsync(sv, h->d_vw, sizeof(double) * B * 2, hipMemcpyDeviceToHost, s));
    if (at_goal) LTV_TRY(h, hipMemcpyAsync(sg, h->d_goal, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    LTV_TRY(h, hipStreamSynchronize(s));
    if (pose) std::memcpy(pose, sp, sizeof(double) * B * 3);
    if (vw) std::memcpy(vw, sv, sizeof(double) * B * 2);
    if (at_goal) std::memcpy(at_goal, sg, sizeof(int) * B);
    return ALORE_LTV_OK;
}

int alore_ltv_plant_device(alore_ltv_handle h, alore_ltv_plant_view* out)
{
    if (!h) return ALORE_LTV_E_INVALID;
    if (!out) return lfail(h, ALORE_LTV_E_INVALID, "plant_device: bad argument");
    if (!h->plant_ready) return lfail(h, ALORE_LTV_E_INVALID, "plant_device: alore_ltv_plant_init has not been called");
    out->pose = h->d_pose; out->vw = h->d_vw; out->cmd = h->d_cmd; out->at_goal = h->d_goal; out->status = h->d_status;
    return ALORE_LTV_OK;
}

namespace {
// what the kernels of a tick take; record: this launch does a plant step, which takes the next slot of the trace ring (*slot: that
// slot, -1 where nothing is recorded)
ltv::PreTick tick_args(alore_ltv_handle h, int B, bool record, long long* slot = nullptr)
{
    ltv::PreTick a{};
    a.p = h->plant; a.meta = h->plant_meta; a.B = B; a.T = h->cfg.predict_steps; a.dt = h->cfg.dt;
    a.xref = h->d_xref; a.dref = h->d_dref; a.goal = h->d_goal;
    a.pose = h->d_pose; a.stride = h->B; a.cmd = h->d_cmd; a.status = h->d_status;
    const long long at = record ? ltv_plan::ring_next_slot(h->trace_total, h->trace_cap) : -1;
    if (at >= 0) {
        const size_t row = (size_t)at * h->B; // a record is laid out for max_robots robots
        a.tr_pose = h->d_tr_pose + row * 5; a.tr_status = h->d_tr_status + row * 2;
    }
    if (record) ++h->trace_total;
    if (slot) *slot = at;
    return a;
}
// the enqueue of each piece; the arguments have been checked
hipError_t enq_refs(alore_ltv_handle h, const nmpc::RefStore& rs, int B, double now, hipStream_t s)
{
    const int T = h->cfg.predict_steps;
    const long total = (long)B * T;
    hipLaunchKernelGGL(ltv::ltv_refs_kernel, dim3((unsigned)((total + 127) / 128)), dim3(128), 0, s, rs, B, T, h->cfg.dt, now, h->d_xref, h->d_dref,
                       h->d_goal);
    hipLaunchKernelGGL(ltv::ltv_unwrap_kernel, dim3((B + 63) / 64), dim3(64), 0, s, rs, B, T, h->d_pose, h->d_xref);
    h->plant_meta = rs.meta;
    return hipGetLastError();
}
hipError_t enq_pre_tick(alore_ltv_handle h, const nmpc::RefStore& rs, int B, double now, bool do_plant, hipStream_t s)
{
    h->plant_meta = rs.meta;
    ltv::PreTick a = tick_args(h, B, do_plant);
    a.s = rs; a.now = now; a.do_plant = do_plant ? 1 : 0;
    hipLaunchKernelGGL(ltv::pre_tick_kernel, dim3(B), dim3(64), 0, s, a);
    return hipGetLastError();
}
// now: the states [B][3] the solve starts from, on the device; null: the plant's pose
hipError_t enq_solve(alore_ltv_handle h, int B, int n_relin, double du_th, int reset, hipStream_t s, const double* now = nullptr)
{
    return launch_solve(solve_args(h, B, now ? now : h->d_pose, n_relin, du_th, reset), du_th, false, s);
}
hipError_t enq_plant(alore_ltv_handle h, int B, hipStream_t s)
{
    const ltv::PreTick a = tick_args(h, B, true);
    hipLaunchKernelGGL(ltv::plant_step_kernel, dim3((B + 63) / 64), dim3(64), 0, s, a);
    return hipGetLastError();
}
// ---- the pieces of the loop on the ICR EKF's estimate
// getRefPoints + smooth_yaw against est_pose: pre_tick_kernel without its plant step reads nothing of `pose` but the heading
hipError_t enq_refs_est(alore_ltv_handle h, const nmpc::RefStore& rs, int B, double now, const double* est_pose, hipStream_t s)
{
    h->plant_meta = rs.meta;
    ltv::PreTick a = tick_args(h, B, false);
    a.s = rs; a.now = now; a.do_plant = 0;
    a.pose = const_cast<double*>(est_pose);
    hipLaunchKernelGGL(ltv::pre_tick_kernel, dim3(B), dim3(64), 0, s, a);
    return hipGetLastError();
}
// plant on the true state, ControlPub, filter step, trace record (ltv::plant_ekf_kernel); takes the next slot of the trace ring,
// the next noise event and the next tick of the filter's count
hipError_t enq_plant_ekf(alore_ltv_handle h, void* nmpc, const ltv::EkfInfo& ei, int B, double dt_tick, hipStream_t s)
{
    long long slot = -1;
    const ltv::PreTick t = tick_args(h, B, true, &slot);
    ltv::PlantEkf a{};
    a.p = h->plant; a.meta = h->plant_meta; a.B = B; a.stride = h->B;
    a.goal = h->d_goal; a.pose = h->d_pose; a.cmd = h->d_cmd; a.status = h->d_status; a.icr = h->d_icr;
    a.tr_pose = t.tr_pose; a.tr_status = t.tr_status;
    if (slot >= 0) {
        const size_t row = (size_t)slot * h->B;
        a.tr_est = h->d_tr_est + row * 3; a.tr_ekf_status = h->d_tr_ekf + row;
    }
    a.dt = dt_tick;
    *ei.ticks += 1;
    a.do_update = ltv_plan::is_update_tick(*ei.ticks, ei.odom_every) ? 1 : 0;
    a.noise_stddev = h->noise_stddev;
    for (int i = 0; i < 3; ++i) a.meas_stddev[i] = h->meas_stddev[i];
    a.seed = h->noise_seed; a.event = h->noise_event++;
    return ltv::launch_plant_ekf(a, nmpc, s);
}
} // namespace

int alore_ltv_refs_from_store_device(alore_ltv_handle h, void* nmpc, int B, double now, void* stream)
{
    if (!h) return ALORE_LTV_E_INVALID;
    nmpc::RefStore rs;
    LTV_ARGS(h, "refs_from_store_device", plant_args_bad(h, B));
    if (!std::isfinite(now)) return lfail(h, ALORE_LTV_E_INVALID, "refs_from_store_device: now is not finite");
    LTV_ARGS(h, "refs_from_store_device", store_bad(h, nmpc, B, &rs));
    LTV_TRY(h, hipSetDevice(h->device));
    LTV_PROMOTE(h, nmpc, now, stream);
    LTV_TRY(h, enq_refs(h, rs, B, now, (hipStream_t)stream));
    return ALORE_LTV_OK;
}

int alore_ltv_get_cmd_device(alore_ltv_handle h, int B, int n_relin, double du_th, int reset, void* stream)
{
    if (!h) return ALORE_LTV_E_INVALID;
    LTV_ARGS(h, "get_cmd_device", plant_args_bad(h, B));
    LTV_ARGS(h, "get_cmd_device", solve_args_bad(n_relin, du_th));
    LTV_TRY(h, hipSetDevice(h->device));
    LTV_TRY(h, enq_solve(h, B, n_relin, du_th, reset ? 1 : 0, (hipStream_t)stream));
    return ALORE_LTV_OK;
}

int alore_ltv_plant_step(alore_ltv_handle h, int B, void* stream)
{
    if (!h) return ALORE_LTV_E_INVALID;
    LTV_ARGS(h, "plant_step", plant_args_bad(h, B));
    LTV_TRY(h, hipSetDevice(h->device));
    LTV_TRY(h, enq_plant(h, B, (hipStream_t)stream));
    return ALORE_LTV_OK;
}

int alore_ltv_closed_loop_run(alore_ltv_handle h, void* nmpc, int B, double t0, double dt_tick, int n_ticks, int n_relin, double du_th, int reset,
                              void* stream)
{
    if (!h) return ALORE_LTV_E_INVALID;
    nmpc::RefStore rs;
    LTV_ARGS(h, "closed_loop_run", plant_args_bad(h, B));
    LTV_ARGS(h, "closed_loop_run", run_args_bad(n_ticks, t0, dt_tick, false, n_relin, du_th));
    LTV_ARGS(h, "closed_loop_run", store_bad(h, nmpc, B, &rs));
    LTV_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const char* env = std::getenv("ALORE_LTV_CLOSED_LOOP_SERIAL");
    const bool serial = env && env[0] == '1';
    // pre_tick_kernel does the plant step of tick k - 1 and the sampling of tick k in one launch, and the plant step reads the store's
    // meta rows: where a pending trajectory becomes due the run is cut (traj_handoff.h: split_run), the part in front ends with its own
    // plant step like a complete run, and the promotion goes between the parts.  No pending start time outstanding: one part.
    const double* starts = nullptr;
    size_t n_starts = 0;
    (void)alore_nmpc_internal_pending_times(nmpc, &starts, &n_starts);
    const std::vector<double> pend(starts, starts + n_starts); // the promotions below shorten the handle's own list
    for (const traj_handoff::Segment& g : traj_handoff::split_run(t0, dt_tick, n_ticks, pend.data(), pend.size())) {
        if (g.promote) LTV_PROMOTE(h, nmpc, traj_handoff::tick_time(t0, dt_tick, g.first), stream);
        for (int k = g.first; k < g.first + g.count; ++k) {
            const double now = t0 + k * dt_tick;
            const int rst = (k == 0 && reset) ? 1 : 0;
            if (serial) {
                LTV_TRY(h, enq_refs(h, rs, B, now, s));
                LTV_TRY(h, enq_solve(h, B, n_relin, du_th, rst, s));
                LTV_TRY(h, enq_plant(h, B, s));
            } else {
                LTV_TRY(h, enq_pre_tick(h, rs, B, now, k > g.first, s));
                LTV_TRY(h, enq_solve(h, B, n_relin, du_th, rst, s));
            }
        }
        if (!serial) LTV_TRY(h, enq_plant(h, B, s));
    }
    return ALORE_LTV_OK;
}

// One column of the trace ring.  host: [ticks][B][width], or null (not asked for); dev: slot 0 of the array the column lies in,
// whose slots are `pitch` elements apart (laid out for max_robots robots); the column starts `first` elements into a slot.
struct TraceCol { void* host; const void* dev; size_t elem, first, width, pitch; };
// the newest min(recorded, capacity, max_ticks) ticks of the columns, oldest first (ltv_plan::ring_newest: one or two runs of slots)
static int get_trace_cols(alore_ltv_handle h, int B, int max_ticks, const TraceCol* cols, int n_cols, int* n_ticks_out, hipStream_t s)
{
    const ltv_plan::RingRuns runs = ltv_plan::ring_newest(h->trace_total, h->trace_cap, max_ticks);
    *n_ticks_out = (int)runs.count;
    size_t done = 0;
    for (int k = 0; k < runs.n; ++k) {
        const size_t slot = (size_t)runs.run[k].slot, rows = (size_t)runs.run[k].rows;
        for (int c = 0; c < n_cols; ++c) {
            const TraceCol& t = cols[c];
            if (!t.host) continue;
            const size_t row = t.elem * B * t.width;
            LTV_TRY(h, hipMemcpy2DAsync((char*)t.host + done * row, row, (const char*)t.dev + (slot * t.pitch + t.first) * t.elem, t.pitch * t.elem, row,
                                        rows, hipMemcpyDeviceToHost, s));
        }
        done += rows;
    }
    LTV_TRY(h, hipStreamSynchronize(s));
    return ALORE_LTV_OK;
}

int alore_ltv_plant_get_trace(alore_ltv_handle h, int B, int max_ticks, double* pose, double* cmd, int* status, int* at_goal, int* n_ticks_out,
                              void* stream)
{
    if (!h) return ALORE_LTV_E_INVALID;
    LTV_ARGS(h, "plant_get_trace", plant_args_bad(h, B));
    if (max_ticks < 0 || !n_ticks_out) return lfail(h, ALORE_LTV_E_INVALID, "plant_get_trace: bad argument");
    LTV_TRY(h, hipSetDevice(h->device));
    const size_t HB = h->B;
    const TraceCol cols[] = {{pose, h->d_tr_pose, sizeof(double), 0, 3, HB * 5}, {cmd, h->d_tr_pose, sizeof(double), HB * 3, 2, HB * 5},
                             {status, h->d_tr_status, sizeof(int), 0, 1, HB * 2}, {at_goal, h->d_tr_status, sizeof(int), HB, 1, HB * 2}};
    return get_trace_cols(h, B, max_ticks, cols, 4, n_ticks_out, (hipStream_t)stream);
}

// ---- the closed loop on the ICR EKF's estimate

// the filter of the NMPC handle: there, large enough, on this device; null: fine
static const char* ekf_bad(alore_ltv_handle h, void* nmpc, int B, ltv::EkfInfo* ei)
{
    if (!ltv::ekf_info(nmpc, ei)) return "no NMPC handle on which alore_nmpc_ekf_init has been called";
    if (ei->capacity < B || ei->device != h->device) return "the NMPC handle's filter is too small for B robots or on another device";
    return nullptr;
}

int alore_ltv_plant_set_icr(alore_ltv_handle h, int B, const double* icr, void* stream)
{
    if (!h) return ALORE_LTV_E_INVALID;
    LTV_ARGS(h, "plant_set_icr", plant_args_bad(h, B));
    if (!icr) return lfail(h, ALORE_LTV_E_INVALID, "plant_set_icr: icr is null");
    for (int b = 0; b < B; ++b) {
        const double* c = icr + (size_t)b * 3;
        if (!std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2]) || c[1] == c[2])
            return lfail(h, ALORE_LTV_E_INVALID, "plant_set_icr: every (xv, yr, yl) must be finite with yl != yr");
    }
    LTV_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    ltv_plan::StageCursor stage(h->h_stage, h->stage_bytes);
    double* sp = stage.take<double>((size_t)B * 3);
    LTV_STAGE(h, "plant_set_icr", stage);
    std::memcpy(sp, icr, sizeof(double) * B * 3);
    LTV_TRY(h, hipMemcpyAsync(h->d_icr, sp, sizeof(double) * B * 3, hipMemcpyHostToDevice, s));
    LTV_TRY(h, hipStreamSynchronize(s)); // the slab is reused
    return ALORE_LTV_OK;
}

int alore_ltv_plant_set_noise(alore_ltv_handle h, double noise_stddev, const double* meas_stddev, unsigned long long seed)
{
    if (!h) return ALORE_LTV_E_INVALID;
    if (!h->plant_ready) return lfail(h, ALORE_LTV_E_INVALID, "plant_set_noise: alore_ltv_plant_init has not been called");
    bool ok = std::isfinite(noise_stddev) && noise_stddev >= 0.0;
    for (int i = 0; meas_stddev && i < 3; ++i) ok = ok && std::isfinite(meas_stddev[i]) && meas_stddev[i] >= 0.0;
    if (!ok) return lfail(h, ALORE_LTV_E_INVALID, "plant_set_noise: a standard deviation is negative or not finite");
    h->noise_stddev = noise_stddev;
    for (int i = 0; i < 3; ++i) h->meas_stddev[i] = meas_stddev ? meas_stddev[i] : 0.0;
    h->noise_seed = seed;
    h->noise_event = 0;
    return ALORE_LTV_OK;
}

int alore_ltv_plant_noise_draws(alore_ltv_handle h, int B, unsigned long long event0, int n_events, int noise_stream, double* out, void* stream)
{
    if (!h) return ALORE_LTV_E_INVALID;
    LTV_ARGS(h, "plant_noise_draws", plant_args_bad(h, B));
    if (n_events < 1 || (long long)n_events * B > (1ll << 24) || noise_stream < 0 || noise_stream > 2 || !out)
        return lfail(h, ALORE_LTV_E_INVALID, "plant_noise_draws: n_events >= 1, at most 2^24 draws, noise_stream 0..2, out not null");
    LTV_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)n_events * B * 2;
    double* d = nullptr;
    LTV_TRY(h, hipMalloc((void**)&d, sizeof(double) * n));
    hipError_t e = ltv::launch_noise_draws(h->noise_seed, B, event0, n_events, noise_stream, d, s);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, sizeof(double) * n, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d);
    if (e != hipSuccess) return lfail(h, ALORE_LTV_E_HIP, "plant_noise_draws", e);
    return ALORE_LTV_OK;
}

int alore_ltv_refs_from_store_est(alore_ltv_handle h, void* nmpc, int B, double now, void* stream)
{
    if (!h) return ALORE_LTV_E_INVALID;
    nmpc::RefStore rs;
    ltv::EkfInfo ei;
    LTV_ARGS(h, "refs_from_store_est", plant_args_bad(h, B));
    if (!std::isfinite(now)) return lfail(h, ALORE_LTV_E_INVALID, "refs_from_store_est: now is not finite");
    LTV_ARGS(h, "refs_from_store_est", store_bad(h, nmpc, B, &rs));
    LTV_ARGS(h, "refs_from_store_est", ekf_bad(h, nmpc, B, &ei));
    LTV_TRY(h, hipSetDevice(h->device));
    LTV_PROMOTE(h, nmpc, now, stream);
    LTV_TRY(h, enq_refs_est(h, rs, B, now, ei.est_pose, (hipStream_t)stream));
    return ALORE_LTV_OK;
}

int alore_ltv_get_cmd_est(alore_ltv_handle h, void* nmpc, int B, int n_relin, double du_th, int reset, void* stream)
{
    if (!h) return ALORE_LTV_E_INVALID;
    ltv::EkfInfo ei;
    LTV_ARGS(h, "get_cmd_est", plant_args_bad(h, B));
    LTV_ARGS(h, "get_cmd_est", solve_args_bad(n_relin, du_th));
    LTV_ARGS(h, "get_cmd_est", ekf_bad(h, nmpc, B, &ei));
    LTV_TRY(h, hipSetDevice(h->device));
    LTV_TRY(h, enq_solve(h, B, n_relin, du_th, reset ? 1 : 0, (hipStream_t)stream, ei.est_pose));
    return ALORE_LTV_OK;
}

int alore_ltv_plant_ekf_step(alore_ltv_handle h, void* nmpc, int B, double dt_tick, void* stream)
{
    if (!h) return ALORE_LTV_E_INVALID;
    ltv::EkfInfo ei;
    LTV_ARGS(h, "plant_ekf_step", plant_args_bad(h, B));
    if (!std::isfinite(dt_tick) || !(dt_tick > 0.0)) return lfail(h, ALORE_LTV_E_INVALID, "plant_ekf_step: dt_tick must be finite and positive");
    LTV_ARGS(h, "plant_ekf_step", ekf_bad(h, nmpc, B, &ei));
    LTV_TRY(h, hipSetDevice(h->device));
    LTV_TRY(h, enq_plant_ekf(h, nmpc, ei, B, dt_tick, (hipStream_t)stream));
    return ALORE_LTV_OK;
}

int alore_ltv_ekf_closed_loop_run(alore_ltv_handle h, void* nmpc, int B, double t0, double dt_tick, int n_ticks, int n_relin, double du_th,
                                  int reset, void* stream)
{
    if (!h) return ALORE_LTV_E_INVALID;
    nmpc::RefStore rs;
    ltv::EkfInfo ei;
    LTV_ARGS(h, "ekf_closed_loop_run", plant_args_bad(h, B));
    LTV_ARGS(h, "ekf_closed_loop_run", run_args_bad(n_ticks, t0, dt_tick, true, n_relin, du_th));
    LTV_ARGS(h, "ekf_closed_loop_run", store_bad(h, nmpc, B, &rs));
    LTV_ARGS(h, "ekf_closed_loop_run", ekf_bad(h, nmpc, B, &ei));
    LTV_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    for (int k = 0; k < n_ticks; ++k) {
        if (k > 0) LTV_TRY(h, enq_plant_ekf(h, nmpc, ei, B, dt_tick, s));
        LTV_PROMOTE(h, nmpc, t0 + k * dt_tick, stream); // plant and sampler are launches of their own here: nothing to cut
        LTV_TRY(h, enq_refs_est(h, rs, B, t0 + k * dt_tick, ei.est_pose, s));
        LTV_TRY(h, enq_solve(h, B, n_relin, du_th, (k == 0 && reset) ? 1 : 0, s, ei.est_pose));
    }
    LTV_TRY(h, enq_plant_ekf(h, nmpc, ei, B, dt_tick, s));
    return ALORE_LTV_OK;
}

int alore_ltv_plant_get_trace_est(alore_ltv_handle h, int B, int max_ticks, double* est, int* ekf_status, int* n_ticks_out, void* stream)
{
    if (!h) return ALORE_LTV_E_INVALID;
    LTV_ARGS(h, "plant_get_trace_est", plant_args_bad(h, B));
    if (max_ticks < 0 || !n_ticks_out) return lfail(h, ALORE_LTV_E_INVALID, "plant_get_trace_est: bad argument");
    LTV_TRY(h, hipSetDevice(h->device));
    const size_t HB = h->B;
    const TraceCol cols[] = {{est, h->d_tr_est, sizeof(double), 0, 3, HB * 3}, {ekf_status, h->d_tr_ekf, sizeof(int), 0, 1, HB}};
    return get_trace_cols(h, B, max_ticks, cols, 2, n_ticks_out, (hipStream_t)stream);
}

} // extern "C"
