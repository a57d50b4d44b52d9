// nmpc_refs_capi.hip -- the part of the C ABI of include/alore_nmpc.h that works on the trajectory store of a handle: device-side
// reference sampling (alore_nmpc_refs_*), the plant and the closed loop on the device (alore_nmpc_plant_*, alore_nmpc_closed_loop_*),
// alore_nmpc_input_column.  The solver's own entry points are in nmpc_capi.hip.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nmpc_solver.h"
#include "../../include/alore_backend.h"

using namespace nmpc_capi;

int nmpc_capi::promote_if_due(alore_nmpc_handle h, double now, hipStream_t s)
{
    if (!h->handoff.times.due(now)) return ALORE_NMPC_OK;
    nmpc::PromoteArgs a{};
    a.act = h->refs.store;
    a.pen = h->handoff.pending;
    a.promotions = h->handoff.d_promotions;
    a.count = h->refs.B;
    a.now = now;
    HIP_TRY(h, nmpc::launch_traj_promote(a, s));
    h->handoff.times.promoted(now);
    return ALORE_NMPC_OK;
}

extern "C" {

int alore_nmpc_refs_init(alore_nmpc_handle h, int B, int max_pieces, int max_checkpoints)
{
    if (!h || B <= 0 || max_pieces <= 0 || max_checkpoints <= 0 || h->refs.store.dur)
        return fail(h, ALORE_NMPC_E_INVALID, "refs_init: bad argument or already initialised");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    h->refs.store.P = max_pieces;
    h->refs.store.C = max_checkpoints;
    h->refs.B = B;
    struct Want { void** p; size_t bytes; };
    const Want want[] = {
        {(void**)&h->refs.store.dur, sizeof(double) * B * max_pieces},
        {(void**)&h->refs.store.coef, sizeof(double) * B * max_pieces * 12},
        {(void**)&h->refs.store.ckpt, sizeof(double) * B * max_checkpoints * 2},
        {(void**)&h->refs.store.meta, sizeof(double) * B * 8},
        {(void**)&h->refs.d_est, sizeof(double) * B * 6}, // pose [B][3], then ICR [B][3]: one block, one copy per tick
        {(void**)&h->refs.d_psi, sizeof(double) * B * (h->cfg.N + 1)},
        {(void**)&h->refs.d_goal, sizeof(int) * B},
    };
    hipError_t e = hipSuccess;
    for (const Want& w : want) { // everything zeroed: slots without a trajectory read as invalid / not at goal
        e = hipMalloc(w.p, w.bytes);
        if (e == hipSuccess) e = hipMemset(*w.p, 0, w.bytes);
        if (e != hipSuccess) break;
    }
    if (e != hipSuccess) { // a retry must see "not initialised"
        for (const Want& w : want) {
            if (*w.p) (void)hipFree(*w.p);
            *w.p = nullptr;
        }
        h->refs.B = 0;
        return fail(h, ALORE_NMPC_E_NOMEM, "refs_init: hipMalloc", e);
    }
    h->refs.d_icr = h->refs.d_est + (size_t)B * 3;
    return ALORE_NMPC_OK;
}

int alore_nmpc_refs_set_trajectory(alore_nmpc_handle h, int robot, int n_pieces, const double* durations,
                                   const double* coeffs, int n_ckpt, const double* ckpt_xy, double start_time,
                                   double state_seq_res, double xv, void* stream)
{
    if (!h || !h->refs.store.dur || robot < 0 || robot >= h->refs.B || n_pieces <= 0 || n_pieces > h->refs.store.P || n_ckpt <= 0 ||
        n_ckpt > h->refs.store.C || !durations || !coeffs || !ckpt_xy || !(state_seq_res > 0.0))
        return fail(h, ALORE_NMPC_E_INVALID, "refs_set_trajectory: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    double total = 0.0;
    for (int i = 0; i < n_pieces; ++i) total += durations[i];
    const double meta[8] = {start_time, total, xv, state_seq_res, (double)n_pieces, (double)n_ckpt, 1.0, 0.0};
    HIP_TRY(h, hipMemcpyAsync(h->refs.store.dur + (size_t)robot * h->refs.store.P, durations, sizeof(double) * n_pieces, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->refs.store.coef + (size_t)robot * h->refs.store.P * 12, coeffs, sizeof(double) * n_pieces * 12, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->refs.store.ckpt + (size_t)robot * h->refs.store.C * 2, ckpt_xy, sizeof(double) * n_ckpt * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->refs.store.meta + (size_t)robot * 8, meta, sizeof(meta), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipStreamSynchronize(s)); // the host buffers (and `meta`) may go away after return
    return ALORE_NMPC_OK;
}

namespace {
struct PolyLayout { // byte offsets of the packed message arrays of one chunk
    size_t robot, n_pieces, inner, t_pts, pva, start, icr, t0, end;
};
PolyLayout poly_layout(int chunk, int P)
{
    PolyLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 15) & ~size_t(15); return at; };
    L.robot = take(sizeof(int) * chunk);
    L.n_pieces = take(sizeof(int) * chunk);
    L.inner = take(sizeof(double) * chunk * (P > 1 ? P - 1 : 1) * 2);
    L.t_pts = take(sizeof(double) * chunk * P);
    L.pva = take(sizeof(double) * chunk * 12);
    L.start = take(sizeof(double) * chunk * 3);
    L.icr = take(sizeof(double) * chunk * 3);
    L.t0 = take(sizeof(double) * chunk);
    L.end = o;
    return L;
}

// the pending store, its status slab and the promotion counters: allocated by the first call that needs them
int ensure_pending(alore_nmpc_handle h)
{
    if (h->handoff.pending.dur) return ALORE_NMPC_OK;
    const int B = h->refs.B, P = h->refs.store.P, Cn = h->refs.store.C;
    nmpc::RefStore& p = h->handoff.pending;
    struct Want { void** p; size_t bytes; };
    const Want want[] = {
        {(void**)&p.dur, sizeof(double) * B * P},
        {(void**)&p.coef, sizeof(double) * B * P * 12},
        {(void**)&p.ckpt, sizeof(double) * B * Cn * 2},
        {(void**)&p.meta, sizeof(double) * B * 8},
        {(void**)&h->handoff.d_promotions, sizeof(int) * B},
        {(void**)&h->handoff.d_status, sizeof(int) * B},
    };
    hipError_t e = hipSuccess;
    for (const Want& w : want) { // zeroed: every pending entry invalid, no promotion yet
        e = hipMalloc(w.p, w.bytes);
        if (e == hipSuccess) e = hipMemset(*w.p, 0, w.bytes);
        if (e != hipSuccess) break;
    }
    if (e == hipSuccess) {
        const std::vector<int> ones((size_t)B, traj_handoff::kNotAddressed);
        e = hipMemcpy(h->handoff.d_status, ones.data(), sizeof(int) * B, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) { // a retry must see "not allocated"
        for (const Want& w : want) {
            if (*w.p) (void)hipFree(*w.p);
            *w.p = nullptr;
        }
        return fail(h, ALORE_NMPC_E_NOMEM, "pending trajectory store: hipMalloc", e);
    }
    p.P = P;
    p.C = Cn;
    return ALORE_NMPC_OK;
}

nmpc::PromoteArgs promote_args(alore_nmpc_handle h, int count, double now, bool forced)
{
    nmpc::PromoteArgs a{};
    a.act = h->refs.store;
    a.pen = h->handoff.pending;
    a.promotions = h->handoff.d_promotions;
    a.count = count;
    a.now = now;
    a.forced = forced ? 1 : 0;
    return a;
}

// alore_nmpc_refs_set_polynomes (pending = false) and alore_nmpc_refs_set_pending_polynomes: the same staging and the same three
// kernels; the pending route targets the pending store, has the forced promotion of the addressed slots in front (mpc.cpp:151-156)
// and reports per slot through the status slab instead of one synchronised flag
int set_polynomes(alore_nmpc_handle h, int count, const int* robots, const alore_polynome* msgs, double state_seq_res, int integral_res_int,
                  void* stream, bool pending)
{
    const char* who = pending ? "refs_set_pending_polynomes: bad argument" : "refs_set_polynomes: bad argument";
    if (!h || !h->refs.store.dur || count < 0 || (count > 0 && (!robots || !msgs)) || !(state_seq_res > 0.0) || integral_res_int < 1)
        return fail(h, ALORE_NMPC_E_INVALID, who);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (pending)
        if (int rc = ensure_pending(h)) return rc;
    const nmpc::RefStore& store = pending ? h->handoff.pending : h->refs.store;
    hipStream_t s = (hipStream_t)stream;
    const int P = h->refs.store.P, CH = alore_nmpc_solver::PolyStaging::kChunk, Pi = (P > 1 ? P - 1 : 1);
    const PolyLayout Lmax = poly_layout(CH, P);
    if (!h->poly.d_poly) {
        HIP_TRY(h, hipMalloc((void**)&h->poly.d_poly, Lmax.end));
        HIP_TRY(h, hipMalloc((void**)&h->poly.d_knot, sizeof(double) * CH * 2 * nmpc::traj_ws_doubles(P)));
        HIP_TRY(h, hipMalloc((void**)&h->poly.d_panels, sizeof(int) * CH));
        HIP_TRY(h, hipMalloc((void**)&h->poly.d_overflow, sizeof(int)));
    }
    // messages per round: as many as the staging allows (one upload, three kernels and one wait per round), fewer when the
    // Simpson increments of a round ([C x res_int x 2] doubles per message) would pass 512 MB
    const size_t inc_per_msg = (size_t)h->refs.store.C * integral_res_int * 2;
    int chunk = (int)(((size_t)512 << 20) / (inc_per_msg * sizeof(double)));
    chunk = chunk < 64 ? 64 : (chunk > CH ? CH : chunk);
    if (chunk > count) chunk = count < 1 ? 1 : count;
    const size_t need = (size_t)chunk * inc_per_msg;
    if (need > h->poly.inc_doubles) {
        if (h->poly.d_inc) (void)hipFree(h->poly.d_inc);
        h->poly.d_inc = nullptr;
        HIP_TRY(h, hipMalloc((void**)&h->poly.d_inc, sizeof(double) * need));
        h->poly.inc_doubles = need;
    }
    HIP_TRY(h, hipMemsetAsync(h->poly.d_overflow, 0, sizeof(int), s));
    const PolyLayout L = poly_layout(chunk, P); // staging laid out for the round size in use: a single message stays a small copy
    std::vector<char> pack(L.end);
    for (int base = 0; base < count; base += chunk) {
        const int n = (count - base < chunk) ? count - base : chunk;
        std::fill(pack.begin(), pack.end(), 0);
        int* p_robot = reinterpret_cast<int*>(pack.data() + L.robot);
        int* p_np = reinterpret_cast<int*>(pack.data() + L.n_pieces);
        double* p_inner = reinterpret_cast<double*>(pack.data() + L.inner);
        double* p_t = reinterpret_cast<double*>(pack.data() + L.t_pts);
        double* p_pva = reinterpret_cast<double*>(pack.data() + L.pva);
        double* p_start = reinterpret_cast<double*>(pack.data() + L.start);
        double* p_icr = reinterpret_cast<double*>(pack.data() + L.icr);
        double* p_t0 = reinterpret_cast<double*>(pack.data() + L.t0);
        for (int i = 0; i < n; ++i) {
            const alore_polynome& m = msgs[base + i];
            if (robots[base + i] < 0 || robots[base + i] >= h->refs.B)
                return fail(h, ALORE_NMPC_E_INVALID, "refs_set_polynomes: robot index out of range");
            p_robot[i] = robots[base + i];
            p_np[i] = m.n_pieces; // > P is reported by the kernel through the overflow flag
            const int M = (m.n_pieces >= 1 && m.n_pieces <= P) ? m.n_pieces : 0;
            if (M > 0 && (!m.t_pts || (M > 1 && !m.innerpoints)))
                return fail(h, ALORE_NMPC_E_INVALID, "refs_set_polynomes: null array in a message");
            for (int k = 0; k < M; ++k) p_t[(size_t)i * P + k] = m.t_pts[k];
            for (int k = 0; k < 2 * (M - 1); ++k) p_inner[(size_t)i * Pi * 2 + k] = m.innerpoints[k];
            for (int d = 0; d < 2; ++d) {
                p_pva[i * 12 + d] = m.init_p[d]; p_pva[i * 12 + 2 + d] = m.init_v[d]; p_pva[i * 12 + 4 + d] = m.init_a[d];
                p_pva[i * 12 + 6 + d] = m.tail_p[d]; p_pva[i * 12 + 8 + d] = m.tail_v[d]; p_pva[i * 12 + 10 + d] = m.tail_a[d];
            }
            for (int k = 0; k < 3; ++k) { p_start[i * 3 + k] = m.start_position[k]; p_icr[i * 3 + k] = m.ICR[k]; }
            p_t0[i] = m.traj_start_time;
        }
        HIP_TRY(h, hipMemcpyAsync(h->poly.d_poly, pack.data(), L.end, hipMemcpyHostToDevice, s));
        nmpc::PolyBatch pb;
        pb.robot = reinterpret_cast<const int*>(h->poly.d_poly + L.robot);
        pb.n_pieces = reinterpret_cast<const int*>(h->poly.d_poly + L.n_pieces);
        pb.inner = reinterpret_cast<const double*>(h->poly.d_poly + L.inner);
        pb.t_pts = reinterpret_cast<const double*>(h->poly.d_poly + L.t_pts);
        pb.pva = reinterpret_cast<const double*>(h->poly.d_poly + L.pva);
        pb.start = reinterpret_cast<const double*>(h->poly.d_poly + L.start);
        pb.icr = reinterpret_cast<const double*>(h->poly.d_poly + L.icr);
        pb.t0 = reinterpret_cast<const double*>(h->poly.d_poly + L.t0);
        pb.P = P;
        if (pending) {
            nmpc::PromoteArgs pa = promote_args(h, n, 0.0, true);
            pa.robots = pb.robot;
            HIP_TRY(h, nmpc::launch_traj_promote(pa, s));
            for (int i = 0; i < n; ++i) h->handoff.times.add(msgs[base + i].traj_start_time);
        }
        HIP_TRY(h, nmpc::launch_traj_build(store, pb, n, state_seq_res, integral_res_int, h->poly.d_knot, h->poly.d_panels,
                                           h->poly.d_inc, h->poly.d_overflow, s, pending ? h->handoff.d_status : nullptr));
        HIP_TRY(h, hipStreamSynchronize(s)); // `pack` is reused by the next chunk
    }
    if (pending) return ALORE_NMPC_OK; // what happened to a slot is in its status word
    int ov = 0;
    HIP_TRY(h, hipMemcpyAsync(&ov, h->poly.d_overflow, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    if (ov & 1) return fail(h, ALORE_NMPC_E_INVALID, "refs_set_polynomes: a message has more pieces than max_pieces (or none)");
    if (ov & 2) return fail(h, ALORE_NMPC_E_INVALID, "refs_set_polynomes: a trajectory needs more checkpoints than max_checkpoints");
    return ALORE_NMPC_OK;
}
} // namespace

int alore_nmpc_refs_set_polynomes(alore_nmpc_handle h, int count, const int* robots, const alore_polynome* msgs,
                                  double state_seq_res, int integral_res_int, void* stream)
{
    return set_polynomes(h, count, robots, msgs, state_seq_res, integral_res_int, stream, false);
}

int alore_nmpc_refs_set_pending_polynomes(alore_nmpc_handle h, int count, const int* robots, const alore_polynome* msgs,
                                          double state_seq_res, int integral_res_int, void* stream)
{
    return set_polynomes(h, count, robots, msgs, state_seq_res, integral_res_int, stream, true);
}

// xv_slot: 0 the scalar xv for every slot, 1 d_xv[t] for slot t (the _xv entry points)
static int set_from_backend(alore_nmpc_handle h, const void* view, int count, double traj_start_time, double xv, const double* d_xv, int xv_slot,
                            double state_seq_res, int integral_res_int, void* stream)
{
    const alore_backend_device_view* v = static_cast<const alore_backend_device_view*>(view);
    if (xv_slot && !d_xv) return fail(h, ALORE_NMPC_E_INVALID, "refs_set_from_backend_xv: d_xv is null");
    if (!h || !h->refs.store.dur || !v || count < 1 || count > h->refs.B || !(state_seq_res > 0.0) || integral_res_int < 1)
        return fail(h, ALORE_NMPC_E_INVALID, "refs_set_from_backend: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (!h->poly.d_overflow) HIP_TRY(h, hipMalloc((void**)&h->poly.d_overflow, sizeof(int)));
    if ((size_t)count > h->poly.panels_cap) {
        if (h->poly.d_panels_be) (void)hipFree(h->poly.d_panels_be);
        h->poly.d_panels_be = nullptr;
        HIP_TRY(h, hipMalloc((void**)&h->poly.d_panels_be, sizeof(int) * count));
        h->poly.panels_cap = count;
    }
    const size_t need = (size_t)count * h->refs.store.C * integral_res_int * 2;
    if (need > h->poly.inc_doubles) {
        if (h->poly.d_inc) (void)hipFree(h->poly.d_inc);
        h->poly.d_inc = nullptr;
        h->poly.inc_doubles = 0;
        HIP_TRY(h, hipMalloc((void**)&h->poly.d_inc, sizeof(double) * need));
        h->poly.inc_doubles = need;
    }
    HIP_TRY(h, hipMemsetAsync(h->poly.d_overflow, 0, sizeof(int), s));
    const nmpc::BackendView bv{v->max_pieces, v->n_pieces, v->T, v->coef, v->start_xytheta, v->ok};
    HIP_TRY(h, nmpc::launch_traj_from_backend(h->refs.store, bv, count, traj_start_time, state_seq_res, integral_res_int, xv, h->poly.d_panels_be,
                                              h->poly.d_inc, h->poly.d_overflow, s, nullptr, 0, nullptr, d_xv));
    int ov = 0;
    HIP_TRY(h, hipMemcpyAsync(&ov, h->poly.d_overflow, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    if (ov & 1) return fail(h, ALORE_NMPC_E_INVALID, "refs_set_from_backend: a plan has more pieces than max_pieces");
    if (ov & 2) return fail(h, ALORE_NMPC_E_INVALID, "refs_set_from_backend: a trajectory needs more checkpoints than max_checkpoints");
    return ALORE_NMPC_OK;
}

int alore_nmpc_refs_set_from_backend(alore_nmpc_handle h, const void* view, int count, double traj_start_time, double xv,
                                     double state_seq_res, int integral_res_int, void* stream)
{
    return set_from_backend(h, view, count, traj_start_time, xv, nullptr, 0, state_seq_res, integral_res_int, stream);
}

int alore_nmpc_refs_set_from_backend_xv(alore_nmpc_handle h, const void* view, int count, double traj_start_time, const double* d_xv,
                                        double state_seq_res, int integral_res_int, void* stream)
{
    return set_from_backend(h, view, count, traj_start_time, 0.0, d_xv, 1, state_seq_res, integral_res_int, stream);
}

static int set_pending_from_backend(alore_nmpc_handle h, const void* view, int count, const int* mask, int mask_stride_bytes,
                                    double traj_start_time, double xv, const double* d_xv, int xv_slot, double state_seq_res,
                                    int integral_res_int, void* stream)
{
    const alore_backend_device_view* v = static_cast<const alore_backend_device_view*>(view);
    if (xv_slot && !d_xv) return fail(h, ALORE_NMPC_E_INVALID, "refs_set_pending_from_backend_xv: d_xv is null");
    if (!h || !h->refs.store.dur || !v || count < 1 || count > h->refs.B || !(state_seq_res > 0.0) || integral_res_int < 1 ||
        (mask && (mask_stride_bytes < (int)sizeof(int) || mask_stride_bytes % (int)sizeof(int))))
        return fail(h, ALORE_NMPC_E_INVALID, "refs_set_pending_from_backend: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ensure_pending(h)) return rc;
    // the workspace for the whole store at once: no later call allocates, whatever its count
    if ((size_t)h->refs.B > h->poly.panels_cap) {
        if (h->poly.d_panels_be) (void)hipFree(h->poly.d_panels_be);
        h->poly.d_panels_be = nullptr;
        h->poly.panels_cap = 0;
        HIP_TRY(h, hipMalloc((void**)&h->poly.d_panels_be, sizeof(int) * h->refs.B));
        h->poly.panels_cap = h->refs.B;
    }
    const size_t need = (size_t)h->refs.B * h->refs.store.C * integral_res_int * 2;
    if (need > h->poly.inc_doubles) {
        if (h->poly.d_inc) (void)hipFree(h->poly.d_inc);
        h->poly.d_inc = nullptr;
        h->poly.inc_doubles = 0;
        HIP_TRY(h, hipMalloc((void**)&h->poly.d_inc, sizeof(double) * need));
        h->poly.inc_doubles = need;
    }
    const int stride = mask ? mask_stride_bytes : 0;
    // mpc.cpp:151-156: an entry that is still pending in an addressed slot becomes active first, whatever its start time
    nmpc::PromoteArgs pa = promote_args(h, count, 0.0, true);
    pa.mask = mask; pa.mask_stride = stride; pa.ok = v->ok;
    HIP_TRY(h, nmpc::launch_traj_promote(pa, s));
    const nmpc::BackendView bv{v->max_pieces, v->n_pieces, v->T, v->coef, v->start_xytheta, v->ok};
    HIP_TRY(h, nmpc::launch_traj_from_backend(h->handoff.pending, bv, count, traj_start_time, state_seq_res, integral_res_int, xv,
                                              h->poly.d_panels_be, h->poly.d_inc, nullptr, s, mask, stride, h->handoff.d_status, d_xv));
    h->handoff.times.add(traj_start_time);
    return ALORE_NMPC_OK;
}

int alore_nmpc_refs_set_pending_from_backend(alore_nmpc_handle h, const void* view, int count, const int* mask, int mask_stride_bytes,
                                             double traj_start_time, double xv, double state_seq_res, int integral_res_int, void* stream)
{
    return set_pending_from_backend(h, view, count, mask, mask_stride_bytes, traj_start_time, xv, nullptr, 0, state_seq_res, integral_res_int,
                                    stream);
}

int alore_nmpc_refs_set_pending_from_backend_xv(alore_nmpc_handle h, const void* view, int count, const int* mask, int mask_stride_bytes,
                                                double traj_start_time, const double* d_xv, double state_seq_res, int integral_res_int,
                                                void* stream)
{
    return set_pending_from_backend(h, view, count, mask, mask_stride_bytes, traj_start_time, 0.0, d_xv, 1, state_seq_res, integral_res_int,
                                    stream);
}

int alore_nmpc_refs_promote(alore_nmpc_handle h, int B, double now, void* stream)
{
    if (!h || !h->refs.store.dur || B <= 0 || B > h->refs.B || now != now) return fail(h, ALORE_NMPC_E_INVALID, "refs_promote: bad argument");
    if (!h->handoff.pending.dur) return ALORE_NMPC_OK; // no pending entry was ever written
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, nmpc::launch_traj_promote(promote_args(h, B, now, false), (hipStream_t)stream));
    if (B == h->refs.B) h->handoff.times.promoted(now);
    return ALORE_NMPC_OK;
}

int alore_nmpc_refs_stop(alore_nmpc_handle h, int B, const int* d_mask, int mask_stride_bytes, void* stream)
{
    if (!h || !h->refs.store.dur || B <= 0 || B > h->refs.B || (d_mask && (mask_stride_bytes < (int)sizeof(int) || mask_stride_bytes % (int)sizeof(int))))
        return fail(h, ALORE_NMPC_E_INVALID, "refs_stop: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (!h->handoff.d_stopped) { // the first stop of the handle allocates the flags
        HIP_TRY(h, hipMalloc((void**)&h->handoff.d_stopped, sizeof(int) * h->refs.B));
        HIP_TRY(h, hipMemset(h->handoff.d_stopped, 0, sizeof(int) * h->refs.B));
    }
    HIP_TRY(h, nmpc::launch_traj_stop(h->refs.store.meta, h->handoff.pending.meta, h->handoff.d_stopped, d_mask, d_mask ? mask_stride_bytes : 0, B,
                                      (hipStream_t)stream));
    return ALORE_NMPC_OK;
}

int alore_nmpc_plant_stop(alore_nmpc_handle h, int B, const int* d_mask, int mask_stride_bytes, void* stream)
{
    if (!h || !h->refs.has_plant || B <= 0 || B > h->refs.B || (d_mask && (mask_stride_bytes < (int)sizeof(int) || mask_stride_bytes % (int)sizeof(int))))
        return fail(h, ALORE_NMPC_E_INVALID, "plant_stop: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, nmpc::launch_plant_stop(h->refs.d_vw, nullptr, 2, d_mask, d_mask ? mask_stride_bytes : 0, B, (hipStream_t)stream));
    return ALORE_NMPC_OK;
}

int alore_nmpc_refs_pending_status(alore_nmpc_handle h, int B, int* status, double* start_time, int* valid, int* promotions, void* stream)
{
    if (!h || !h->refs.store.dur || B <= 0 || B > h->refs.B) return fail(h, ALORE_NMPC_E_INVALID, "refs_pending_status: bad argument");
    if (!h->handoff.pending.dur) { // nothing pending, nothing promoted, no slot addressed
        for (int b = 0; b < B; ++b) {
            if (status) status[b] = traj_handoff::kNotAddressed;
            if (start_time) start_time[b] = 0.0;
            if (valid) valid[b] = 0;
            if (promotions) promotions[b] = 0;
        }
        return ALORE_NMPC_OK;
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    std::vector<double> meta((size_t)B * 8);
    HIP_TRY(h, hipMemcpyAsync(meta.data(), h->handoff.pending.meta, sizeof(double) * B * 8, hipMemcpyDeviceToHost, s));
    if (status) HIP_TRY(h, hipMemcpyAsync(status, h->handoff.d_status, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    if (promotions) HIP_TRY(h, hipMemcpyAsync(promotions, h->handoff.d_promotions, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) {
        if (start_time) start_time[b] = meta[(size_t)b * 8];
        if (valid) valid[b] = meta[(size_t)b * 8 + 6] != 0.0 ? 1 : 0;
    }
    return ALORE_NMPC_OK;
}

int alore_nmpc_refs_pending_device(alore_nmpc_handle h, alore_refs_pending_view* out)
{
    if (!h || !h->refs.store.dur || !out) return fail(h, ALORE_NMPC_E_INVALID, "refs_pending_device: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (int rc = ensure_pending(h)) return rc;
    out->status = h->handoff.d_status;
    out->promotions = h->handoff.d_promotions;
    out->pending_meta = h->handoff.pending.meta;
    out->active_meta = h->refs.store.meta;
    return ALORE_NMPC_OK;
}

namespace {
int download_slot(alore_nmpc_handle h, const nmpc::RefStore& st, int robot, double* meta8, double* durations, double* coeffs, double* ckpt_xy)
{
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipDeviceSynchronize());
    if (meta8) HIP_TRY(h, hipMemcpy(meta8, st.meta + (size_t)robot * 8, sizeof(double) * 8, hipMemcpyDeviceToHost));
    if (durations) HIP_TRY(h, hipMemcpy(durations, st.dur + (size_t)robot * st.P, sizeof(double) * st.P, hipMemcpyDeviceToHost));
    if (coeffs) HIP_TRY(h, hipMemcpy(coeffs, st.coef + (size_t)robot * st.P * 12, sizeof(double) * st.P * 12, hipMemcpyDeviceToHost));
    if (ckpt_xy) HIP_TRY(h, hipMemcpy(ckpt_xy, st.ckpt + (size_t)robot * st.C * 2, sizeof(double) * st.C * 2, hipMemcpyDeviceToHost));
    return ALORE_NMPC_OK;
}
} // namespace

int alore_nmpc_refs_download(alore_nmpc_handle h, int robot, double* meta8, double* durations, double* coeffs, double* ckpt_xy)
{
    if (!h || !h->refs.store.dur || robot < 0 || robot >= h->refs.B) return fail(h, ALORE_NMPC_E_INVALID, "refs_download: bad argument");
    return download_slot(h, h->refs.store, robot, meta8, durations, coeffs, ckpt_xy);
}

int alore_nmpc_refs_pending_download(alore_nmpc_handle h, int robot, double* meta8, double* durations, double* coeffs, double* ckpt_xy)
{
    if (!h || !h->refs.store.dur || robot < 0 || robot >= h->refs.B) return fail(h, ALORE_NMPC_E_INVALID, "refs_pending_download: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (int rc = ensure_pending(h)) return rc;
    return download_slot(h, h->handoff.pending, robot, meta8, durations, coeffs, ckpt_xy);
}

int alore_nmpc_refs_sample(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, double now, const double* est,
                           const double* icr, int do_smooth, int* at_goal, void* stream)
{
    if (!h || !h->refs.store.dur || !dev || B <= 0 || B > h->refs.B || !est || !icr || !dev->y || !dev->yN || !dev->od || !dev->x0)
        return fail(h, ALORE_NMPC_E_INVALID, "refs_sample: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    // pose and ICR from pageable memory go through pinned staging (two buffers in turn, so that the call never waits for its
    // predecessor's copies): a hipMemcpyAsync out of pageable memory blocks the host for the whole transfer, twice per tick
    const size_t bytes = sizeof(double) * (size_t)B * 3;
    const double *se = est, *si = icr;
    int turn = -1;
    if (!host_is_pinned(est) || !host_is_pinned(icr)) {
        turn = h->refs.pose_turn++ & 1;
        if (h->refs.pose_ev[turn]) HIP_TRY(h, hipEventSynchronize(h->refs.pose_ev[turn]));
        if (int rc = grow_stage(h, h->refs.pose_stage[turn], h->refs.pose_cap[turn], 2 * bytes)) return rc;
        std::memcpy(h->refs.pose_stage[turn], est, bytes);
        std::memcpy(h->refs.pose_stage[turn] + bytes, icr, bytes);
        se = reinterpret_cast<const double*>(h->refs.pose_stage[turn]);
        si = reinterpret_cast<const double*>(h->refs.pose_stage[turn] + bytes);
    }
    if (turn >= 0 && B == h->refs.B) { // staged back to back, stored back to back: one copy
        HIP_TRY(h, hipMemcpyAsync(h->refs.d_est, se, 2 * bytes, hipMemcpyHostToDevice, s));
    } else {
        HIP_TRY(h, hipMemcpyAsync(h->refs.d_est, se, bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(h->refs.d_icr, si, bytes, hipMemcpyHostToDevice, s));
    }
    if (turn >= 0) {
        if (!h->refs.pose_ev[turn]) HIP_TRY(h, hipEventCreateWithFlags(&h->refs.pose_ev[turn], hipEventDisableTiming));
        HIP_TRY(h, hipEventRecord(h->refs.pose_ev[turn], s));
    }
    HIP_TRY(h, nmpc::launch_ref_sample(h->refs.store, *dev, B, h->cfg.N, (double)h->cfg.dt, now, h->refs.d_est, h->refs.d_icr, h->refs.d_goal,
                                       h->refs.d_psi, do_smooth, s));
    if (at_goal) {
        HIP_TRY(h, hipMemcpyAsync(at_goal, h->refs.d_goal, sizeof(int) * B, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
    }
    return ALORE_NMPC_OK;
}

int alore_nmpc_refs_eval(alore_nmpc_handle h, int B, double now, double* out, void* stream)
{
    if (!h || !h->refs.store.dur || B <= 0 || B > h->refs.B || !out) return fail(h, ALORE_NMPC_E_INVALID, "refs_eval: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (!h->refs.d_flat) HIP_TRY(h, hipMalloc((void**)&h->refs.d_flat, sizeof(double) * h->refs.B * 4));
    HIP_TRY(h, nmpc::launch_ref_eval(h->refs.store, B, now, h->refs.d_flat, s));
    HIP_TRY(h, hipMemcpyAsync(out, h->refs.d_flat, sizeof(double) * B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return ALORE_NMPC_OK;
}

int alore_nmpc_plant_init(alore_nmpc_handle h, const alore_plant_params* p)
{
    if (!h || !h->refs.store.dur || !p || p->substeps < 1 || !(p->state_propa_period > 0.0) || !(p->pose_pub_period > 0.0))
        return fail(h, ALORE_NMPC_E_INVALID, "plant_init: needs refs_init first and positive periods");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (!h->refs.d_vw) HIP_TRY(h, hipMalloc((void**)&h->refs.d_vw, sizeof(double) * h->refs.B * 2));
    HIP_TRY(h, hipMemset(h->refs.d_vw, 0, sizeof(double) * h->refs.B * 2));
    h->refs.plant.max_a = p->max_acc; h->refs.plant.max_domega = p->max_domega;
    h->refs.plant.pose_pub_period = p->pose_pub_period; h->refs.plant.propa_period = p->state_propa_period;
    h->refs.plant.substeps = p->substeps;
    // closed_loop_run's second reference buffer and the float64 headings of the walk sampled ahead (nothing is allocated inside a run)
    if (h->refs.cl_B < h->refs.B) {
        const int Bc = h->refs.B, N = h->cfg.N;
        if (h->refs.cl_y) (void)hipFree(h->refs.cl_y);
        if (h->refs.cl_yN) (void)hipFree(h->refs.cl_yN);
        h->refs.cl_y = nullptr; h->refs.cl_yN = nullptr; h->refs.cl_B = 0;
        for (int i = 0; i < 2; ++i) { if (h->refs.cl_psi[i]) (void)hipFree(h->refs.cl_psi[i]); h->refs.cl_psi[i] = nullptr; }
        HIP_TRY(h, hipMalloc(&h->refs.cl_y, sizeof(float) * (size_t)Bc * N * 5));
        HIP_TRY(h, hipMalloc(&h->refs.cl_yN, sizeof(float) * (size_t)Bc * 3));
        for (int i = 0; i < 2; ++i) HIP_TRY(h, hipMalloc(&h->refs.cl_psi[i], sizeof(double) * (size_t)Bc * (N + 1)));
        h->refs.cl_B = Bc;
    }
    h->refs.has_plant = true;
    return ALORE_NMPC_OK;
}

int alore_nmpc_plant_set_state(alore_nmpc_handle h, int B, const double* pose, const double* vw, const double* icr, void* stream)
{
    if (!h || !h->refs.has_plant || B <= 0 || B > h->refs.B || !pose || !icr)
        return fail(h, ALORE_NMPC_E_INVALID, "plant_set_state: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(h, hipMemcpyAsync(h->refs.d_est, pose, sizeof(double) * B * 3, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->refs.d_icr, icr, sizeof(double) * B * 3, hipMemcpyHostToDevice, s));
    if (vw) HIP_TRY(h, hipMemcpyAsync(h->refs.d_vw, vw, sizeof(double) * B * 2, hipMemcpyHostToDevice, s));
    else HIP_TRY(h, hipMemsetAsync(h->refs.d_vw, 0, sizeof(double) * B * 2, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return ALORE_NMPC_OK;
}

int alore_nmpc_plant_get_state(alore_nmpc_handle h, int B, double* pose, double* vw, int* at_goal, void* stream)
{
    if (!h || !h->refs.has_plant || B <= 0 || B > h->refs.B) return fail(h, ALORE_NMPC_E_INVALID, "plant_get_state: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (pose) HIP_TRY(h, hipMemcpyAsync(pose, h->refs.d_est, sizeof(double) * B * 3, hipMemcpyDeviceToHost, s));
    if (vw) HIP_TRY(h, hipMemcpyAsync(vw, h->refs.d_vw, sizeof(double) * B * 2, hipMemcpyDeviceToHost, s));
    if (at_goal) HIP_TRY(h, hipMemcpyAsync(at_goal, h->refs.d_goal, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return ALORE_NMPC_OK;
}

int alore_nmpc_closed_loop_reset(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, const unsigned char* mask, void* stream)
{
    if (!h || !h->refs.has_plant || !dev || !dev->x || !dev->u || B <= 0 || B > h->refs.B)
        return fail(h, ALORE_NMPC_E_INVALID, "closed_loop_reset: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    unsigned char* d_mask = nullptr;
    if (mask) {
        if (!h->refs.d_mask) HIP_TRY(h, hipMalloc((void**)&h->refs.d_mask, (size_t)h->refs.B));
        HIP_TRY(h, hipMemcpyAsync(h->refs.d_mask, mask, (size_t)B, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipStreamSynchronize(s)); // `mask` may go away after return
        d_mask = h->refs.d_mask;
    }
    HIP_TRY(h, nmpc::launch_iterate_reset(*dev, B, h->cfg.N, h->refs.d_est, d_mask, s));
    return ALORE_NMPC_OK;
}

int alore_nmpc_closed_loop_tick(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, double now, int delay_num, void* stream)
{
    if (!h || !h->refs.has_plant || !dev || B <= 0 || B > h->refs.B || delay_num < 0)
        return fail(h, ALORE_NMPC_E_INVALID, "closed_loop_tick: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    const int N = h->cfg.N;
    if (int rc = promote_if_due(h, now, s)) return rc; // mpc.cpp:177-182: a pending trajectory whose start time has passed is swapped in
    // CmdCallback: references from the measured pose, one real-time iteration, command = input column delay_num
    HIP_TRY(h, nmpc::launch_ref_sample(h->refs.store, *dev, B, N, (double)h->cfg.dt, now, h->refs.d_est, h->refs.d_icr, h->refs.d_goal, h->refs.d_psi, 1, s));
    const int rc = alore_nmpc_rti(h, dev, B, 1, stream);
    if (rc != ALORE_NMPC_OK) return rc;
    // alore_nmpc_refs_stop: the zero command of emergencyStop holds while the robot has no trajectory (a handle that never stopped
    // a robot enqueues what it always did)
    if (h->handoff.d_stopped)
        HIP_TRY(h, nmpc::launch_stop_hold(dev->u, h->refs.store.meta, h->handoff.d_stopped, B, N, delay_num < N ? delay_num : N - 1, s));
    HIP_TRY(h, nmpc::launch_plant(*dev, B, N, delay_num < N ? delay_num : N - 1, h->refs.d_icr, h->refs.d_goal, h->refs.d_est, h->refs.d_vw, h->refs.plant, s));
    return ALORE_NMPC_OK;
}

int alore_nmpc_refs_at_goal(alore_nmpc_handle h, int B, int* at_goal, void* stream)
{
    if (!h || !h->refs.store.dur || B <= 0 || B > h->refs.B || !at_goal) return fail(h, ALORE_NMPC_E_INVALID, "refs_at_goal: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipMemcpyAsync(at_goal, h->refs.d_goal, sizeof(int) * B, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return ALORE_NMPC_OK;
}

namespace {
static __global__ void pack_input_column_kernel(const float* u, const int* status, int B, int N, int node, float* cmd, int* st)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    cmd[2 * b] = u[((size_t)b * N + node) * 2];
    cmd[2 * b + 1] = u[((size_t)b * N + node) * 2 + 1];
    if (st) st[b] = status[b];
}
} // namespace

int alore_nmpc_input_column(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, int node, float* cmd, int* status, void* stream)
{
    if (!h || !dev || !dev->u || B <= 0 || node < 0 || node >= h->cfg.N || !cmd || (status && !dev->status))
        return fail(h, ALORE_NMPC_E_INVALID, "input_column: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    const size_t need = (size_t)B * 12;
    if (int rc = grow_stage(h, h->pinned.down, h->pinned.down_cap, need)) return rc;
    // the pack kernel writes the 12 bytes per problem straight into the pinned slab (device alias of the host pointer)
    void* dalias = nullptr;
    HIP_TRY(h, hipHostGetDevicePointer(&dalias, h->pinned.down, 0));
    float* dc = (float*)dalias;
    int* ds = (int*)(dc + (size_t)B * 2);
    hipLaunchKernelGGL(pack_input_column_kernel, dim3((B + 255) / 256), dim3(256), 0, s, dev->u, dev->status, B, h->cfg.N, node, dc,
                       status ? ds : nullptr);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(s));
    std::memcpy(cmd, h->pinned.down, sizeof(float) * B * 2);
    if (status) std::memcpy(status, h->pinned.down + sizeof(float) * B * 2, sizeof(int) * B);
    return ALORE_NMPC_OK;
}

namespace {
// ticks [first, first + n_ticks) of a run that started at t0, as a complete run: tick t of them has the time of tick first + t of the
// whole run (traj_handoff::tick_time), never a time summed up from a shifted t0
int run_segment(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, double t0, double dt_tick, int first, int n_ticks, int delay_num,
                void* stream)
{
    auto time_of = [&](int t) { return traj_handoff::tick_time(t0, dt_tick, (long)first + t); };
    static const bool serial = [] { const char* e = getenv("ALORE_NMPC_CLOSED_LOOP_SERIAL"); return e && atoi(e) != 0; }();
    // a handle that has stopped a robot (alore_nmpc_refs_stop) runs tick by tick: the hold of the zero command sits between solve and plant
    const bool ahead = !serial && n_ticks >= 3 && h && h->refs.has_plant && dev && dev->y && dev->yN && dev->x0 && B > 0 && B <= h->refs.B &&
                       delay_num >= 0 && nmpc::ref_sample_ahead_supported(h->cfg.N) && !h->handoff.d_stopped;
    if (!ahead) {
        for (int t = 0; t < n_ticks; ++t) {
            const int rc = alore_nmpc_closed_loop_tick(h, dev, B, time_of(t), delay_num, stream);
            if (rc != ALORE_NMPC_OK) return rc;
        }
        return ALORE_NMPC_OK;
    }
    // The chain of a tick is sampler -> solve -> plant, and the sampler needs the pose only for x0 and for the turns that the heading
    // walk starts from (smooth_yaw's first step): everything else of tick t + 1 is sampled by extra workgroups of the grid that
    // solves tick t (rti_block_sampler_kernel), into the other of two reference buffers; the plant step of tick t writes x0 and
    // shifts the headings, and runs in front of the solve of tick t + 1 in that solve's grid.  One launch per tick on the caller's
    // stream.  (A second stream for the sampler was built first: its two cross-stream events per tick cost what the overlap saved.)
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    const int N = h->cfg.N, node = delay_num < N ? delay_num : N - 1;
    if (h->refs.cl_B < B) return fail(h, ALORE_NMPC_E_INVALID, "closed_loop_run: more robots than plant_init allocated for");
    alore_nmpc_batch buf[2] = {*dev, *dev};
    buf[1].y = h->refs.cl_y;
    buf[1].yN = h->refs.cl_yN;
    // both buffers start as the caller's references: a robot without a trajectory keeps them, whichever buffer its tick reads
    HIP_TRY(h, hipMemcpyAsync(h->refs.cl_y, dev->y, sizeof(float) * (size_t)B * N * 5, hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->refs.cl_yN, dev->yN, sizeof(float) * (size_t)B * 3, hipMemcpyDeviceToDevice, s));
    // tick 0 is sampled whole (od, x0 from the current pose)
    HIP_TRY(h, nmpc::launch_ref_sample(h->refs.store, *dev, B, N, (double)h->cfg.dt, time_of(0), h->refs.d_est, h->refs.d_icr, h->refs.d_goal, h->refs.d_psi, 1, s));
    // per tick ONE launch: [plant step of tick t - 1 -> solve of tick t] beside [sampler of tick t + 1]
    auto plant_of = [&](int t, bool more) {
        const int cur = t & 1, nxt = cur ^ 1;
        nmpc::PlantAhead a{};
        a.u = buf[cur].u;
        a.x0 = const_cast<float*>(buf[nxt].x0);
        a.y = const_cast<float*>(buf[nxt].y);
        a.yN = const_cast<float*>(buf[nxt].yN);
        a.meta = h->refs.store.meta;
        a.icr = h->refs.d_icr;
        a.at_goal = h->refs.d_goal;
        a.pose = h->refs.d_est;
        a.vw = h->refs.d_vw;
        a.psi_rel = more ? h->refs.cl_psi[nxt] : nullptr;
        a.p = h->refs.plant;
        a.now = time_of(t);
        a.B = B; a.N = N; a.node = node;
        return a;
    };
    for (int t = 0; t < n_ticks; ++t) {
        const bool more = t + 1 < n_ticks;
        const int cur = t & 1, nxt = cur ^ 1;
        nmpc::AheadSampler sa{};
        sa.store = h->refs.store;
        sa.y = const_cast<float*>(buf[nxt].y);
        sa.yN = const_cast<float*>(buf[nxt].yN);
        sa.icr = h->refs.d_icr;
        sa.psi_rel = h->refs.cl_psi[nxt];
        sa.dt = (double)h->cfg.dt;
        sa.now = time_of(t + 1);
        sa.B = more ? B : 0; // the last tick has nothing to sample for
        sa.N = N;
        bool sampled = false;
        if (!batch_complete(&buf[cur])) return fail(h, ALORE_NMPC_E_INVALID, "closed_loop_run: batch has NULL members");
        const nmpc::PlantAhead prev = plant_of(t > 0 ? t - 1 : 0, true);
        const int rc = rti_one(h, &buf[cur], B, 1, stream, 0, &sa, &sampled, t > 0 ? &prev : nullptr);
        if (rc != ALORE_NMPC_OK) return rc;
        if (more && !sampled) // no build of this mapping carries the sampler: its own launch, in the chain
            HIP_TRY(h, nmpc::launch_ref_sample_ahead(h->refs.store, buf[nxt], B, N, sa.dt, sa.now, h->refs.d_icr, h->refs.cl_psi[nxt], s));
    }
    HIP_TRY(h, nmpc::launch_plant_ahead(plant_of(n_ticks - 1, false), s)); // the plant step of the last tick
    if ((n_ticks - 1) & 1) { // the last tick read the internal buffer: the caller's y / yN are those of the last tick afterwards, as in a tick-by-tick run
        HIP_TRY(h, hipMemcpyAsync(const_cast<float*>(dev->y), h->refs.cl_y, sizeof(float) * (size_t)B * N * 5, hipMemcpyDeviceToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(const_cast<float*>(dev->yN), h->refs.cl_yN, sizeof(float) * (size_t)B * 3, hipMemcpyDeviceToDevice, s));
    }
    return ALORE_NMPC_OK;
}
} // namespace

int alore_nmpc_closed_loop_run(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, double t0, double dt_tick, int n_ticks,
                               int delay_num, void* stream)
{
    if (n_ticks < 0 || !(dt_tick > 0.0)) return fail(h, ALORE_NMPC_E_INVALID, "closed_loop_run: bad argument");
    if (!h || !h->handoff.times.any()) return run_segment(h, dev, B, t0, dt_tick, 0, n_ticks, delay_num, stream);
    // The fused run reads the store for two ticks at once (the ahead sampler of tick t + 1 beside the plant step of tick t - 1), so
    // a promotion cannot go between two of its launches: the run is cut where one is due, every part runs as a complete run (with its
    // trailing plant step and the copy back of y / yN), and the promotion goes between the parts (traj_handoff.h: split_run)
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const std::vector<double> starts = h->handoff.times.t;
    for (const traj_handoff::Segment& g : traj_handoff::split_run(t0, dt_tick, n_ticks, starts.data(), starts.size())) {
        if (g.promote)
            if (int rc = promote_if_due(h, traj_handoff::tick_time(t0, dt_tick, g.first), (hipStream_t)stream)) return rc;
        if (int rc = run_segment(h, dev, B, t0, dt_tick, g.first, g.count, delay_num, stream)) return rc;
    }
    return ALORE_NMPC_OK;
}

// internal (not in the public header), for the LTV-MPC loops on this handle's store (ltv_mpc_capi.hip): the promotion that goes in
// front of a sampler at `now` (enqueued only while a pending start time is outstanding; nonzero: a HIP error), and the outstanding
// start times, for the run splitter
int alore_nmpc_internal_promote_if_due(void* nmpc_handle, double now, void* stream)
{
    alore_nmpc_handle h = static_cast<alore_nmpc_handle>(nmpc_handle);
    if (!h || !h->handoff.times.any()) return 0;
    return promote_if_due(h, now, (hipStream_t)stream);
}
int alore_nmpc_internal_pending_times(void* nmpc_handle, const double** starts, size_t* n)
{
    alore_nmpc_handle h = static_cast<alore_nmpc_handle>(nmpc_handle);
    if (!h || !starts || !n) return -1;
    *starts = h->handoff.times.t.data();
    *n = h->handoff.times.t.size();
    return 0;
}

// internal (not in the public header): the trajectory store of a handle, for the LTV-MPC reference sampler (ltv_mpc.hip)
int alore_nmpc_internal_refstore(void* nmpc_handle, nmpc::RefStore* out, int* capacity, int* device)
{
    alore_nmpc_handle h = static_cast<alore_nmpc_handle>(nmpc_handle);
    if (!h || !h->refs.store.dur || !out) return -1;
    *out = h->refs.store;
    if (capacity) *capacity = h->refs.B;
    if (device) *device = h->cfg.device;
    return 0;
}

} // extern "C"
