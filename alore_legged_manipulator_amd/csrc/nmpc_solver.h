// nmpc_solver.h -- the handle behind the C ABI of include/alore_nmpc.h and what its implementation files (nmpc_capi.hip: the
// solver; nmpc_refs_capi.hip: reference store, plant, closed loop; icr_ekf.hip: the ICR EKF and the loop on its estimate) share (internal).
#ifndef ALORE_NMPC_SOLVER_H
#define ALORE_NMPC_SOLVER_H

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "nmpc_kernels.h"
#include "traj_handoff.h"

// The handle: the configuration and the per-call settings, then one member per subsystem that owns device or host resources, each
// with the function that gives them back (alore_nmpc_destroy calls them).
struct alore_nmpc_solver {
    alore_nmpc_config cfg;
    int n_cu = 256;
    int lds_limit = 160 * 1024;
    std::string err;
    nmpc::LaunchGeom last_geom{};
    bool have_geom = false;
    unsigned shared = 0;          // see alore_nmpc_set_shared_members
    const unsigned char* mask = nullptr; // see alore_nmpc_set_problem_mask
    const float* lin_x = nullptr; // see alore_nmpc_set_linearization_point
    const float* lin_u = nullptr;
    // alore_nmpc_rti_converge / alore_nmpc_rti_many_converge: the request of the call in progress (conv_tol < 0: none), and the row of
    // conv_iters ([count][B]) that belongs to the first batch of the launch being enqueued
    float conv_tol = -1.0f;
    int* conv_iters = nullptr;
    int conv_row = 0;
    // alore_nmpc_rti_many: launches of independent batches in flight at once (side streams forked from the caller's)
    int overlap = 16;
    bool auto_pg = false; // warm_start_steps was left to the library: 6 for a launch on its own, 3 inside a grid of many batches
    int many_mode = 0; // alore_nmpc_rti_many: 0 = groups of batches per grid, 1 = one launch per batch on forked streams

    // alore_nmpc_set_timing: one pair of events around the last launch
    struct Timing {
        bool on = false;
        bool pending = false;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        float last_ms = -1.0f;
        void release()
        {
            if (ev0) (void)hipEventDestroy(ev0);
            if (ev1) (void)hipEventDestroy(ev1);
        }
    } timing;

    // device-side reference sampling (alore_nmpc_refs_*) and the closed loop on the device (alore_nmpc_plant_*, alore_nmpc_closed_loop_*)
    struct Refs {
        nmpc::RefStore store{};
        int B = 0;
        double* d_est = nullptr;  // [B][3]
        double* d_icr = nullptr;  // [B][3]
        double* d_psi = nullptr;  // [B][N+1]
        int* d_goal = nullptr;    // [B]
        // closed loop: pose = d_est, ICR = d_icr
        double* d_vw = nullptr;   // [B][2] current (v, omega) of the plant
        double* d_flat = nullptr; // [B][4] alore_nmpc_refs_eval output
        unsigned char* d_mask = nullptr; // [B] alore_nmpc_closed_loop_reset
        nmpc::PlantParams plant{};
        bool has_plant = false;
        // alore_nmpc_closed_loop_run: the sampler of tick t + 1 runs in the grid of the solve of tick t, into the second of two
        // reference buffers (the caller's y / yN and these), its float64 headings into cl_psi for the plant step to complete
        float* cl_y = nullptr;   // [B][N][5]
        float* cl_yN = nullptr;  // [B][3]
        double* cl_psi[2] = {};  // [B][N + 1]
        int cl_B = 0;
        char* pose_stage[2] = {};      // alore_nmpc_refs_sample: pinned staging of the pose + ICR of a tick
        size_t pose_cap[2] = {};
        hipEvent_t pose_ev[2] = {};
        unsigned pose_turn = 0;
        void release()
        {
            if (store.dur) (void)hipFree(store.dur);
            if (store.coef) (void)hipFree(store.coef);
            if (store.ckpt) (void)hipFree(store.ckpt);
            if (store.meta) (void)hipFree(store.meta);
            for (int i = 0; i < 2; ++i)
                if (cl_psi[i]) (void)hipFree(cl_psi[i]);
            for (int i = 0; i < 2; ++i) {
                if (pose_ev[i]) { (void)hipEventSynchronize(pose_ev[i]); (void)hipEventDestroy(pose_ev[i]); }
                if (pose_stage[i]) (void)hipHostFree(pose_stage[i]);
            }
            if (cl_y) (void)hipFree(cl_y);
            if (cl_yN) (void)hipFree(cl_yN);
            if (d_est) (void)hipFree(d_est); // d_icr is its second half
            if (d_psi) (void)hipFree(d_psi);
            if (d_goal) (void)hipFree(d_goal);
            if (d_vw) (void)hipFree(d_vw);
            if (d_flat) (void)hipFree(d_flat);
            if (d_mask) (void)hipFree(d_mask);
        }
    } refs;

    // hand-over to a replanned trajectory (alore_nmpc_refs_set_pending_*, alore_nmpc_refs_promote; traj_handoff.h): a second store
    // with the P and C of refs.store, allocated by the first call that needs it
    struct Handoff {
        nmpc::RefStore pending{};
        int* d_status = nullptr;      // [B] traj_handoff::kWritten ... of the last set_pending call that addressed the slot
        int* d_promotions = nullptr;  // [B]
        int* d_stopped = nullptr;     // [B] alore_nmpc_refs_stop: robots whose command is held at zero until they have a trajectory again
        traj_handoff::PendingTimes times; // start times handed in and not yet passed by a promotion over every robot
        void release()
        {
            if (d_stopped) (void)hipFree(d_stopped);
            if (pending.dur) (void)hipFree(pending.dur);
            if (pending.coef) (void)hipFree(pending.coef);
            if (pending.ckpt) (void)hipFree(pending.ckpt);
            if (pending.meta) (void)hipFree(pending.meta);
            if (d_status) (void)hipFree(d_status);
            if (d_promotions) (void)hipFree(d_promotions);
        }
    } handoff;

    // Polynome -> store on the device: staging + workspace for chunks of kChunk messages
    struct PolyStaging {
        static constexpr int kChunk = 2048;
        char* d_poly = nullptr;       // packed message arrays (layout: poly_layout)
        double* d_knot = nullptr;     // [chunk][2][traj_ws_doubles(P)] workspace of the spline kernel
        int* d_panels = nullptr;      // [chunk]
        int* d_overflow = nullptr;    // [1]
        double* d_inc = nullptr;      // [chunk][C * res_int][2], grown on demand
        int* d_panels_be = nullptr;   // [count] panels per plan (alore_nmpc_refs_set_from_backend)
        size_t panels_cap = 0;
        size_t inc_doubles = 0;
        void release()
        {
            if (d_poly) (void)hipFree(d_poly);
            if (d_knot) (void)hipFree(d_knot);
            if (d_panels) (void)hipFree(d_panels);
            if (d_overflow) (void)hipFree(d_overflow);
            if (d_inc) (void)hipFree(d_inc);
            if (d_panels_be) (void)hipFree(d_panels_be);
        }
    } poly;

    // pinned staging for alore_nmpc_batch_upload / _download from pageable host memory (and alore_nmpc_input_column)
    struct PinnedStaging {
        char* up = nullptr;
        char* down = nullptr;
        size_t up_cap = 0, down_cap = 0;
        hipEvent_t up_done = nullptr; // the copies out of `up` enqueued by the last upload
        void release()
        {
            if (up_done) { (void)hipEventSynchronize(up_done); (void)hipEventDestroy(up_done); }
            if (up) (void)hipHostFree(up);
            if (down) (void)hipHostFree(down);
        }
    } pinned;

    // the last descriptor sets that passed the independence check of alore_nmpc_rti_many, kept whole (with the B and the shared-member
    // mask they were checked for): any contiguous run of one is independent too
    // (four sets, least recently used replaced: a host that alternates between slot ranges -- warm-up slots and timed slots, two fleets --
    // keeps both known; with one set the second range's call overwrote the first and every call paid the check again)
    struct IndepCache {
        static constexpr int kSets = 4;
        std::vector<alore_nmpc_batch> set[kSets];
        int B[kSets] = {0, 0, 0, 0};
        unsigned shared[kSets] = {0, 0, 0, 0};
        unsigned long long used[kSets] = {0, 0, 0, 0}, clock = 0;
    } indep; // (nothing to release: host memory of its own)

    // alore_nmpc_rti_many, streams mode: side streams forked from the caller's and joined back into it
    struct Forks {
        hipStream_t side[31] = {};
        hipEvent_t fork_ev = nullptr, join_ev[31] = {};
        void release()
        {
            for (int w = 0; w < 31; ++w) {
                if (side[w]) (void)hipStreamDestroy(side[w]);
                if (join_ev[w]) (void)hipEventDestroy(join_ev[w]);
            }
            if (fork_ev) (void)hipEventDestroy(fork_ev);
        }
    } forks;

    // diagnostic phase stamps (env ALORE_NMPC_STAMPS=1): per-phase cycle shares, printed when the handle goes
    struct Stamps {
        bool on = false;
        long long* d_stamps = nullptr;
        size_t cap = 0;
        double sum[7] = {0, 0, 0, 0, 0, 0, 0};
        double max_total = 0;
        double max[7] = {0, 0, 0, 0, 0, 0, 0};
        double slowest[7] = {0, 0, 0, 0, 0, 0, 0};
        long n = 0;
        void release()
        {
            if (on && n > 0) {
                static const char* names[7] = {"load+linearise", "backward sweeps", "forward sweeps", "kkt+expand",
                                               "objective+store", "total", "ws prediction"};
                std::fprintf(stderr, "[alore_nmpc stamps] mean cycles per workgroup over %ld workgroup-launches:\n", n);
                for (int i = 0; i < 7; ++i)
                    std::fprintf(stderr, "  %-16s %10.0f  (%5.1f %%)\n", names[i], sum[i] / n, 100.0 * sum[i] / sum[5]);
                std::fprintf(stderr, "  slowest workgroup total: %.0f cycles; its phases:", max_total);
                for (int i = 0; i < 7; ++i) std::fprintf(stderr, " %.0f", slowest[i]);
                std::fprintf(stderr, "\n  per-phase maxima:");
                for (int i = 0; i < 7; ++i) std::fprintf(stderr, " %.0f", max[i]);
                std::fprintf(stderr, "\n");
            }
            if (d_stamps) (void)hipFree(d_stamps);
        }
    } stamps;

    // XCD shares of the grid builds (nmpc_block_kernel.hip: RtiGroup::xcd_on): relative speed of the eight XCDs as the finishing times of
    // their last workgroups showed it at the previous launches, the host-memory record the running launch writes, its event
    struct XcdShares {
        double speed[8] = {1, 1, 1, 1, 1, 1, 1, 1};
        unsigned long long* rec = nullptr;  // pinned host memory [8][4] end stamps + [32] start stamp
        hipEvent_t ev = nullptr;
        bool pending = false;
        int updates = 0;
        void release()
        {
            if (std::getenv("ALORE_NMPC_XCD_DEBUG") && updates > 0)
                std::fprintf(stderr, "[alore_nmpc xcd shares] %d updates; relative speeds %.3f %.3f %.3f %.3f %.3f %.3f %.3f %.3f\n", updates, speed[0], speed[1],
                             speed[2], speed[3], speed[4], speed[5], speed[6], speed[7]);
            if (ev) { (void)hipEventSynchronize(ev); (void)hipEventDestroy(ev); }
            if (rec) (void)hipHostFree(rec);
        }
    } xcd;

    // two-phase grids (nmpc_block_kernel.hip: TWOPH): queue regions (header + entries per batch, all 0 between launches), one per launch
    // in turn with the stream and an event of its last user; the host-memory record of the last launch (deferred problems per batch,
    // error word) that sizes the next launch's tail
    struct TwoPhaseRing {
        static constexpr int kRing = 4;
        char* queue[kRing] = {};
        size_t cap[kRing] = {};
        hipStream_t stream[kRing] = {};
        hipEvent_t ev[kRing] = {};
        bool used[kRing] = {};
        unsigned turn = 0;
        int* rec = nullptr;      // pinned host memory [40]
        hipEvent_t rec_ev = nullptr;
        bool rec_pending = false;
        double share = 0.30;     // share of a batch's problems the tail is sized for
        int mode = -1;           // alore_nmpc_set_two_phase: -1 automatic, 0 never, 1 wherever the build exists
        int last = 0;            // the last grid ran in two phases (launch info)
        int slot_of_launch = -1;
        int info[3] = {0, 0, 0}; // two-phase batches, tail workgroups per batch, lag of the last two-phase grid
        void release()
        {
            if (rec_ev) { (void)hipEventSynchronize(rec_ev); (void)hipEventDestroy(rec_ev); }
            if (rec) (void)hipHostFree(rec);
            for (int i = 0; i < kRing; ++i) {
                if (ev[i]) { (void)hipEventSynchronize(ev[i]); (void)hipEventDestroy(ev[i]); }
                if (queue[i]) (void)hipFree(queue[i]);
            }
        }
    } tp;

    // ticket counters of the persistent grids (nmpc_block_kernel.hip: PERSIST): a ring of pairs, one pair per launch in turn, so
    // that grids of this handle that overlap on different streams never share one; every pair is back at 0 when its grid ends
    struct Tickets {
        static constexpr int kRing = 16;
        int* d_tickets = nullptr;
        unsigned turn = 0;
        void release()
        {
            if (d_tickets) (void)hipFree(d_tickets);
        }
    } tickets;

    // the ICR EKF on the device (alore_nmpc_ekf_*, icr_ekf.hip): one allocation for the capacity of the trajectory store, made by
    // alore_nmpc_ekf_init and cut up there; the parameters as the caller gave them; the ticks of the EKF closed loop since the reset
    struct Ekf {
        char* d_block = nullptr;
        int B = 0;
        alore_ekf_params params{};
        long ticks = 0;
        void release()
        {
            if (d_block) (void)hipFree(d_block);
        }
    } ekf;
};

namespace nmpc_capi {

inline int fail(alore_nmpc_handle h, int code, const char* what, hipError_t e = hipSuccess)
{
    if (h) {
        h->err = what;
        if (e != hipSuccess) {
            h->err += ": ";
            h->err += hipGetErrorString(e);
        }
    }
    return code;
}

#define HIP_TRY(h, call)                                                              \
    do {                                                                              \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess) return nmpc_capi::fail(h, ALORE_NMPC_E_HIP, #call, e_); \
    } while (0)

struct Member {
    size_t offset; // byte offset of the pointer inside alore_nmpc_batch
    int per_problem(int N) const { return mult * (per_node ? (N + extra) : 1); }
    int mult;      // floats per node (or per problem when !per_node)
    bool per_node;
    int extra;     // nodes = N + extra
    bool is_int;
};

// every member of alore_nmpc_batch with its per-problem element count
inline const Member kMembers[] = {
    {offsetof(alore_nmpc_batch, x), 3, true, 1, false},
    {offsetof(alore_nmpc_batch, u), 2, true, 0, false},
    {offsetof(alore_nmpc_batch, od), 3, true, 1, false},
    {offsetof(alore_nmpc_batch, y), 5, true, 0, false},
    {offsetof(alore_nmpc_batch, yN), 3, false, 0, false},
    {offsetof(alore_nmpc_batch, W), 25, true, 0, false},
    {offsetof(alore_nmpc_batch, WN), 9, false, 0, false},
    {offsetof(alore_nmpc_batch, x0), 3, false, 0, false},
    {offsetof(alore_nmpc_batch, lbValues), 2, true, 0, false},
    {offsetof(alore_nmpc_batch, ubValues), 2, true, 0, false},
    {offsetof(alore_nmpc_batch, dual), 2, true, 0, false},
    {offsetof(alore_nmpc_batch, status), 1, false, 0, true},
    {offsetof(alore_nmpc_batch, n_iter), 1, false, 0, true},
    {offsetof(alore_nmpc_batch, kkt), 1, false, 0, false},
    {offsetof(alore_nmpc_batch, obj), 1, false, 0, false},
};
constexpr int kNumMembers = sizeof(kMembers) / sizeof(kMembers[0]);

inline void*& member_ptr(alore_nmpc_batch* b, const Member& m)
{
    return *reinterpret_cast<void**>(reinterpret_cast<char*>(b) + m.offset);
}
inline void* member_ptr(const alore_nmpc_batch* b, const Member& m)
{
    return *reinterpret_cast<void* const*>(reinterpret_cast<const char*>(b) + m.offset);
}

inline bool batch_complete(const alore_nmpc_batch* b)
{
    for (int i = 0; i < kNumMembers; ++i) {
        const size_t off = kMembers[i].offset;
        if (off == offsetof(alore_nmpc_batch, kkt) || off == offsetof(alore_nmpc_batch, obj)) continue; // optional
        if (!member_ptr(b, kMembers[i])) return false;
    }
    return true;
}

// Host memory the runtime can DMA from directly (hipHostMalloc / hipHostRegister)?
inline bool host_is_pinned(const void* p)
{
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError(); // an unregistered pointer is reported as an error: not one of ours
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

inline int grow_stage(alore_nmpc_handle h, char*& buf, size_t& cap, size_t need)
{
    if (need <= cap) return ALORE_NMPC_OK;
    if (buf) (void)hipHostFree(buf);
    buf = nullptr; cap = 0;
    hipError_t e = hipHostMalloc((void**)&buf, need, hipHostMallocDefault);
    if (e != hipSuccess) return fail(h, ALORE_NMPC_E_NOMEM, "hipHostMalloc (staging)", e);
    cap = need;
    return ALORE_NMPC_OK;
}

// One launch for one batch (nmpc_capi.hip); B_in_flight = problems of all launches that run concurrently with it (0: only this one).
// `co` (alore_nmpc_closed_loop_run): the sampler of the next tick, to run in the same grid when the mapping has such a build;
// *co_done says whether it did
int rti_one(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, int n_sqp, void* stream, int B_in_flight, const nmpc::AheadSampler* co = nullptr,
            bool* co_done = nullptr, const nmpc::PlantAhead* plant = nullptr);

// What every sampler of the closed loops has in front of it (nmpc_refs_capi.hip): while the handle has an outstanding pending start
// time below `now`, the promotion for `now` over all robots of the store; otherwise nothing is enqueued
int promote_if_due(alore_nmpc_handle h, double now, hipStream_t s);

} // namespace nmpc_capi
#endif
