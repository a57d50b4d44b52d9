// flat_traj_build.hip -- FlatTrajData from way-point paths on the device (gfx950): what alore_backend_set_paths launches.
//
// build_problems_kernel: one wavefront per path, node j of its at most 63 nodes on lane j, the arithmetic of flat_traj_build.h.
// The headings are a chain (each is normalised against the one before): the directions come from one atan2 per lane, the chain
// is walked by all lanes together.  Plain and weighted lengths are wave prefix sums on the DPP path (fixed order), the cut node
// is the first set bit of one ballot, lane 0 computes the trapezoid's duration, lane j then takes sample j: it finds its segment
// by walking the weighted lengths (broadcast lane by lane) and fetches the two nodes with per-lane shuffles.  Skipped samples are
// compacted by a ballot prefix.  No LDS, no barrier, no scratch; every cross-lane operation is in wave-uniform control flow.
// Nothing of a slot is written before the path is known to build; a slot that the mask leaves out is not touched at all.
//
// launch_order_kernel: d_order = the slots by piece count, most pieces first, stable in the slot index -- the order of the
// std::stable_sort in alore_backend_set_problems -- by a counting sort in one workgroup (arithmetic and shapes in launch_order.h):
// every thread owns a contiguous run of slots, counts its pieces into its own row of an LDS histogram, a prefix per bucket over the
// threads (slot order) and over the buckets (descending) gives every thread its first position per bucket.
#include "backend_kernels.h"
#include "flat_traj_build.h"
#include "launch_order.h"

namespace backend {
namespace {

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double old, double x)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(x), CTRL, ROW_MASK, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(x), CTRL, ROW_MASK, 0xF, false);
    return __hiloint2double(hi, lo);
}
// inclusive prefix sum over the 64 lanes: row_shr 1, 2, 4, 8, then row_bcast15 / row_bcast31 (the scan of backend_kernels.hip)
__device__ __forceinline__ double wave_prefix(double v)
{
    v += dpp_f64<0x111, 0xF>(0.0, v);
    v += dpp_f64<0x112, 0xF>(0.0, v);
    v += dpp_f64<0x114, 0xF>(0.0, v);
    v += dpp_f64<0x118, 0xF>(0.0, v);
    v += dpp_f64<0x142, 0xA>(0.0, v);
    v += dpp_f64<0x143, 0xC>(0.0, v);
    return v;
}
__device__ __forceinline__ double lane_of(double v, int src) { return __shfl(v, src); }

} // namespace

__global__ __launch_bounds__(64) void build_problems_kernel(const BuildArgs* __restrict__ gp)
{
    namespace ft = flat_traj;
    const BuildArgs& a = *gp;
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= a.count) return;
    if (a.mask && *(const int*)((const char*)a.mask + (size_t)b * a.mask_stride) == 0) {
        if (lane == 0) a.status[b] = ft::MASKED_OUT;
        return;
    }
    const int P = a.P, K = a.K, n = __builtin_amdgcn_readfirstlane(a.n_points[b]);
    if (n < 2 || n > K || n > ft::MAX_POINTS) {
        if (lane == 0) a.status[b] = ft::E_POINTS;
        return;
    }
    // the front-end parameters of the slot's class (alore_backend_set_classes with fe), or the call's
    const ft::Params fe = a.fe_classes ? a.fe_classes[__builtin_amdgcn_readfirstlane(a.class_of[b])] : a.fe;
    const double* xy = a.xy + (size_t)b * K * 2;
    const double start_yaw = a.start_yaw[b], end_yaw = a.end_yaw[b];
    const double v0 = a.start_vaj ? a.start_vaj[(size_t)b * 3] : 0.0;
    int nn = 2 * n + 1;

    // ---- getSampleTraj: node `lane`
    const double dir = lane < n - 1 ? ft::segment_heading(xy, lane) : end_yaw; // direction of segment `lane`; the final yaw after the last
    const double th = ft::first_heading(xy, start_yaw), th2 = ft::first_heading_again(xy, start_yaw);
    ft::Node nd{0.0, 0.0, 0.0, 0.0, 0.0};
    if (lane < nn) {
        const int pi = ft::node_point(lane);
        nd.x = xy[2 * pi];
        nd.y = xy[2 * pi + 1];
        if (lane >= 3 && (lane & 1)) nd.ds = ft::drive_length(xy, pi);
    }
    if (lane == 0) nd.yaw = start_yaw;
    if (lane == 1) { nd.yaw = th; nd.dyaw = th - start_yaw; }
    if (lane == 2) { nd.yaw = th2; nd.dyaw = th2 - start_yaw; }
    double H = th2;
    for (int i = 1; i < n; ++i) { // wave-uniform: the chain of headings
        const double Hn = ft::next_heading(H, lane_of(dir, i));
        if (lane == 2 * i + 1) nd.yaw = H;
        if (lane == 2 * i + 2) { nd.yaw = Hn; nd.dyaw = Hn - H; }
        H = Hn;
    }

    // ---- getTrajsWithTime: lengths, the cut, weighted lengths
    double len = wave_prefix(nd.ds);
    double len_before = __shfl_up(len, 1);
    if (lane == 0) len_before = 0.0;
    const unsigned long long cuts = __ballot(lane >= 1 && lane < nn && ft::cuts_here(fe, len_before, nd.ds));
    const int if_cut = cuts != 0;
    {
        const int kc = if_cut ? __ffsll((long long)cuts) - 1 : 63;
        const int src = kc > 0 ? kc - 1 : 0;
        const ft::Node former{lane_of(nd.x, src), lane_of(nd.y, src), lane_of(nd.yaw, src), lane_of(nd.dyaw, src), lane_of(nd.ds, src)};
        if (if_cut) {
            nn = kc + 1;
            if (lane == kc) {
                nd = ft::cut_node(fe, former, nd, len_before);
                len = len_before + nd.ds;
            }
            if (lane > kc) nd = ft::Node{0.0, 0.0, 0.0, 0.0, 0.0};
        }
    }
    const double wl = wave_prefix(lane >= 1 && lane < nn ? ft::node_weight(fe, nd.dyaw, nd.ds) : 0.0);
    const double all_w = lane_of(wl, nn - 1);
    const ft::Node last{lane_of(nd.x, nn - 1), lane_of(nd.y, nn - 1), lane_of(nd.yaw, nn - 1), 0.0, 0.0};
    const double all_len = lane_of(len, nn - 1);

    // ---- timing: one lane computes the trapezoid
    double total_t = 0.0;
    if (lane == 0) total_t = ft::evaluate_duration(all_w, v0, 0.0, fe.max_vel, fe.max_acc);
    total_t = lane_of(total_t, 0);
    const double sample_t = ft::sample_step(fe, total_t);
    double t = sample_t, t_mine = sample_t;
    for (int k = 0; k < 63; ++k) { // repeated addition, as the reference accumulates it: lane j keeps the j-th sum
        t += sample_t;
        if (lane == k + 1) t_mine = t;
    }
    const bool in_range = ft::sample_in_range(t_mine, total_t);
    const double arc = in_range ? ft::evaluate_length(t_mine, all_w, v0, 0.0, fe.max_vel, fe.max_acc) : 0.0;

    // ---- segment look-up: the first k >= 1 with wl[k] >= arc
    int k_mine = 0;
    for (int k = 1; k < nn; ++k) { // wave-uniform
        const double wk = lane_of(wl, k);
        if (k_mine == 0 && wk >= arc) k_mine = k;
    }
    const bool taken = in_range && k_mine > 0;
    const int k1 = k_mine > 0 ? k_mine : 1, k0 = k1 - 1;
    const ft::Node n0{lane_of(nd.x, k0), lane_of(nd.y, k0), lane_of(nd.yaw, k0), 0.0, 0.0};
    const ft::Node n1{lane_of(nd.x, k1), lane_of(nd.y, k1), 0.0, lane_of(nd.dyaw, k1), lane_of(nd.ds, k1)};
    const double wl0 = lane_of(wl, k0), wl1 = lane_of(wl, k1), len0 = lane_of(len, k0);

    // ---- compaction and the overflow test; nothing has been written so far
    const unsigned long long in_mask = __ballot(in_range), tk_mask = __ballot(taken);
    const int M = __popcll(tk_mask) + 1;
    if ((in_mask >> 63) != 0 || M > P) { // the samples do not end inside the wavefront, or more pieces than the slot holds
        if (lane == 0) a.status[b] = ft::E_PIECES;
        return;
    }
    const int rank = __popcll(tk_mask & ((1ull << lane) - 1ull));
    double* inner = a.inner + (size_t)b * (P - 1) * 2;
    double* pos = a.positions + (size_t)b * P * 2;
    if (taken) {
        const ft::Sample q = ft::interpolate(arc, wl0, wl1, len0, n0, n1);
        inner[2 * rank] = q.yaw;
        inner[2 * rank + 1] = q.s;
        pos[2 * rank] = q.x;
        pos[2 * rank + 1] = q.y;
    }
    // the rest of the rows is zero, as alore_backend_set_problems uploads it
    for (int v = 2 * (M - 1) + lane; v < 2 * (P - 1); v += 64) inner[v] = 0.0;
    for (int v = 2 * M + lane; v < 2 * P; v += 64) pos[v] = 0.0;
    if (lane == 0) {
        pos[2 * (M - 1)] = last.x;
        pos[2 * (M - 1) + 1] = last.y;
        a.M[b] = M;
        a.if_cut[b] = if_cut;
        a.init_T[b] = sample_t;
        double* head = a.head + (size_t)b * 6;
        double* tail = a.tail + (size_t)b * 6;
        head[0] = start_yaw;
        head[1] = a.start_oaj ? a.start_oaj[(size_t)b * 3] : 0.0;
        head[2] = a.start_oaj ? a.start_oaj[(size_t)b * 3 + 1] : 0.0;
        head[3] = 0.0;
        head[4] = a.start_vaj ? a.start_vaj[(size_t)b * 3] : 0.0;
        head[5] = a.start_vaj ? a.start_vaj[(size_t)b * 3 + 1] : 0.0;
        tail[0] = last.yaw; tail[1] = 0.0; tail[2] = 0.0;
        tail[3] = all_len; tail[4] = 0.0; tail[5] = 0.0;
        a.start_xy[(size_t)b * 2] = xy[0];
        a.start_xy[(size_t)b * 2 + 1] = xy[1];
        a.final_xy[(size_t)b * 2] = last.x;
        a.final_xy[(size_t)b * 2 + 1] = last.y;
        a.sxyt[(size_t)b * 3] = xy[0];
        a.sxyt[(size_t)b * 3 + 1] = xy[1];
        a.sxyt[(size_t)b * 3 + 2] = start_yaw;
        a.status[b] = ft::BUILT;
    }
}

// the shapes are those of launch_order.h: 256 threads and 33 buckets for the 16- and 32-piece builds, 128 and 65 for the 64-piece build
template <int BUCKETS, int THREADS>
__global__ __launch_bounds__(THREADS) void launch_order_kernel(const BuildArgs* __restrict__ gp)
{
    namespace lo = launch_order;
    __shared__ int hist[THREADS][BUCKETS]; // [thread][pieces] -> first position of that thread's slots with that many pieces
    __shared__ int total[BUCKETS];
    const int count = gp->count, tid = threadIdx.x;
    const int* __restrict__ Mg = gp->M;
    int* __restrict__ order = gp->order;
    int first, last;
    lo::run_of(tid, count, THREADS, &first, &last);
    lo::count_run<BUCKETS>(Mg, first, last, hist[tid]);
    __syncthreads();
    if (tid < BUCKETS) total[tid] = lo::prefix_threads<BUCKETS>(hist, THREADS, tid);
    __syncthreads();
    if (tid == 0) lo::prefix_buckets<BUCKETS>(total);
    __syncthreads();
    lo::scatter_run<BUCKETS>(Mg, first, last, hist[tid], total, order);
}

hipError_t build_problems(const BuildArgs* d_args, int count, int P, hipStream_t s)
{
    void* args[] = {&d_args};
    hipError_t e = hipLaunchKernel((const void*)build_problems_kernel, dim3(count), dim3(64), args, 0, s);
    if (e != hipSuccess) return e;
    namespace lo = launch_order;
    if (P <= 32) e = hipLaunchKernel((const void*)launch_order_kernel<lo::buckets_of(32), lo::threads_of(32)>, dim3(1), dim3(lo::threads_of(32)), args, 0, s);
    else e = hipLaunchKernel((const void*)launch_order_kernel<lo::buckets_of(64), lo::threads_of(64)>, dim3(1), dim3(lo::threads_of(64)), args, 0, s);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

} // namespace backend
