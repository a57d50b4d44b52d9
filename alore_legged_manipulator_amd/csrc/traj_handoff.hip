// traj_handoff.hip -- promotion of pending trajectories on the device (rules and the run splitter: traj_handoff.h).
//
// Every robot has a pending slot beside its active slot in the trajectory store, both with the layout of nmpc::RefStore.  A promotion
// copies pending -> active for the robots whose pending entry is due and invalidates the pending entry.  It copies and does not
// switch an index: no sampler, plant or checkpoint builder reads through an indirection, and a handle that never uses a pending
// entry runs what it ran before.
//
// One wavefront per robot.  It reads the pending meta row and leaves at once when nothing is due; otherwise its lanes copy only the
// rows in use (n_pieces durations, n_pieces * 12 coefficients, n_ckpt * 2 checkpoint doubles) as 16-byte loads and stores, and the
// meta row last.  No LDS, no scratch.  Stream order is the only ordering: a sampler on another stream is the caller's to order.
#include "nmpc_kernels.h"

#include <cstdint>

#include "traj_handoff.h"

namespace nmpc {

namespace {
// n doubles, dst and src at the same offset of two allocations of one layout (so both reach 16-byte alignment at the same element)
__device__ inline void copy_row(double* dst, const double* src, int n, int lane)
{
    int head = (int)((reinterpret_cast<uintptr_t>(src) >> 3) & 1);
    if (head > n) head = n;
    if (lane == 0 && head) dst[0] = src[0];
    const int pairs = (n - head) >> 1;
    const double2* s2 = reinterpret_cast<const double2*>(src + head);
    double2* d2 = reinterpret_cast<double2*>(dst + head);
    for (int i = lane; i < pairs; i += 64) d2[i] = s2[i];
    const int tail = head + 2 * pairs;
    if (lane == 0 && tail < n) dst[tail] = src[tail];
}
} // namespace

__global__ __launch_bounds__(256) void traj_promote_kernel(PromoteArgs a)
{
    const int t = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    if (t >= a.count) return;
    const int r = a.robots ? a.robots[t] : t;
    if (a.forced) { // only the slots that the build kernels behind this launch are going to write
        if (a.mask && *(const int*)((const char*)a.mask + (size_t)t * a.mask_stride) == 0) return;
        if (a.ok && a.ok[t] == 0) return;
    }
    double* pm = a.pen.meta + (size_t)r * 8;
    if (!traj_handoff::promote_due(pm[6] != 0.0, pm[0], a.now, a.forced != 0)) return;
    int n = (int)pm[4], nck = (int)pm[5];
    n = n < 0 ? 0 : (n > a.act.P ? a.act.P : n);
    nck = nck < 0 ? 0 : (nck > a.act.C ? a.act.C : nck);
    copy_row(a.act.dur + (size_t)r * a.act.P, a.pen.dur + (size_t)r * a.act.P, n, lane);
    copy_row(a.act.coef + (size_t)r * a.act.P * 12, a.pen.coef + (size_t)r * a.act.P * 12, n * 12, lane);
    copy_row(a.act.ckpt + (size_t)r * a.act.C * 2, a.pen.ckpt + (size_t)r * a.act.C * 2, nck * 2, lane);
    if (lane < 4) { // the meta row last (64-byte rows of 256-byte aligned slabs); lane 3 holds (valid, -) and clears the pending flag
        const double2 v = reinterpret_cast<const double2*>(pm)[lane];
        reinterpret_cast<double2*>(a.act.meta + (size_t)r * 8)[lane] = v;
        if (lane == 3) pm[6] = 0.0;
    }
    if (lane == 0) a.promotions[r] += 1;
}

// ---- the controllers' side of an emergency stop (nmpc_controller/src/mpc.cpp:279-294, mpc_controller/src/mpc.cpp:616-632):
//      receive_traj_ = false and a zero command.  One lane per robot, ordinary stores, no LDS.
namespace {
__device__ inline bool stop_selected(const int* mask, int stride, int t) { return !mask || *(const int*)((const char*)mask + (size_t)t * stride) != 0; }
} // namespace

__global__ __launch_bounds__(256) void traj_stop_kernel(double* act_meta, double* pen_meta, int* stopped, const int* mask, int mask_stride, int count)
{
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= count || !stop_selected(mask, mask_stride, t)) return;
    act_meta[(size_t)t * 8 + 6] = 0.0;
    if (pen_meta) pen_meta[(size_t)t * 8 + 6] = 0.0;
    stopped[t] = 1;
}

__global__ __launch_bounds__(256) void plant_stop_kernel(double* state, double* desired, int width, const int* mask, int mask_stride, int count)
{
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= count || !stop_selected(mask, mask_stride, t)) return;
    for (int k = 0; k < width; ++k) {
        state[(size_t)t * width + k] = 0.0;
        if (desired) desired[(size_t)t * width + k] = 0.0;
    }
}

__global__ __launch_bounds__(256) void stop_hold_kernel(float* u, const double* act_meta, int* stopped, int B, int N, int node)
{
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= B || !stopped[r]) return;
    if (act_meta[(size_t)r * 8 + 6] != 0.0) { stopped[r] = 0; return; } // a promotion since: the robot tracks again
    u[((size_t)r * N + node) * 2] = 0.f;
    u[((size_t)r * N + node) * 2 + 1] = 0.f;
}

hipError_t launch_traj_stop(double* act_meta, double* pen_meta, int* stopped, const int* mask, int mask_stride, int count, hipStream_t st)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(traj_stop_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, act_meta, pen_meta, stopped, mask, mask_stride, count);
    return hipGetLastError();
}

hipError_t launch_plant_stop(double* state, double* desired, int width, const int* mask, int mask_stride, int count, hipStream_t st)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(plant_stop_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, state, desired, width, mask, mask_stride, count);
    return hipGetLastError();
}

hipError_t launch_stop_hold(float* u, const double* act_meta, int* stopped, int B, int N, int node, hipStream_t st)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(stop_hold_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, u, act_meta, stopped, B, N, node);
    return hipGetLastError();
}

hipError_t launch_traj_promote(const PromoteArgs& a, hipStream_t st)
{
    if (a.count <= 0) return hipSuccess;
    hipLaunchKernelGGL(traj_promote_kernel, dim3((unsigned)((a.count + 3) / 4)), dim3(256), 0, st, a);
    return hipGetLastError();
}

} // namespace nmpc
