// fleet_manager.hip -- the kernels behind alore_backend_manager_* (rules, deviations and the slab: fleet_manager.h).
//
// One lane per robot, 256 lanes a workgroup.  The slab is structure of arrays, so a wavefront reads and writes whole lines; a lane
// loads its robot, runs the header's function and stores the robot again.  No LDS, no scratch, no allocation, nothing waits.
//   manager_request_kernel    start_callback / goal_callback
//   manager_begin_kernel      the head of MainThread: who plans, FRESH or REPLAN, and the predicted time; resets the five masks
//   manager_starts_kernel     behind alore_backend_predicted_state_device: the start state of FRESH robots into the predicted-state
//                             rows, the predicted pose of REPLAN robots into plan_start_xytheta, start_yaw / end_yaw for set_paths
//   manager_end_kernel        the rest of MainThread: what became of the plans, the delivery masks, the finish rule
//   manager_next_legs_kernel  the next leg of a mission for robots that are IDLE without a goal
// COUNTERS.  Every lane has the EV_* bits of what the call did to its robot; a wavefront counts each bit by ballot and pop-count and
// lane 0 adds the count with one integer atomic per counter that moved: integer sums, the same whatever the order.
#include "fleet_manager.h"

namespace fleet {
namespace {

__device__ inline bool selected(const int* mask, int stride, int b) { return !mask || *(const int*)((const char*)mask + (size_t)b * stride) != 0; }

// all 64 lanes of the wavefront get here, with ev = 0 for a lane without a robot
__device__ inline void count_events(int* counters, int ev)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const int n = __popcll(__ballot((ev >> k) & 1));
        if (lane == 0 && n) atomicAdd(&counters[k], n);
    }
}

__global__ void __launch_bounds__(256) manager_request_kernel(Slab s, int count, const double* start, const double* goal, int stride, const int* mask,
                                                               int mask_stride)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    int refused = 0;
    if (b < count && selected(mask, mask_stride, b)) {
        Robot r = load(s, b);
        refused = request(r, start ? (const double*)((const char*)start + (size_t)b * stride) : nullptr,
                          goal ? (const double*)((const char*)goal + (size_t)b * stride) : nullptr);
        store(s, b, r);
    }
    // 0, 1 or 2 refusals a robot
    const int lane = threadIdx.x & 63;
    const int n = __popcll(__ballot(refused >= 1)) + __popcll(__ballot(refused >= 2));
    if (lane == 0 && n) atomicAdd(&s.counters[6], n);
}

__global__ void __launch_bounds__(256) manager_begin_kernel(Slab s, Params P, Map m, int count, double now, const double* poses, int pose_stride,
                                                             const int* collision, int collision_stride)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    int ev = 0;
    if (b < count) {
        Robot r = load(s, b);
        const double* p = (const double*)((const char*)poses + (size_t)b * pose_stride);
        const double pose[3] = {p[0], p[1], 0.0};
        const bool inside = P.stop_inside_obstacle && r.have_goal && inside_obstacle(m.dist, m.nx, m.ny, m.x_lo, m.y_lo, m.x_hi, m.y_hi, m.res, pose[0], pose[1]);
        const bool hit = collision && selected(collision, collision_stride, b);
        Flags f;
        ev = begin(r, P, now, pose, inside, hit, f);
        store(s, b, r);
        store_flags(s, b, f);
    }
    count_events(s.counters, ev);
}

__global__ void __launch_bounds__(256) manager_starts_kernel(Slab s, int count, double* xytheta, double* vaj, double* oaj, double* start_yaw,
                                                              double* end_yaw)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= count) return;
    const int action = s.action[b];
    const size_t B = (size_t)s.B;
    if (action == ACT_FRESH) {
        for (int k = 0; k < 3; ++k) {
            xytheta[(size_t)b * 3 + k] = s.start[k * B + b];
            vaj[(size_t)b * 3 + k] = 0.0;
            oaj[(size_t)b * 3 + k] = 0.0;
        }
    } else if (action == ACT_REPLAN) { // :588
        for (int k = 0; k < 3; ++k) s.plan_start_xytheta[k * B + b] = xytheta[(size_t)b * 3 + k];
    }
    if (start_yaw) start_yaw[b] = s.plan_start_xytheta[2 * B + b];
    if (end_yaw) end_yaw[b] = s.goal[2 * B + b];
}

__global__ void __launch_bounds__(256) manager_end_kernel(Slab s, Params P, int count, double now, const int* search_status, const int* build_status,
                                                           const int* plan_ok, const double* T, int T_stride, const int* n_pieces)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    int ev = 0;
    if (b < count) {
        Robot r = load(s, b);
        Flags f = load_flags(s, b);
        double duration = 0.0;
        int st = SEARCH_OK, bs = BUILD_OK, ok = 0;
        if (!r.returned && r.action != ACT_NONE) { // the statuses of a robot that did not plan are never read
            st = search_status[b];
            bs = build_status[b];
            ok = plan_ok[b];
            int n = n_pieces[b];
            n = n < 0 ? 0 : (n > T_stride ? T_stride : n);
            duration = total_duration(T + (size_t)b * T_stride, n);
        }
        ev = end(r, P, now, st, bs, ok, duration, f);
        store(s, b, r);
        store_flags(s, b, f);
    }
    count_events(s.counters, ev);
}

__global__ void __launch_bounds__(256) manager_next_legs_kernel(Slab s, int count, const double* poses, int pose_stride, const int* task_status,
                                                                 const int* n_order, const double* leg_goal_xy, const double* leg_yaw, int reset_legs)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= count) return;
    Robot r = load(s, b);
    const double* p = (const double*)((const char*)poses + (size_t)b * pose_stride);
    const double pose[3] = {p[0], p[1], p[2]};
    if (r.state != IDLE || r.have_goal) return;
    next_leg(r, task_status[b], n_order[b], leg_goal_xy + (size_t)b * MAX_LEGS * 2, leg_yaw + (size_t)b * MAX_LEGS, pose, reset_legs != 0);
    store(s, b, r);
}

inline dim3 grid_of(int count) { return dim3((unsigned)((count + 255) / 256)); }

} // namespace

hipError_t request_enqueue(const Slab& s, int count, const double* start, const double* goal, int stride, const int* mask, int mask_stride, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(s.counters + 6, 0, sizeof(int), st); // the refusals of THIS call
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(manager_request_kernel, grid_of(count), dim3(256), 0, st, s, count, start, goal, stride, mask, mask_stride);
    return hipGetLastError();
}

hipError_t begin_enqueue(const Slab& s, const Params& P, const Map& m, int count, double now, const double* poses, int pose_stride, const int* collision,
                         int collision_stride, hipStream_t st)
{
    hipLaunchKernelGGL(manager_begin_kernel, grid_of(count), dim3(256), 0, st, s, P, m, count, now, poses, pose_stride, collision, collision_stride);
    return hipGetLastError();
}

hipError_t starts_enqueue(const Slab& s, int count, double* xytheta, double* vaj, double* oaj, double* start_yaw, double* end_yaw, hipStream_t st)
{
    hipLaunchKernelGGL(manager_starts_kernel, grid_of(count), dim3(256), 0, st, s, count, xytheta, vaj, oaj, start_yaw, end_yaw);
    return hipGetLastError();
}

hipError_t end_enqueue(const Slab& s, const Params& P, int count, double now, const int* search_status, const int* build_status, const int* plan_ok,
                       const double* T, int T_stride, const int* n_pieces, hipStream_t st)
{
    hipLaunchKernelGGL(manager_end_kernel, grid_of(count), dim3(256), 0, st, s, P, count, now, search_status, build_status, plan_ok, T, T_stride, n_pieces);
    return hipGetLastError();
}

hipError_t next_legs_enqueue(const Slab& s, int count, const double* poses, int pose_stride, const int* task_status, const int* n_order,
                             const double* leg_goal_xy, const double* leg_yaw, int reset_legs, hipStream_t st)
{
    hipLaunchKernelGGL(manager_next_legs_kernel, grid_of(count), dim3(256), 0, st, s, count, poses, pose_stride, task_status, n_order, leg_goal_xy, leg_yaw,
                       reset_legs);
    return hipGetLastError();
}

} // namespace fleet
