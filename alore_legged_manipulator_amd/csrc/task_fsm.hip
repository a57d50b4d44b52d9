// task_fsm.hip -- the ALORE task FSM of B robots on the device and the C ABI of include/alore_fsm.h.
// One robot per lane, a workgroup is ONE wavefront of 64 lanes, as in arm_ik.hip.  A lane runs fsm::tick_head of task_fsm.h on its
// robot's words; a lane whose robot is in GRASPING then runs fsm::tick_grasp, i.e. z1::grasp_step with the IK inside it, in the SAME
// launch: the branch is taken per wavefront (__any), so a wavefront without a grasping robot leaves without entering the IK, and
// one with some runs it under the EXEC mask of those lanes.  A second launch would cost its dispatch on every tick to save
// nothing: the early exit is per wavefront either way, and the registers of the IK are only held by wavefronts that exist anyway.
// The state is a structure of arrays next to the arm's grasp slab (arm_handle.h); sequences, paths and targets are rows per robot.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/alore_fsm.h"
#include "arm_handle.h"
#include "task_fsm.h"

static_assert(sizeof(alore_fsm_params) == sizeof(fsm::Params), "alore_fsm_params mirrors fsm::Params");
static_assert(ALORE_FSM_MAX_TASKS == fsm::MAX_TASKS, "ALORE_FSM_MAX_TASKS");

namespace fsm {

constexpr int LANES = arm::LANES;
constexpr int N_COUNTERS = 2, REFUSED_SEQUENCES = 0, REFUSED_PATHS = 1;

// the FSM's device slab.  words: ROBOT_INTS rows of [B] in the order of fsm::Robot
struct Slab {
    int B, max_tasks, max_objects, max_pts;
    int *words, *object_sequence, *target_sequence, *counters;
    double *reach_threshold, *object_vel_cmd, *start_xytheta, *goal_xytheta, *object_pose_used, *control, *robot_path, *object_path,
        *target_poses;
};

template <typename T> __device__ inline const T* row(const T* base, int b, int stride_bytes)
{
    return reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + (size_t)b * (size_t)stride_bytes);
}
__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ inline void load(const Slab& s, int b, Robot& r, int* seq)
{
    int* w = &r.task_state;
    for (int i = 0; i < ROBOT_INTS; ++i) w[i] = s.words[(size_t)i * s.B + b];
    r.reach_threshold = s.reach_threshold[b];
    for (int i = 0; i < 3; ++i) {
        r.object_vel_cmd[i] = s.object_vel_cmd[(size_t)b * 3 + i];
        r.start_xytheta[i] = s.start_xytheta[(size_t)b * 3 + i];
        r.goal_xytheta[i] = s.goal_xytheta[(size_t)b * 3 + i];
    }
    for (int i = 0; i < 4; ++i) r.object_pose_used[i] = s.object_pose_used[(size_t)b * 4 + i];
    for (int i = 0; i < MAX_TASKS; ++i) {
        seq[i] = s.object_sequence[(size_t)b * MAX_TASKS + i];
        seq[MAX_TASKS + i] = s.target_sequence[(size_t)b * MAX_TASKS + i];
    }
    // the words are exposed by the device view: what indexes memory is clamped where it is read
    r.task_num = clampi(r.task_num, 0, MAX_TASKS - 1);
    r.object_type = clampi(r.object_type, 0, s.max_objects - 1);
    r.target_type = clampi(r.target_type, 0, s.max_tasks - 1);
    r.n_robot_path = clampi(r.n_robot_path, 0, s.max_pts);
    r.n_object_path = clampi(r.n_object_path, 0, s.max_pts);
    r.robot_path_index = r.robot_path_index < 0 ? 0 : r.robot_path_index;
    r.object_path_index = r.object_path_index < 0 ? 0 : r.object_path_index;
    for (int i = 0; i < MAX_TASKS; ++i) {
        seq[i] = clampi(seq[i], 0, s.max_objects - 1);
        seq[MAX_TASKS + i] = clampi(seq[MAX_TASKS + i], 0, s.max_tasks - 1);
    }
}
__device__ inline void store(const Slab& s, int b, const Robot& r)
{
    const int* w = &r.task_state;
    for (int i = 0; i < ROBOT_INTS; ++i) s.words[(size_t)i * s.B + b] = w[i];
    s.reach_threshold[b] = r.reach_threshold;
    for (int i = 0; i < 3; ++i) {
        s.object_vel_cmd[(size_t)b * 3 + i] = r.object_vel_cmd[i];
        s.start_xytheta[(size_t)b * 3 + i] = r.start_xytheta[i];
        s.goal_xytheta[(size_t)b * 3 + i] = r.goal_xytheta[i];
    }
    for (int i = 0; i < 4; ++i) s.object_pose_used[(size_t)b * 4 + i] = r.object_pose_used[i];
}
__device__ inline void load_grasp(const arm::GraspSlab& s, int b, z1::Grasp& g)
{
    g.k = s.k[b]; g.d_gripper = s.d_gripper[b]; g.gripper_ang = s.gripper_ang[b]; g.err_norm = s.err_norm[b];
    g.grasp_time = s.grasp_time[b]; g.flag = s.flag[b]; g.stable = s.stable[b]; g.done = s.done[b];
    g.ik_iterations = s.ik_iterations[b]; g.ik_status = s.ik_status[b];
    for (int i = 0; i < 7; ++i) g.joint_cmd[i] = s.joint_cmd[(size_t)b * 7 + i];
    for (int i = 0; i < 3; ++i) g.robot_vel_cmd[i] = s.robot_vel_cmd[(size_t)b * 3 + i];
}
__device__ inline void store_grasp(const arm::GraspSlab& s, int b, const z1::Grasp& g)
{
    s.k[b] = g.k; s.d_gripper[b] = g.d_gripper; s.gripper_ang[b] = g.gripper_ang; s.err_norm[b] = g.err_norm;
    s.grasp_time[b] = g.grasp_time; s.flag[b] = g.flag; s.stable[b] = g.stable; s.done[b] = g.done;
    s.ik_iterations[b] = g.ik_iterations; s.ik_status[b] = g.ik_status;
    for (int i = 0; i < 7; ++i) s.joint_cmd[(size_t)b * 7 + i] = g.joint_cmd[i];
    for (int i = 0; i < 3; ++i) s.robot_vel_cmd[(size_t)b * 3 + i] = g.robot_vel_cmd[i];
}

__global__ __launch_bounds__(LANES) void tick_kernel(z1::Params P, Params F, int count, const z1::Class* classes, int n_classes, const int* class_of,
                                                     const double* com, arm::GraspSlab gs, Slab s, const double* robot_pose, int pose_stride,
                                                     const double* object_poses, int objects_stride, const double* arm_base_pose, int base_stride,
                                                     const double* joint_positions, int joint_stride)
{
    const int b = blockIdx.x * LANES + threadIdx.x;
    if (b >= count) return;
    const int ci = clampi(class_of[b], 0, n_classes - 1);
    const z1::Class c = classes[ci];
    const double off[2] = {com[2 * ci], com[2 * ci + 1]};
    Robot r;
    z1::Grasp g;
    int seq[2 * MAX_TASKS];
    load(s, b, r, seq);
    load_grasp(gs, b, g);
    double pose[4];
    const double* pr = row(robot_pose, b, pose_stride);
    for (int i = 0; i < 4; ++i) pose[i] = pr[i];
    const size_t path_at = (size_t)b * s.max_pts * 2;
    const int need = tick_head(F, c, off, r, g, seq, s.robot_path + path_at, s.object_path + path_at,
                               s.target_poses + (size_t)b * s.max_tasks * 4, pose, row(object_poses, b, objects_stride));
    if (__any(need)) { // a wavefront without a robot in GRASPING skips the IK altogether
        if (need) {
            double base[7], jp[7];
            const double *br = row(arm_base_pose, b, base_stride), *jr = row(joint_positions, b, joint_stride);
            for (int i = 0; i < 7; ++i) base[i] = br[i];
            for (int i = 0; i < 7; ++i) jp[i] = jr[i];
            tick_grasp(F, P, c, r, g, pose, base, jp);
        }
    }
    store(s, b, r);
    store_grasp(gs, b, g);
    double ctl[ALORE_FSM_CONTROL_ROW];
    control_row(r, g, ctl);
    for (int i = 0; i < ALORE_FSM_CONTROL_ROW; ++i) s.control[(size_t)b * ALORE_FSM_CONTROL_ROW + i] = ctl[i];
}

__global__ __launch_bounds__(LANES) void reset_kernel(z1::Params P, Params F, int count, const int* mask, arm::GraspSlab gs, Slab s)
{
    const int b = blockIdx.x * LANES + threadIdx.x;
    if (b >= count || (mask && mask[b] == 0)) return;
    Robot r;
    z1::Grasp g;
    int seq[2 * MAX_TASKS];
    reset(F, r, seq);
    z1::grasp_initial(P, g);
    store(s, b, r);
    store_grasp(gs, b, g);
    for (int i = 0; i < MAX_TASKS; ++i) {
        s.object_sequence[(size_t)b * MAX_TASKS + i] = clampi(seq[i], 0, s.max_objects - 1);
        s.target_sequence[(size_t)b * MAX_TASKS + i] = clampi(seq[MAX_TASKS + i], 0, s.max_tasks - 1);
    }
    double ctl[ALORE_FSM_CONTROL_ROW];
    control_row(r, g, ctl);
    for (int i = 0; i < ALORE_FSM_CONTROL_ROW; ++i) s.control[(size_t)b * ALORE_FSM_CONTROL_ROW + i] = ctl[i];
}

__global__ __launch_bounds__(LANES) void set_targets_kernel(int count, Slab s, const double* targets, int stride)
{
    const int b = blockIdx.x * LANES + threadIdx.x;
    if (b >= count) return;
    const double* t = row(targets, b, stride);
    for (int i = 0; i < s.max_tasks * 4; ++i) s.target_poses[(size_t)b * s.max_tasks * 4 + i] = t[i];
}

__global__ __launch_bounds__(LANES) void set_sequences_kernel(int count, Slab s, const int* order, int order_stride, const int* n_order, const int* mask)
{
    const int b = blockIdx.x * LANES + threadIdx.x;
    if (b >= count || (mask && mask[b] == 0)) return;
    Robot r;
    int seq[2 * MAX_TASKS], ord[2 * MAX_TASKS];
    load(s, b, r, seq);
    const int n = n_order[b];
    const int* o = row(order, b, order_stride);
    for (int i = 0; i < 2 * MAX_TASKS; ++i) ord[i] = (i < n && i < 2 * s.max_tasks) ? o[i] : 0; // nothing beyond the row is read
    if (!set_sequence(r, seq, ord, n, s.max_tasks, s.max_objects)) {
        atomicAdd(s.counters + REFUSED_SEQUENCES, 1);
        return;
    }
    s.words[(size_t)2 * s.B + b] = r.n_tasks;
    s.words[(size_t)11 * s.B + b] = r.is_task_plan;
    for (int i = 0; i < MAX_TASKS; ++i) {
        s.object_sequence[(size_t)b * MAX_TASKS + i] = seq[i];
        s.target_sequence[(size_t)b * MAX_TASKS + i] = seq[MAX_TASKS + i];
    }
}

__global__ __launch_bounds__(LANES) void set_paths_kernel(int count, Slab s, const double* xy, int xy_stride, const int* n_points, const int* mask)
{
    const int b = blockIdx.x * LANES + threadIdx.x;
    if (b >= count || (mask && mask[b] == 0)) return;
    Robot r;
    int seq[2 * MAX_TASKS];
    load(s, b, r, seq);
    const int n = n_points[b];
    const int which = deliver_path(r, n, s.max_pts);
    if (which == 0) return; // untouched
    if (which < 0) {
        atomicAdd(s.counters + REFUSED_PATHS, 1);
        return;
    }
    const double* src = row(xy, b, xy_stride);
    double* dst = (which == 1 ? s.robot_path : s.object_path) + (size_t)b * s.max_pts * 2;
    for (int i = 0; i < 2 * n; ++i) dst[i] = src[i]; // n <= max_pts
    s.words[(size_t)0 * s.B + b] = r.task_state;
    if (which == 1) {
        s.words[(size_t)5 * s.B + b] = r.robot_path_index;
        s.words[(size_t)7 * s.B + b] = r.n_robot_path;
    } else {
        s.words[(size_t)6 * s.B + b] = r.object_path_index;
        s.words[(size_t)8 * s.B + b] = r.n_object_path;
    }
}

} // namespace fsm

// the order of the words in fsm::Robot, which the kernels above index by number
static_assert(offsetof(fsm::Robot, task_state) == 0 && offsetof(fsm::Robot, n_tasks) == 8 && offsetof(fsm::Robot, robot_path_index) == 20 &&
                  offsetof(fsm::Robot, object_path_index) == 24 && offsetof(fsm::Robot, n_robot_path) == 28 &&
                  offsetof(fsm::Robot, n_object_path) == 32 && offsetof(fsm::Robot, is_task_plan) == 44 && offsetof(fsm::Robot, request) == 56,
              "the word numbers of fsm::Robot");

// ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
struct alore_fsm_slab {
    fsm::Params F;
    fsm::Slab s;
    double* d_com;     // [ALORE_ARM_MAX_CLASSES][2]
    double* d_doubles; // the block of doubles: the slab, then the staging
    int* d_ints;
    double* d_stage;   // [B][stage_row] doubles: host inputs of a call with device_pointers == 0
    int* d_stage_int;  // [B][STAGE_INTS]
    int stage_row;
};

namespace {
constexpr int STAGE_INTS = 2 * fsm::MAX_TASKS + 2;

int fail(alore_arm* h, int code, const char* fmt, const char* a = "", long v = 0)
{
    static char g_err[256];
    std::snprintf(h ? h->err : g_err, 256, fmt, a, v);
    return code;
}
int hip_fail(alore_arm* h, hipError_t e, const char* what) { return fail(h, ALORE_ARM_E_HIP, "%s: HIP error %ld", what, (long)e); }
#define FSM_HIP(call)                                       \
    do {                                                    \
        hipError_t e_ = (call);                             \
        if (e_ != hipSuccess) return hip_fail(h, e_, #call); \
    } while (0)

bool bad_stride(int stride, int row_bytes, int unit) { return stride < row_bytes || stride % unit != 0; }
int grid(int count) { return (count + fsm::LANES - 1) / fsm::LANES; }
int check(alore_arm* h, const char* call, int count)
{
    if (!h) return fail(nullptr, ALORE_ARM_E_INVALID, "%s: NULL handle", call);
    if (!h->fsm) return fail(h, ALORE_ARM_E_INVALID, "%s: the handle has no FSM (alore_fsm_create first)", call);
    if (count < 0 || count > h->max_problems) return fail(h, ALORE_ARM_E_INVALID, "%s: count %ld is outside 0 .. max_problems", call, count);
    return ALORE_ARM_OK;
}
hipError_t upload(void* dst, size_t dst_row, const void* src, size_t stride, size_t width, int count, hipStream_t st)
{
    return hipMemcpy2DAsync(dst, dst_row, src, stride, width, (size_t)count, hipMemcpyHostToDevice, st);
}
void fsm_free(alore_arm* h)
{
    alore_fsm_slab* f = h->fsm;
    if (!f) return;
    (void)hipDeviceSynchronize();
    (void)hipFree(f->d_doubles);
    (void)hipFree(f->d_ints);
    (void)hipFree(f->d_com);
    delete f;
    h->fsm = nullptr;
    h->fsm_free = nullptr;
}
} // namespace

extern "C" {

void alore_fsm_default_params(alore_fsm_params* p)
{
    if (p) fsm::default_params(reinterpret_cast<fsm::Params*>(p));
}

int alore_fsm_create(alore_arm_handle h, const alore_fsm_params* params, int max_tasks, int max_objects, int max_path_points)
{
    if (!h) return fail(nullptr, ALORE_ARM_E_INVALID, "alore_fsm_create: NULL handle%s");
    if (h->fsm) return fail(h, ALORE_ARM_E_INVALID, "alore_fsm_create: the handle has an FSM already%s");
    fsm::Params F;
    fsm::default_params(&F);
    if (params) std::memcpy(&F, params, sizeof(F));
    if (max_tasks < 1 || max_tasks > fsm::MAX_TASKS) return fail(h, ALORE_ARM_E_INVALID, "alore_fsm_create: max_tasks %s must be 1 .. 10 (got %ld)", "", max_tasks);
    if (max_objects < 1 || max_objects > 4096) return fail(h, ALORE_ARM_E_INVALID, "alore_fsm_create: max_objects %s must be 1 .. 4096 (got %ld)", "", max_objects);
    if (max_path_points < 1 || max_path_points > 65536)
        return fail(h, ALORE_ARM_E_INVALID, "alore_fsm_create: max_path_points %s must be 1 .. 65536 (got %ld)", "", max_path_points);
    const int* ticks = &F.ticks_no_plan;
    for (int i = 0; i < 8; ++i)
        if (ticks[i] < 1) return fail(h, ALORE_ARM_E_INVALID, "alore_fsm_create: %severy tick count must be at least 1 (got %ld)", "", ticks[i]);
    alore_fsm_slab* f = new (std::nothrow) alore_fsm_slab();
    if (!f) return fail(h, ALORE_ARM_E_NOMEM, "alore_fsm_create: out of host memory%s");
    f->F = F;
    const size_t B = (size_t)h->max_problems, mp = (size_t)max_path_points, mt = (size_t)max_tasks, mo = (size_t)max_objects;
    size_t stage = 4 + 4 * mo + 7 + 7;
    if (stage < 2 * mp) stage = 2 * mp;
    if (stage < 4 * mt) stage = 4 * mt;
    f->stage_row = (int)stage;
    const size_t slab_doubles = B * (1 + 3 + 3 + 3 + 4 + ALORE_FSM_CONTROL_ROW + 4 * mp + 4 * mt);
    const size_t n_doubles = slab_doubles + B * stage;
    const size_t n_ints = B * (fsm::ROBOT_INTS + 2 * fsm::MAX_TASKS + STAGE_INTS) + fsm::N_COUNTERS;
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipMalloc(&f->d_doubles, n_doubles * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&f->d_ints, n_ints * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&f->d_com, ALORE_ARM_MAX_CLASSES * 2 * sizeof(double));
    if (e == hipSuccess) e = hipMemset(f->d_doubles, 0, n_doubles * sizeof(double));
    if (e == hipSuccess) e = hipMemset(f->d_ints, 0, n_ints * sizeof(int));
    if (e == hipSuccess) e = hipMemset(f->d_com, 0, ALORE_ARM_MAX_CLASSES * 2 * sizeof(double));
    fsm::Slab& s = f->s;
    s.B = (int)B; s.max_tasks = max_tasks; s.max_objects = max_objects; s.max_pts = max_path_points;
    double* d = f->d_doubles;
    s.reach_threshold = d; d += B;
    s.object_vel_cmd = d; d += 3 * B;
    s.start_xytheta = d; d += 3 * B;
    s.goal_xytheta = d; d += 3 * B;
    s.object_pose_used = d; d += 4 * B;
    s.control = d; d += ALORE_FSM_CONTROL_ROW * B;
    s.robot_path = d; d += 2 * mp * B;
    s.object_path = d; d += 2 * mp * B;
    s.target_poses = d; d += 4 * mt * B;
    f->d_stage = d;
    int* w = f->d_ints;
    s.words = w; w += fsm::ROBOT_INTS * B;
    s.object_sequence = w; w += fsm::MAX_TASKS * B;
    s.target_sequence = w; w += fsm::MAX_TASKS * B;
    s.counters = w; w += fsm::N_COUNTERS;
    f->d_stage_int = w;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(fsm::reset_kernel, dim3(grid((int)B)), dim3(fsm::LANES), 0, nullptr, h->P, f->F, (int)B, (const int*)nullptr, h->g, f->s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        if (f->d_doubles) (void)hipFree(f->d_doubles);
        if (f->d_ints) (void)hipFree(f->d_ints);
        if (f->d_com) (void)hipFree(f->d_com);
        delete f;
        return fail(h, e == hipErrorOutOfMemory ? ALORE_ARM_E_NOMEM : ALORE_ARM_E_HIP, "alore_fsm_create: %sHIP error %ld", "", (long)e);
    }
    h->fsm = f;
    h->fsm_free = fsm_free;
    return ALORE_ARM_OK;
}

int alore_fsm_destroy(alore_arm_handle h)
{
    if (h) fsm_free(h);
    return ALORE_ARM_OK;
}

int alore_fsm_set_class_offsets(alore_arm_handle h, int n_classes, const double* com_offset)
{
    if (int rc = check(h, "alore_fsm_set_class_offsets", 0)) return rc;
    if (!com_offset || n_classes < 1 || n_classes > ALORE_ARM_MAX_CLASSES || !z1::finite_n(com_offset, 2 * n_classes))
        return fail(h, ALORE_ARM_E_INVALID, "alore_fsm_set_class_offsets: %s1 .. 64 classes of finite numbers (got %ld)", "", n_classes);
    double table[ALORE_ARM_MAX_CLASSES * 2] = {};
    std::memcpy(table, com_offset, (size_t)n_classes * 2 * sizeof(double));
    FSM_HIP(hipDeviceSynchronize());
    FSM_HIP(hipMemcpy(h->fsm->d_com, table, sizeof(table), hipMemcpyHostToDevice));
    return ALORE_ARM_OK;
}

int alore_fsm_reset(alore_arm_handle h, int count, const int* mask)
{
    if (int rc = check(h, "alore_fsm_reset", count)) return rc;
    if (count == 0) return ALORE_ARM_OK;
    alore_fsm_slab* f = h->fsm;
    FSM_HIP(hipDeviceSynchronize());
    if (mask) FSM_HIP(hipMemcpy(f->d_stage_int, mask, (size_t)count * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(fsm::reset_kernel, dim3(grid(count)), dim3(fsm::LANES), 0, nullptr, h->P, f->F, count, mask ? (const int*)f->d_stage_int : nullptr, h->g,
                       f->s);
    FSM_HIP(hipGetLastError());
    FSM_HIP(hipStreamSynchronize(nullptr));
    return ALORE_ARM_OK;
}

int alore_fsm_set_targets(alore_arm_handle h, int count, const double* target_poses, int row_stride, int device_pointers, void* stream)
{
    if (int rc = check(h, "alore_fsm_set_targets", count)) return rc;
    alore_fsm_slab* f = h->fsm;
    const int row_bytes = f->s.max_tasks * 32;
    if (!target_poses || bad_stride(row_stride, row_bytes, 8))
        return fail(h, ALORE_ARM_E_INVALID, "alore_fsm_set_targets: %sNULL target_poses, or a stride smaller than its row or not a multiple of 8");
    if (count == 0) return ALORE_ARM_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!device_pointers) {
        FSM_HIP(upload(f->d_stage, (size_t)row_bytes, target_poses, (size_t)row_stride, (size_t)row_bytes, count, st));
        target_poses = f->d_stage; row_stride = row_bytes;
    }
    hipLaunchKernelGGL(fsm::set_targets_kernel, dim3(grid(count)), dim3(fsm::LANES), 0, st, count, f->s, target_poses, row_stride);
    FSM_HIP(hipGetLastError());
    if (!device_pointers) FSM_HIP(hipStreamSynchronize(st));
    return ALORE_ARM_OK;
}

int alore_fsm_set_sequences(alore_arm_handle h, int count, const int* order, int order_stride, const int* n_order, const int* mask, int device_pointers,
                            void* stream)
{
    if (int rc = check(h, "alore_fsm_set_sequences", count)) return rc;
    alore_fsm_slab* f = h->fsm;
    if (!order || !n_order || bad_stride(order_stride, 8, 4))
        return fail(h, ALORE_ARM_E_INVALID, "alore_fsm_set_sequences: %sNULL array, or a stride smaller than two ints or not a multiple of 4");
    if (count == 0) return ALORE_ARM_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!device_pointers) {
        const size_t B = (size_t)count;
        size_t width = (size_t)f->s.max_tasks * 8; // the row as far as it can count, and never beyond the caller's stride
        if (width > (size_t)order_stride) width = (size_t)order_stride;
        for (int b = 0; b < count; ++b)
            if (n_order[b] > 0 && (size_t)n_order[b] * 4 > (size_t)order_stride && n_order[b] <= 2 * f->s.max_tasks)
                return fail(h, ALORE_ARM_E_INVALID, "alore_fsm_set_sequences: %sthe row of robot %ld is longer than the stride", "", b);
        FSM_HIP(hipMemsetAsync(f->d_stage_int, 0, B * STAGE_INTS * sizeof(int), st));
        FSM_HIP(upload(f->d_stage_int, 2 * fsm::MAX_TASKS * 4, order, (size_t)order_stride, width, count, st));
        FSM_HIP(hipMemcpyAsync(f->d_stage_int + 2 * fsm::MAX_TASKS * B, n_order, B * sizeof(int), hipMemcpyHostToDevice, st));
        if (mask) FSM_HIP(hipMemcpyAsync(f->d_stage_int + (2 * fsm::MAX_TASKS + 1) * B, mask, B * sizeof(int), hipMemcpyHostToDevice, st));
        order = f->d_stage_int; order_stride = 2 * fsm::MAX_TASKS * 4;
        n_order = f->d_stage_int + 2 * fsm::MAX_TASKS * B;
        if (mask) mask = f->d_stage_int + (2 * fsm::MAX_TASKS + 1) * B;
    }
    hipLaunchKernelGGL(fsm::set_sequences_kernel, dim3(grid(count)), dim3(fsm::LANES), 0, st, count, f->s, order, order_stride, n_order, mask);
    FSM_HIP(hipGetLastError());
    if (!device_pointers) FSM_HIP(hipStreamSynchronize(st));
    return ALORE_ARM_OK;
}

int alore_fsm_set_paths(alore_arm_handle h, int count, const double* xy, int xy_stride, const int* n_points, const int* mask, int device_pointers,
                        void* stream)
{
    if (int rc = check(h, "alore_fsm_set_paths", count)) return rc;
    alore_fsm_slab* f = h->fsm;
    if (!xy || !n_points || bad_stride(xy_stride, 16, 8))
        return fail(h, ALORE_ARM_E_INVALID, "alore_fsm_set_paths: %sNULL array, or a stride smaller than one point or not a multiple of 8");
    if (count == 0) return ALORE_ARM_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!device_pointers) {
        const size_t B = (size_t)count, row_bytes = (size_t)f->s.max_pts * 16;
        const size_t width = row_bytes < (size_t)xy_stride ? row_bytes : (size_t)xy_stride;
        for (int b = 0; b < count; ++b)
            if (n_points[b] > 0 && n_points[b] <= f->s.max_pts && (size_t)n_points[b] * 16 > (size_t)xy_stride)
                return fail(h, ALORE_ARM_E_INVALID, "alore_fsm_set_paths: %sthe row of robot %ld is longer than the stride", "", b);
        FSM_HIP(upload(f->d_stage, row_bytes, xy, (size_t)xy_stride, width, count, st));
        FSM_HIP(hipMemcpyAsync(f->d_stage_int, n_points, B * sizeof(int), hipMemcpyHostToDevice, st));
        if (mask) FSM_HIP(hipMemcpyAsync(f->d_stage_int + B, mask, B * sizeof(int), hipMemcpyHostToDevice, st));
        xy = f->d_stage; xy_stride = (int)row_bytes;
        n_points = f->d_stage_int;
        if (mask) mask = f->d_stage_int + B;
    }
    hipLaunchKernelGGL(fsm::set_paths_kernel, dim3(grid(count)), dim3(fsm::LANES), 0, st, count, f->s, xy, xy_stride, n_points, mask);
    FSM_HIP(hipGetLastError());
    if (!device_pointers) FSM_HIP(hipStreamSynchronize(st));
    return ALORE_ARM_OK;
}

int alore_fsm_tick(alore_arm_handle h, int count, const double* robot_pose, int pose_stride, const double* object_poses, int objects_stride,
                   const double* arm_base_pose, int base_stride, const double* joint_positions, int joint_stride, int device_pointers, void* stream)
{
    if (int rc = check(h, "alore_fsm_tick", count)) return rc;
    alore_fsm_slab* f = h->fsm;
    const int mo = f->s.max_objects;
    if (!robot_pose || !object_poses || !arm_base_pose || !joint_positions || bad_stride(pose_stride, 32, 8) || bad_stride(objects_stride, mo * 32, 8) ||
        bad_stride(base_stride, 56, 8) || bad_stride(joint_stride, 56, 8))
        return fail(h, ALORE_ARM_E_INVALID, "alore_fsm_tick: %sNULL array, or a stride smaller than its row or not a multiple of 8");
    if (count == 0) return ALORE_ARM_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!device_pointers) {
        const size_t B = (size_t)count, o = (size_t)mo * 4;
        double *d_pose = f->d_stage, *d_obj = d_pose + 4 * B, *d_base = d_obj + o * B, *d_jp = d_base + 7 * B;
        FSM_HIP(upload(d_pose, 32, robot_pose, (size_t)pose_stride, 32, count, st));
        FSM_HIP(upload(d_obj, o * 8, object_poses, (size_t)objects_stride, o * 8, count, st));
        FSM_HIP(upload(d_base, 56, arm_base_pose, (size_t)base_stride, 56, count, st));
        FSM_HIP(upload(d_jp, 56, joint_positions, (size_t)joint_stride, 56, count, st));
        robot_pose = d_pose; pose_stride = 32;
        object_poses = d_obj; objects_stride = (int)(o * 8);
        arm_base_pose = d_base; base_stride = 56;
        joint_positions = d_jp; joint_stride = 56;
    }
    hipLaunchKernelGGL(fsm::tick_kernel, dim3(grid(count)), dim3(fsm::LANES), 0, st, h->P, f->F, count, h->d_classes, h->n_classes, h->d_class_of, f->d_com,
                       h->g, f->s, robot_pose, pose_stride, object_poses, objects_stride, arm_base_pose, base_stride, joint_positions, joint_stride);
    FSM_HIP(hipGetLastError());
    if (!device_pointers) FSM_HIP(hipStreamSynchronize(st));
    return ALORE_ARM_OK;
}

int alore_fsm_device_view(alore_arm_handle h, alore_fsm_view* out)
{
    if (int rc = check(h, "alore_fsm_device_view", 0)) return rc;
    if (!out) return fail(h, ALORE_ARM_E_INVALID, "alore_fsm_device_view: NULL out%s");
    const fsm::Slab& s = h->fsm->s;
    int** words = &out->task_state;
    for (int i = 0; i < fsm::ROBOT_INTS; ++i) words[i] = s.words + (size_t)i * s.B; // request_mask is the last word
    out->object_sequence = s.object_sequence;
    out->target_sequence = s.target_sequence;
    out->reach_threshold = s.reach_threshold;
    out->object_vel_cmd = s.object_vel_cmd;
    out->start_xytheta = s.start_xytheta;
    out->goal_xytheta = s.goal_xytheta;
    out->object_pose_used = s.object_pose_used;
    out->control = s.control;
    out->robot_path = s.robot_path;
    out->object_path = s.object_path;
    out->target_poses = s.target_poses;
    out->counters = s.counters;
    out->max_tasks = s.max_tasks; out->max_objects = s.max_objects; out->max_path_points = s.max_pts; out->reserved = 0;
    return ALORE_ARM_OK;
}

int alore_fsm_get(alore_arm_handle h, int count, alore_fsm_view* out)
{
    if (int rc = check(h, "alore_fsm_get", count)) return rc;
    if (!out) return fail(h, ALORE_ARM_E_INVALID, "alore_fsm_get: NULL out%s");
    const fsm::Slab& s = h->fsm->s;
    out->max_tasks = s.max_tasks; out->max_objects = s.max_objects; out->max_path_points = s.max_pts; out->reserved = 0;
    FSM_HIP(hipDeviceSynchronize());
    const size_t n = (size_t)count;
    if (out->counters) FSM_HIP(hipMemcpy(out->counters, s.counters, fsm::N_COUNTERS * sizeof(int), hipMemcpyDeviceToHost));
    if (n == 0) return ALORE_ARM_OK;
    int** words = &out->task_state;
    for (int i = 0; i < fsm::ROBOT_INTS; ++i)
        if (words[i]) FSM_HIP(hipMemcpy(words[i], s.words + (size_t)i * s.B, n * 4, hipMemcpyDeviceToHost));
    const struct { void* dst; const void* src; size_t bytes; } copies[] = {
        {out->object_sequence, s.object_sequence, n * fsm::MAX_TASKS * 4}, {out->target_sequence, s.target_sequence, n * fsm::MAX_TASKS * 4},
        {out->reach_threshold, s.reach_threshold, n * 8}, {out->object_vel_cmd, s.object_vel_cmd, n * 24}, {out->start_xytheta, s.start_xytheta, n * 24},
        {out->goal_xytheta, s.goal_xytheta, n * 24}, {out->object_pose_used, s.object_pose_used, n * 32},
        {out->control, s.control, n * ALORE_FSM_CONTROL_ROW * 8}, {out->robot_path, s.robot_path, n * s.max_pts * 16},
        {out->object_path, s.object_path, n * s.max_pts * 16}, {out->target_poses, s.target_poses, n * s.max_tasks * 32}};
    for (const auto& c : copies)
        if (c.dst) FSM_HIP(hipMemcpy(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost));
    return ALORE_ARM_OK;
}

} // extern "C"

// the view's int pointers are filled by number: they must lie in the order of fsm::Robot, request_mask last
static_assert(offsetof(alore_fsm_view, request_mask) == (fsm::ROBOT_INTS - 1) * sizeof(int*) && offsetof(alore_fsm_view, object_sequence) ==
                  fsm::ROBOT_INTS * sizeof(int*), "alore_fsm_view's words follow fsm::Robot");
