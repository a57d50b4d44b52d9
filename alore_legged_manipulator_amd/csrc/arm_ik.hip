// arm_ik.hip -- the batched Z1 grasp kinematics on the device and the C ABI of include/alore_arm.h.
// One problem (one robot) per lane, in float64; a workgroup is ONE wavefront of 64 lanes.  A lane runs z1::ik_solve of
// z1_kinematics.h as it stands: its loop ends when its own problem has finished (below eps, at the limit, at a bad pivot), from then
// on the lane is masked off and its q, err_norm and iteration count are frozen; the wavefront goes on under the EXEC mask of the
// lanes that are left and leaves the loop with its slowest problem.  With one wavefront per workgroup nothing else waits for it:
// the slot is free for the next workgroup as soon as that wavefront is done.  Chain, Jacobian, Je and the factor are per-lane
// arrays with compile-time indices after unrolling, i.e. registers; see DESIGN.md for what the compiler reports.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>

#include "arm_handle.h"

static_assert(sizeof(alore_arm_params) == sizeof(z1::Params), "alore_arm_params mirrors z1::Params");
static_assert(sizeof(alore_arm_class) == sizeof(z1::Class), "alore_arm_class mirrors z1::Class");

namespace arm {

template <typename T> __device__ inline const T* row(const T* base, int b, int stride_bytes)
{
    return reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + (size_t)b * (size_t)stride_bytes);
}
template <typename T> __device__ inline T* row(T* base, int b, int stride_bytes)
{
    return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + (size_t)b * (size_t)stride_bytes);
}

__global__ __launch_bounds__(LANES) void ik_kernel(z1::Params P, int count, const double* q_init, int q_stride, const double* target, int target_stride,
                                                   double* q_out, double* err_norm, int* iterations, int* status)
{
    const int b = blockIdx.x * LANES + threadIdx.x;
    if (b >= count) return;
    double qi[7], T[12], q[7];
    const double* qr = row(q_init, b, q_stride);
    const double* tr = row(target, b, target_stride);
    for (int i = 0; i < 7; ++i) qi[i] = qr[i];
    for (int i = 0; i < 12; ++i) T[i] = tr[i];
    const z1::IkResult r = z1::ik_solve(P, qi, T, q);
    for (int i = 0; i < 7; ++i) q_out[(size_t)b * 7 + i] = q[i];
    err_norm[b] = r.err_norm;
    iterations[b] = r.iterations;
    status[b] = r.status;
}

__global__ __launch_bounds__(LANES) void grasp_step_kernel(z1::Params P, int count, const z1::Class* classes, int n_classes, const int* class_of,
                                                           GraspSlab s, const double* robot_xy, int xy_stride, const double* object_pose,
                                                           int object_stride, const double* arm_base_pose, int base_stride,
                                                           const double* joint_positions, int joint_stride)
{
    const int b = blockIdx.x * LANES + threadIdx.x;
    if (b >= count) return;
    int ci = class_of[b];
    ci = ci < 0 ? 0 : (ci > n_classes - 1 ? n_classes - 1 : ci);
    const z1::Class c = classes[ci];
    z1::Grasp g;
    g.k = s.k[b]; g.d_gripper = s.d_gripper[b]; g.gripper_ang = s.gripper_ang[b]; g.err_norm = s.err_norm[b];
    g.grasp_time = s.grasp_time[b]; g.flag = s.flag[b]; g.stable = s.stable[b];
    for (int i = 0; i < 7; ++i) g.joint_cmd[i] = s.joint_cmd[(size_t)b * 7 + i];
    for (int i = 0; i < 3; ++i) g.robot_vel_cmd[i] = s.robot_vel_cmd[(size_t)b * 3 + i];
    double xy[2], obj[4], base[7], jp[7];
    const double *xr = row(robot_xy, b, xy_stride), *orow = row(object_pose, b, object_stride), *br = row(arm_base_pose, b, base_stride),
                 *jr = row(joint_positions, b, joint_stride);
    xy[0] = xr[0]; xy[1] = xr[1];
    for (int i = 0; i < 4; ++i) obj[i] = orow[i];
    for (int i = 0; i < 7; ++i) base[i] = br[i];
    for (int i = 0; i < 7; ++i) jp[i] = jr[i];
    z1::grasp_step(P, c, g, xy, obj, base, jp);
    s.k[b] = g.k; s.d_gripper[b] = g.d_gripper; s.gripper_ang[b] = g.gripper_ang; s.err_norm[b] = g.err_norm;
    s.grasp_time[b] = g.grasp_time; s.flag[b] = g.flag; s.stable[b] = g.stable; s.done[b] = g.done;
    s.ik_iterations[b] = g.ik_iterations; s.ik_status[b] = g.ik_status;
    for (int i = 0; i < 7; ++i) s.joint_cmd[(size_t)b * 7 + i] = g.joint_cmd[i];
    for (int i = 0; i < 3; ++i) s.robot_vel_cmd[(size_t)b * 3 + i] = g.robot_vel_cmd[i];
}

__global__ __launch_bounds__(LANES) void grasp_reset_kernel(z1::Params P, int count, const int* mask, GraspSlab s)
{
    const int b = blockIdx.x * LANES + threadIdx.x;
    if (b >= count || (mask && mask[b] == 0)) return;
    z1::Grasp g;
    z1::grasp_initial(P, g);
    s.k[b] = g.k; s.d_gripper[b] = g.d_gripper; s.gripper_ang[b] = g.gripper_ang; s.err_norm[b] = g.err_norm;
    s.grasp_time[b] = g.grasp_time; s.flag[b] = g.flag; s.stable[b] = g.stable; s.done[b] = g.done;
    s.ik_iterations[b] = g.ik_iterations; s.ik_status[b] = g.ik_status;
    for (int i = 0; i < 7; ++i) s.joint_cmd[(size_t)b * 7 + i] = g.joint_cmd[i];
    for (int i = 0; i < 3; ++i) s.robot_vel_cmd[(size_t)b * 3 + i] = g.robot_vel_cmd[i];
}

__global__ __launch_bounds__(LANES) void grasp_pose_kernel(int count, const z1::Class* classes, int n_classes, const int* class_of, int which,
                                                           const double* object_pose, int object_stride, double* out_pose, int pose_stride,
                                                           double* out_goal, int goal_stride)
{
    const int b = blockIdx.x * LANES + threadIdx.x;
    if (b >= count) return;
    int ci = class_of[b];
    ci = ci < 0 ? 0 : (ci > n_classes - 1 ? n_classes - 1 : ci);
    const double* cfg = which == ALORE_ARM_POSE_PLAN ? classes[ci].plan_cfg : classes[ci].grasp_cfg;
    const double c3[3] = {cfg[0], cfg[1], cfg[2]};
    double obj[4], pose[7];
    const double* orow = row(object_pose, b, object_stride);
    for (int i = 0; i < 4; ++i) obj[i] = orow[i];
    z1::grasp_pose(obj, c3, pose);
    if (out_pose) {
        double* o = row(out_pose, b, pose_stride);
        for (int i = 0; i < 7; ++i) o[i] = pose[i];
    }
    if (out_goal) {
        double* o = row(out_goal, b, goal_stride);
        o[0] = pose[0]; o[1] = pose[1]; o[2] = obj[3];
    }
}

__global__ __launch_bounds__(LANES) void fk_kernel(z1::Params P, int count, const double* q, int q_stride, double* pose, int pose_stride, double* jac,
                                                   int jac_stride)
{
    const int b = blockIdx.x * LANES + threadIdx.x;
    if (b >= count) return;
    double qq[7];
    const double* qr = row(q, b, q_stride);
    for (int i = 0; i < 7; ++i) qq[i] = qr[i];
    z1::Chain c;
    z1::chain(P, qq, c);
    if (pose) {
        double* o = row(pose, b, pose_stride);
        for (int i = 0; i < 9; ++i) o[i] = c.R[i];
        for (int i = 0; i < 3; ++i) o[9 + i] = c.p[i];
    }
    if (jac) {
        double J[36];
        z1::jac_of_chain(c, J);
        double* o = row(jac, b, jac_stride);
        for (int i = 0; i < 36; ++i) o[i] = J[i];
    }
}

} // namespace arm

// ---- the C ABI (struct alore_arm: arm_handle.h) ----------------------------------------------------------------------------------------
namespace {
constexpr int STAGE_ROW = 56; // the widest call: fk, 7 in + 12 + 36 out
char g_err[256] = "";

int fail(alore_arm* h, int code, const char* fmt, const char* a = "", long v = 0)
{
    std::snprintf(h ? h->err : g_err, 256, fmt, a, v);
    return code;
}
int hip_fail(alore_arm* h, hipError_t e, const char* what) { return fail(h, ALORE_ARM_E_HIP, "%s: HIP error %ld", what, (long)e); }
#define ARM_HIP(call)                                       \
    do {                                                    \
        hipError_t e_ = (call);                             \
        if (e_ != hipSuccess) return hip_fail(h, e_, #call); \
    } while (0)

bool pos_finite(double v) { return v > 0.0 && z1::finite(v); }
bool bad_stride(int stride, int row_doubles) { return stride < row_doubles * 8 || stride % 8 != 0; }
int grid(int count) { return (count + arm::LANES - 1) / arm::LANES; }

int check_params(alore_arm* h, const z1::Params& P)
{
    if (P.max_iter < 1) return fail(h, ALORE_ARM_E_INVALID, "max_iter %s must be at least 1 (got %ld)", "", P.max_iter);
    if (!pos_finite(P.eps) || !pos_finite(P.damp) || !pos_finite(P.dt)) return fail(h, ALORE_ARM_E_INVALID, "eps, damp and dt must be finite and positive%s", "");
    if (!z1::finite_n(P.joint1_xyz, 3) || !z1::finite_n(P.tool_xyz, 3) || !z1::finite_n(P.joint_default, 7))
        return fail(h, ALORE_ARM_E_INVALID, "joint1_xyz, tool_xyz and joint_default must be finite%s", "");
    return ALORE_ARM_OK;
}
int check_count(alore_arm* h, const char* call, int count)
{
    if (!h) return fail(nullptr, ALORE_ARM_E_INVALID, "%s: NULL handle", call);
    if (count < 0 || count > h->max_problems) return fail(h, ALORE_ARM_E_INVALID, "%s: count %ld is outside 0 .. max_problems", call, count);
    return ALORE_ARM_OK;
}
// rows of `n` doubles from HOST memory with a byte stride into the packed staging area at `at` (in doubles per row: n)
hipError_t upload(double* dst, const double* src, int stride, int n, int count, hipStream_t st)
{
    return hipMemcpy2DAsync(dst, (size_t)n * 8, src, (size_t)stride, (size_t)n * 8, (size_t)count, hipMemcpyHostToDevice, st);
}
hipError_t download(double* dst, int stride, const double* src, int n, int count, hipStream_t st)
{
    return hipMemcpy2DAsync(dst, (size_t)stride, src, (size_t)n * 8, (size_t)n * 8, (size_t)count, hipMemcpyDeviceToHost, st);
}
void default_classes(z1::Class* c)
{
    // config.yaml `objects`: chair, table, box
    const z1::Class presets[3] = {{ALORE_ARM_CATEGORY_OTHER, 0, {0.45, 0.96, 60.0}, {0.8, 0.0, 0.0}, {0.0, 1.9, -1.72, 0.72, 0.0, 0.0, -0.1}},
                                  {ALORE_ARM_CATEGORY_TABLE, 0, {0.5, 0.62, 6.0}, {1.07, 0.0, 0.0}, {0.0, 2.8, -1.15, -1.4, 0.0, 0.0, -0.1}},
                                  {ALORE_ARM_CATEGORY_BOX, 0, {0.25, 0.45, 80.0}, {0.83, 0.0, 0.0}, {0.0, 2.71, -0.82, -0.5, 0.0, 0.0, -0.1}}};
    for (int i = 0; i < 3; ++i) c[i] = presets[i];
}
} // namespace

extern "C" {

void alore_arm_default_params(alore_arm_params* p)
{
    if (p) z1::default_params(reinterpret_cast<z1::Params*>(p));
}

int alore_arm_create(const alore_arm_params* params, int device, int max_problems, alore_arm_handle* out)
{
    alore_arm* h = nullptr;
    if (!out) return fail(h, ALORE_ARM_E_INVALID, "alore_arm_create: NULL out%s", "");
    *out = nullptr;
    z1::Params P;
    z1::default_params(&P);
    if (params) std::memcpy(&P, params, sizeof(P));
    if (max_problems < 1) return fail(h, ALORE_ARM_E_INVALID, "alore_arm_create: max_problems %s must be at least 1 (got %ld)", "", max_problems);
    if (int rc = check_params(h, P)) return rc;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
        return fail(h, ALORE_ARM_E_NO_DEVICE, "alore_arm_create: no GPU %s(device %ld); there is no CPU path", "", device);
    h = new (std::nothrow) alore_arm();
    if (!h) return fail(nullptr, ALORE_ARM_E_NOMEM, "alore_arm_create: out of host memory%s", "");
    h->device = device;
    h->max_problems = max_problems;
    h->P = P;
    h->err[0] = 0;
    const size_t B = (size_t)max_problems;
    double* dbl = nullptr;
    int* ints = nullptr;
    // one block of doubles and one of ints: q 7, err 1, grasp 7 + 3 + 4, staging
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&dbl, B * (7 + 1 + 14 + STAGE_ROW) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&ints, B * (2 + 6 + 1 + 1) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&h->d_classes, ALORE_ARM_MAX_CLASSES * sizeof(z1::Class));
    if (e == hipSuccess) e = hipMemset(ints, 0, B * 10 * sizeof(int));
    if (e != hipSuccess) {
        if (dbl) (void)hipFree(dbl);
        if (ints) (void)hipFree(ints);
        if (h->d_classes) (void)hipFree(h->d_classes);
        delete h;
        return fail(nullptr, e == hipErrorOutOfMemory ? ALORE_ARM_E_NOMEM : ALORE_ARM_E_HIP, "alore_arm_create: %sHIP error %ld", "", (long)e);
    }
    h->d_q = dbl;
    h->d_err = dbl + 7 * B;
    h->g.joint_cmd = dbl + 8 * B;
    h->g.robot_vel_cmd = dbl + 15 * B;
    h->g.k = dbl + 18 * B;
    h->g.d_gripper = dbl + 19 * B;
    h->g.gripper_ang = dbl + 20 * B;
    h->g.err_norm = dbl + 21 * B;
    h->d_stage = dbl + 22 * B;
    h->d_iterations = ints;
    h->d_status = ints + B;
    h->g.done = ints + 2 * B;
    h->g.grasp_time = ints + 3 * B;
    h->g.flag = ints + 4 * B;
    h->g.stable = ints + 5 * B;
    h->g.ik_iterations = ints + 6 * B;
    h->g.ik_status = ints + 7 * B;
    h->d_class_of = ints + 8 * B; // 0: the first class
    h->d_stage_int = ints + 9 * B;
    z1::Class table[3];
    default_classes(table);
    h->n_classes = 3;
    e = hipMemcpy(h->d_classes, table, sizeof(table), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dbl, 0, B * 22 * sizeof(double));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(arm::grasp_reset_kernel, dim3(grid(max_problems)), dim3(arm::LANES), 0, nullptr, h->P, max_problems, (const int*)nullptr, h->g);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        alore_arm_destroy(h);
        return fail(nullptr, ALORE_ARM_E_HIP, "alore_arm_create: %sHIP error %ld", "", (long)e);
    }
    *out = h;
    return ALORE_ARM_OK;
}

int alore_arm_destroy(alore_arm_handle h)
{
    if (!h) return ALORE_ARM_OK;
    if (h->fsm_free) h->fsm_free(h); // the task FSM of alore_fsm_create, if it is still attached
    (void)hipFree(h->d_q);          // the block of doubles
    (void)hipFree(h->d_iterations); // the block of ints
    (void)hipFree(h->d_classes);
    delete h;
    return ALORE_ARM_OK;
}

const char* alore_arm_last_error(alore_arm_handle h) { return h ? h->err : g_err; }

int alore_arm_fk(alore_arm_handle h, int count, const double* q, int q_stride, double* pose, int pose_stride, double* jac, int jac_stride,
                 int device_pointers, void* stream)
{
    if (int rc = check_count(h, "alore_arm_fk", count)) return rc;
    if (!q || bad_stride(q_stride, 7) || (pose && bad_stride(pose_stride, 12)) || (jac && bad_stride(jac_stride, 36)))
        return fail(h, ALORE_ARM_E_INVALID, "alore_arm_fk: %sNULL q, or a stride smaller than its row or not a multiple of 8", "");
    if (count == 0) return ALORE_ARM_OK;
    hipStream_t st = (hipStream_t)stream;
    const double* dq = q;
    double *dpose = pose, *djac = jac;
    int sq = q_stride, sp = pose_stride, sj = jac_stride;
    if (!device_pointers) {
        const size_t B = (size_t)count;
        ARM_HIP(upload(h->d_stage, q, q_stride, 7, count, st));
        dq = h->d_stage; sq = 56;
        if (pose) { dpose = h->d_stage + 7 * B; sp = 96; }
        if (jac) { djac = h->d_stage + 19 * B; sj = 288; }
    }
    hipLaunchKernelGGL(arm::fk_kernel, dim3(grid(count)), dim3(arm::LANES), 0, st, h->P, count, dq, sq, dpose, sp, djac, sj);
    ARM_HIP(hipGetLastError());
    if (!device_pointers) {
        if (pose) ARM_HIP(download(pose, pose_stride, dpose, 12, count, st));
        if (jac) ARM_HIP(download(jac, jac_stride, djac, 36, count, st));
        ARM_HIP(hipStreamSynchronize(st));
    }
    return ALORE_ARM_OK;
}

int alore_arm_ik(alore_arm_handle h, int count, const double* q_init, int q_stride, const double* target, int target_stride, int device_pointers,
                 void* stream)
{
    if (int rc = check_count(h, "alore_arm_ik", count)) return rc;
    if (!q_init || !target || bad_stride(q_stride, 7) || bad_stride(target_stride, 12))
        return fail(h, ALORE_ARM_E_INVALID, "alore_arm_ik: %sNULL array, or a stride smaller than its row or not a multiple of 8", "");
    if (count == 0) return ALORE_ARM_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!device_pointers) {
        ARM_HIP(upload(h->d_stage, q_init, q_stride, 7, count, st));
        ARM_HIP(upload(h->d_stage + 7 * (size_t)count, target, target_stride, 12, count, st));
        q_init = h->d_stage; q_stride = 56;
        target = h->d_stage + 7 * (size_t)count; target_stride = 96;
    }
    hipLaunchKernelGGL(arm::ik_kernel, dim3(grid(count)), dim3(arm::LANES), 0, st, h->P, count, q_init, q_stride, target, target_stride, h->d_q, h->d_err,
                       h->d_iterations, h->d_status);
    ARM_HIP(hipGetLastError());
    if (!device_pointers) ARM_HIP(hipStreamSynchronize(st));
    return ALORE_ARM_OK;
}

int alore_arm_device_ik(alore_arm_handle h, alore_arm_ik_view* out)
{
    if (!h || !out) return fail(h, ALORE_ARM_E_INVALID, "alore_arm_device_ik: NULL argument%s", "");
    out->q = h->d_q;
    out->err_norm = h->d_err;
    out->iterations = h->d_iterations;
    out->status = h->d_status;
    return ALORE_ARM_OK;
}

int alore_arm_get_ik(alore_arm_handle h, int count, double* q, double* err_norm, int* iterations, int* status)
{
    if (int rc = check_count(h, "alore_arm_get_ik", count)) return rc;
    ARM_HIP(hipDeviceSynchronize());
    const size_t n = (size_t)count;
    if (n == 0) return ALORE_ARM_OK;
    if (q) ARM_HIP(hipMemcpy(q, h->d_q, n * 7 * sizeof(double), hipMemcpyDeviceToHost));
    if (err_norm) ARM_HIP(hipMemcpy(err_norm, h->d_err, n * sizeof(double), hipMemcpyDeviceToHost));
    if (iterations) ARM_HIP(hipMemcpy(iterations, h->d_iterations, n * sizeof(int), hipMemcpyDeviceToHost));
    if (status) ARM_HIP(hipMemcpy(status, h->d_status, n * sizeof(int), hipMemcpyDeviceToHost));
    return ALORE_ARM_OK;
}

int alore_arm_set_classes(alore_arm_handle h, int n_classes, const alore_arm_class* classes)
{
    if (!h) return fail(nullptr, ALORE_ARM_E_INVALID, "alore_arm_set_classes: NULL handle%s", "");
    if (!classes || n_classes < 1 || n_classes > ALORE_ARM_MAX_CLASSES)
        return fail(h, ALORE_ARM_E_INVALID, "alore_arm_set_classes: %s1 .. 64 classes (got %ld)", "", n_classes);
    for (int i = 0; i < n_classes; ++i) {
        const alore_arm_class& c = classes[i];
        if (c.category < ALORE_ARM_CATEGORY_OTHER || c.category > ALORE_ARM_CATEGORY_BOX)
            return fail(h, ALORE_ARM_E_INVALID, "alore_arm_set_classes: %sclass %ld has an unknown category", "", i);
        if (!z1::finite_n(c.grasp_cfg, 3) || !z1::finite_n(c.plan_cfg, 3) || !z1::finite_n(c.arm_default_pose, 7))
            return fail(h, ALORE_ARM_E_INVALID, "alore_arm_set_classes: %sclass %ld has a number that is not finite", "", i);
    }
    ARM_HIP(hipDeviceSynchronize());
    ARM_HIP(hipMemcpy(h->d_classes, classes, (size_t)n_classes * sizeof(z1::Class), hipMemcpyHostToDevice));
    h->n_classes = n_classes;
    return ALORE_ARM_OK;
}

int alore_arm_set_robot_classes(alore_arm_handle h, int count, const int* class_of, int device_pointer, void* stream)
{
    if (int rc = check_count(h, "alore_arm_set_robot_classes", count)) return rc;
    if (!class_of) return fail(h, ALORE_ARM_E_INVALID, "alore_arm_set_robot_classes: NULL class_of%s", "");
    if (count == 0) return ALORE_ARM_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!device_pointer) {
        for (int b = 0; b < count; ++b)
            if (class_of[b] < 0 || class_of[b] >= h->n_classes)
                return fail(h, ALORE_ARM_E_INVALID, "alore_arm_set_robot_classes: %sthe class index of slot %ld is outside the table", "", b);
        ARM_HIP(hipMemcpyAsync(h->d_class_of, class_of, (size_t)count * sizeof(int), hipMemcpyHostToDevice, st));
        ARM_HIP(hipStreamSynchronize(st));
    } else
        ARM_HIP(hipMemcpyAsync(h->d_class_of, class_of, (size_t)count * sizeof(int), hipMemcpyDeviceToDevice, st));
    return ALORE_ARM_OK;
}

int alore_arm_grasp_poses(alore_arm_handle h, int count, const double* object_pose, int object_stride, int which, double* out_pose, int pose_stride,
                          double* out_goal, int goal_stride, int device_pointers, void* stream)
{
    if (int rc = check_count(h, "alore_arm_grasp_poses", count)) return rc;
    if (which != ALORE_ARM_POSE_GRASP && which != ALORE_ARM_POSE_PLAN) return fail(h, ALORE_ARM_E_INVALID, "alore_arm_grasp_poses: %sunknown `which` %ld", "", which);
    if (!object_pose || bad_stride(object_stride, 4) || (out_pose && bad_stride(pose_stride, 7)) || (out_goal && bad_stride(goal_stride, 3)))
        return fail(h, ALORE_ARM_E_INVALID, "alore_arm_grasp_poses: %sNULL object_pose, or a stride smaller than its row or not a multiple of 8", "");
    if (count == 0) return ALORE_ARM_OK;
    hipStream_t st = (hipStream_t)stream;
    const double* dobj = object_pose;
    double *dpose = out_pose, *dgoal = out_goal;
    int so = object_stride, sp = pose_stride, sg = goal_stride;
    if (!device_pointers) {
        const size_t B = (size_t)count;
        ARM_HIP(upload(h->d_stage, object_pose, object_stride, 4, count, st));
        dobj = h->d_stage; so = 32;
        if (out_pose) { dpose = h->d_stage + 4 * B; sp = 56; }
        if (out_goal) { dgoal = h->d_stage + 11 * B; sg = 24; }
    }
    hipLaunchKernelGGL(arm::grasp_pose_kernel, dim3(grid(count)), dim3(arm::LANES), 0, st, count, h->d_classes, h->n_classes, h->d_class_of, which, dobj, so,
                       dpose, sp, dgoal, sg);
    ARM_HIP(hipGetLastError());
    if (!device_pointers) {
        if (out_pose) ARM_HIP(download(out_pose, pose_stride, dpose, 7, count, st));
        if (out_goal) ARM_HIP(download(out_goal, goal_stride, dgoal, 3, count, st));
        ARM_HIP(hipStreamSynchronize(st));
    }
    return ALORE_ARM_OK;
}

int alore_arm_grasp_reset(alore_arm_handle h, int count, const int* mask)
{
    if (int rc = check_count(h, "alore_arm_grasp_reset", count)) return rc;
    if (count == 0) return ALORE_ARM_OK;
    ARM_HIP(hipDeviceSynchronize());
    if (mask) ARM_HIP(hipMemcpy(h->d_stage_int, mask, (size_t)count * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(arm::grasp_reset_kernel, dim3(grid(count)), dim3(arm::LANES), 0, nullptr, h->P, count, mask ? (const int*)h->d_stage_int : nullptr, h->g);
    ARM_HIP(hipGetLastError());
    ARM_HIP(hipStreamSynchronize(nullptr));
    return ALORE_ARM_OK;
}

int alore_arm_grasp_step(alore_arm_handle h, int count, const double* robot_xy, int xy_stride, const double* object_pose, int object_stride,
                         const double* arm_base_pose, int base_stride, const double* joint_positions, int joint_stride, int device_pointers, void* stream)
{
    if (int rc = check_count(h, "alore_arm_grasp_step", count)) return rc;
    if (!robot_xy || !object_pose || !arm_base_pose || !joint_positions || bad_stride(xy_stride, 2) || bad_stride(object_stride, 4) ||
        bad_stride(base_stride, 7) || bad_stride(joint_stride, 7))
        return fail(h, ALORE_ARM_E_INVALID, "alore_arm_grasp_step: %sNULL array, or a stride smaller than its row or not a multiple of 8", "");
    if (count == 0) return ALORE_ARM_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!device_pointers) {
        const size_t B = (size_t)count;
        ARM_HIP(upload(h->d_stage, robot_xy, xy_stride, 2, count, st));
        ARM_HIP(upload(h->d_stage + 2 * B, object_pose, object_stride, 4, count, st));
        ARM_HIP(upload(h->d_stage + 6 * B, arm_base_pose, base_stride, 7, count, st));
        ARM_HIP(upload(h->d_stage + 13 * B, joint_positions, joint_stride, 7, count, st));
        robot_xy = h->d_stage; xy_stride = 16;
        object_pose = h->d_stage + 2 * B; object_stride = 32;
        arm_base_pose = h->d_stage + 6 * B; base_stride = 56;
        joint_positions = h->d_stage + 13 * B; joint_stride = 56;
    }
    hipLaunchKernelGGL(arm::grasp_step_kernel, dim3(grid(count)), dim3(arm::LANES), 0, st, h->P, count, h->d_classes, h->n_classes, h->d_class_of, h->g,
                       robot_xy, xy_stride, object_pose, object_stride, arm_base_pose, base_stride, joint_positions, joint_stride);
    ARM_HIP(hipGetLastError());
    if (!device_pointers) ARM_HIP(hipStreamSynchronize(st));
    return ALORE_ARM_OK;
}

int alore_arm_device_grasp(alore_arm_handle h, alore_arm_grasp_view* out)
{
    if (!h || !out) return fail(h, ALORE_ARM_E_INVALID, "alore_arm_device_grasp: NULL argument%s", "");
    out->joint_cmd = h->g.joint_cmd;
    out->robot_vel_cmd = h->g.robot_vel_cmd;
    out->done = h->g.done;
    out->k = h->g.k;
    out->d_gripper = h->g.d_gripper;
    out->gripper_ang = h->g.gripper_ang;
    out->err_norm = h->g.err_norm;
    out->grasp_time = h->g.grasp_time;
    out->flag = h->g.flag;
    out->stable = h->g.stable;
    out->ik_iterations = h->g.ik_iterations;
    out->ik_status = h->g.ik_status;
    return ALORE_ARM_OK;
}

int alore_arm_get_grasp(alore_arm_handle h, int count, const alore_arm_grasp_host* out)
{
    if (int rc = check_count(h, "alore_arm_get_grasp", count)) return rc;
    if (!out) return fail(h, ALORE_ARM_E_INVALID, "alore_arm_get_grasp: NULL out%s", "");
    ARM_HIP(hipDeviceSynchronize());
    const size_t n = (size_t)count;
    if (n == 0) return ALORE_ARM_OK;
    const struct { void* dst; const void* src; size_t bytes; } copies[] = {
        {out->joint_cmd, h->g.joint_cmd, n * 56}, {out->robot_vel_cmd, h->g.robot_vel_cmd, n * 24}, {out->done, h->g.done, n * 4},
        {out->k, h->g.k, n * 8}, {out->d_gripper, h->g.d_gripper, n * 8}, {out->gripper_ang, h->g.gripper_ang, n * 8},
        {out->err_norm, h->g.err_norm, n * 8}, {out->grasp_time, h->g.grasp_time, n * 4}, {out->flag, h->g.flag, n * 4},
        {out->stable, h->g.stable, n * 4}, {out->ik_iterations, h->g.ik_iterations, n * 4}, {out->ik_status, h->g.ik_status, n * 4}};
    for (const auto& c : copies)
        if (c.dst) ARM_HIP(hipMemcpy(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost));
    return ALORE_ARM_OK;
}

} // extern "C"
