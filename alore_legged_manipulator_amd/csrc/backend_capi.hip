// backend_capi.hip -- implementation of include/alore_backend.h: argument checks, device storage, staging
// through pinned host memory, launches.  No CPU path: alore_backend_create fails without a GPU.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "backend_classes.h"
#include "backend_kernels.h"
#include "esdf_window.h"
#include "flat_traj_build.h"
#include "fleet_manager.h"
#include "laser_scan_launch.h"
#include "mission_map.h"
#include "path_search.h"
#include "path_search_wide.h"
#include "task_plan.h"

struct alore_backend_planner {
    alore_backend_config cfg;
    int device = 0, P = 0, B = 0, count = 0;
    std::string err;
    // map
    double* d_map = nullptr;
    backend::MapView map{};
    // problems
    int *d_M = nullptr, *d_cut = nullptr;
    double *d_inner = nullptr, *d_initT = nullptr, *d_pos = nullptr, *d_head = nullptr, *d_tail = nullptr, *d_sxy = nullptr,
           *d_fxy = nullptr, *d_sxyt = nullptr;
    // results
    double *r_inner = nullptr, *r_T = nullptr, *r_coef = nullptr, *r_tail = nullptr;
    int* r_ok = nullptr;
    backend::Status* r_status = nullptr;
    // workspace
    double *d_hist = nullptr, *d_gram = nullptr, *d_pcr = nullptr, *d_x = nullptr, *d_g = nullptr, *d_lam = nullptr, *d_rho = nullptr, *d_cost = nullptr, *d_err = nullptr;
    int* d_ret = nullptr;
    long long* d_stamps = nullptr; // ALORE_BE_STAMPS=1: diagnostic phase cycles of workgroup 0
    backend::Params* d_params = nullptr; // the kernel reads its parameter block from here
    int* d_order = nullptr;              // problems by piece count, longest first (launch order of alore_backend_plan)
    // pinned staging (one slab, carved per call)
    char* h_stage = nullptr;
    size_t stage_bytes = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    // alore_backend_check_plans: the argument block followed by the windows [t_from[count], t_to[count]], pinned and on the
    // device (one upload per call), and the records of the last check
    char *h_check = nullptr, *d_check_in = nullptr;
    alore_backend_check* d_check = nullptr;
    hipEvent_t ev_check = nullptr, ev_check_done = nullptr; // the upload of the previous call has left h_check; its kernel has ended
    bool check_pending = false;
    // alore_backend_set_paths: the argument block followed by the staged inputs of the host route, pinned and on the device, and
    // the build status per slot
    char *h_build = nullptr, *d_build_in = nullptr;
    int* d_build_status = nullptr;
    hipEvent_t ev_build = nullptr; // the upload of the previous call has left h_build
    bool build_pending = false;
    // alore_backend_plan_masked: its parameter block goes up from pinned memory
    backend::Params* h_params = nullptr;
    hipEvent_t ev_params = nullptr;
    bool params_pending = false;
    // the resident occupancy map (alore_backend_map_create): state grid, log-odds and counts; its distance field is d_map.  The
    // argument blocks of up to MAP_SCANS scans go up from pinned memory in one copy
    bool resident = false;
    backend::OccMap omap{};
    backend::EsdfWorkspace esdf_ws{};
    char *h_scan = nullptr, *d_scan = nullptr;
    size_t scan_block = 0;
    hipEvent_t ev_scan = nullptr, ev_scan_done = nullptr; // the upload of the previous blocks has left h_scan; their kernels have ended
    bool scan_pending = false;
    char* d_points = nullptr; // staging of host points (grows)
    size_t points_bytes = 0;
    // alore_backend_search_paths: the argument block followed by the staged inputs of the host route, pinned and on the device,
    // and the slab of searched paths
    char *h_search = nullptr, *d_search_in = nullptr;
    int *d_path_n = nullptr, *d_path_cost = nullptr, *d_search_status = nullptr, *d_search_sweeps = nullptr;
    double* d_path_xy = nullptr;
    hipEvent_t ev_search = nullptr; // the upload of the previous call has left h_search
    bool search_pending = false;
    // alore_backend_search_reserve: wide_slots slabs of wide_cells words for windows of more than psearch::MAX_CELLS cells
    unsigned* d_wide = nullptr;
    long long* d_wide_ticks = nullptr; // [B][2] diagnostic of the wide kernel
    int wide_cells = 0, wide_slots = 0;
    hipEvent_t ev_wide = nullptr; // the last search that read the slabs has ended
    bool wide_pending = false;
    // alore_backend_task_plan: the argument block followed by the staged inputs of the host route, pinned and on the device, and
    // the slab of the missions
    char *h_task = nullptr, *d_task_in = nullptr;
    int *t_status = nullptr, *t_matrix = nullptr, *t_order = nullptr, *t_n_order = nullptr, *t_total = nullptr, *t_fields = nullptr,
        *t_sweeps = nullptr, *t_src_fields = nullptr, *t_src_sweeps = nullptr, *t_assignment = nullptr, *t_assign_total = nullptr;
    double *t_leg_start = nullptr, *t_leg_goal = nullptr;
    hipEvent_t ev_task = nullptr; // the upload of the previous call has left h_task
    bool task_pending = false;
    int task_last_count = 0, task_last_mode = 0; // of the launch whose argument block lies in d_task_in
    // alore_backend_task_reserve: task_slots slabs of task_cells words for missions on windows of more than psearch::MAX_CELLS
    // cells (its own: the search's reservation stays the search's), and the per-source range flags of such missions [B][20]
    unsigned* d_task_wide = nullptr;
    int* t_src_range = nullptr;
    long long* d_task_ticks = nullptr; // [B][20] diagnostic of the wide kernel, with a reservation
    int task_cells = 0, task_slots = 0;
    hipEvent_t ev_task_wide = nullptr; // the last task launch that read the slabs has ended
    bool task_wide_pending = false;
    // alore_backend_laser_*: the sensor (alore_backend_laser_create), its world cloud and the slabs of the scans; the argument
    // block is followed by the staged poses of the host route, pinned and on the device
    bool has_laser = false, has_cloud = false;
    laser::Derived laser_d{};
    int laser_scans = 0, laser_slots = 0, laser_bins = 0, n_cloud = 0;
    size_t cloud_cap = 0; // points
    float *d_cloud = nullptr, *l_laser = nullptr, *l_world = nullptr, *l_compact = nullptr;
    double *l_tables = nullptr, *l_image = nullptr;
    int *l_index = nullptr, *l_n = nullptr, *l_status = nullptr;
    char *h_laser = nullptr, *d_laser_in = nullptr;
    hipEvent_t ev_laser = nullptr; // the upload of the previous call has left h_laser
    bool laser_pending = false;
    // alore_backend_map_paint: the descriptors of one launch, the counters, the staging of a host list (grows); allocated by the
    // first paint call or by alore_backend_mission_create, whichever comes first
    mission::Desc* p_desc = nullptr;
    int p_desc_cap = 0; // descriptors: at least mission::PAINT_CHUNK, the longest host list, the missions' edit list
    int* p_counters = nullptr;
    mission::Edit* p_host_edits = nullptr;
    size_t p_host_cap = 0; // edits
    // alore_backend_mission_*: the slab of the missions (one allocation, m_slab_mem), their edit list with its length on the
    // device, and the staging of the host routes
    bool has_mission = false;
    mission::Params m_params{};
    mission::Slab m_slab{};
    char *m_slab_mem = nullptr, *m_stage = nullptr;
    int *m_was_set = nullptr, *m_n_edits = nullptr;
    mission::Edit* m_edits = nullptr;
    // alore_backend_manager_*: the slab of the robots' state machines (one allocation, g_mem), the staging of the host routes and
    // the `now` of the last begin
    bool has_manager = false, g_begun = false;
    fleet::Params g_params{};
    fleet::Slab g_slab{};
    char *g_mem = nullptr, *g_stage = nullptr;
    double g_now = 0.0;
    // alore_backend_set_classes / _set_problem_classes: the table of configs (and front-end parameters) for bclass::MAX_CLASSES
    // classes, the class and the effective xv of every slot, the counter of clamped indices, the staging of host indices and the
    // records of alore_backend_class_stats; allocated by the first call of that section
    int n_classes = 0; // 0: no table, every slot is planned with cfg
    bool class_fe = false;
    alore_backend_config* k_table = nullptr;
    alore_front_end_params* k_fe = nullptr;
    int *k_class_of = nullptr, *k_clamped = nullptr, *k_stage = nullptr;
    double* k_xv = nullptr;
    alore_backend_class_stat* k_stats = nullptr;
    backend::Params* k_params = nullptr; // the parameter block per class that a launch with classes reads (backend::launch)
};

namespace {

int fail(alore_backend_handle h, int code, const char* what, hipError_t e = hipSuccess)
{
    if (h) {
        h->err = what;
        if (e != hipSuccess) { h->err += ": "; h->err += hipGetErrorString(e); }
    }
    return code;
}
#define BE_TRY(h, call)                                                  \
    do {                                                                 \
        hipError_t e_ = (call);                                          \
        if (e_ != hipSuccess) return fail(h, ALORE_BE_E_HIP, #call, e_); \
    } while (0)

template <class T>
hipError_t dalloc(T** p, size_t count)
{
    hipError_t e = hipMalloc((void**)p, sizeof(T) * (count ? count : 1));
    if (e == hipSuccess) e = hipMemset(*p, 0, sizeof(T) * (count ? count : 1));
    return e;
}

constexpr int MAP_SCANS = 8; // scans per upload of argument blocks

// ends the resident occupancy map; the distance field (d_map) stays the handle's map
void end_map(alore_backend_handle h)
{
    if (!h->resident && !h->h_scan && !h->d_points) return;
    (void)hipDeviceSynchronize();
    void* ptrs[] = {h->omap.grid, h->omap.log_odds, h->omap.count_hit, h->omap.count_all, h->esdf_ws.tmp, h->esdf_ws.pos, h->esdf_ws.neg,
                    h->esdf_ws.v, h->esdf_ws.z, h->d_scan, h->d_points};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (h->h_scan) (void)hipHostFree(h->h_scan);
    delete[] h->omap.h_row;
    h->omap = backend::OccMap{};
    h->esdf_ws = backend::EsdfWorkspace{};
    h->h_scan = h->d_scan = h->d_points = nullptr;
    h->points_bytes = 0;
    h->scan_pending = false;
    h->resident = false;
}

// ends the sensor of alore_backend_laser_create: slabs, tables, cloud and argument block
void end_laser(alore_backend_handle h)
{
    if (!h->has_laser && !h->d_cloud && !h->h_laser) return;
    (void)hipDeviceSynchronize();
    void* ptrs[] = {h->d_cloud, h->l_laser, h->l_world, h->l_compact, h->l_tables, h->l_image, h->l_index, h->l_n, h->l_status, h->d_laser_in};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (h->h_laser) (void)hipHostFree(h->h_laser);
    h->d_cloud = h->l_laser = h->l_world = h->l_compact = nullptr;
    h->l_tables = h->l_image = nullptr;
    h->l_index = h->l_n = h->l_status = nullptr;
    h->h_laser = h->d_laser_in = nullptr;
    h->cloud_cap = 0;
    h->n_cloud = h->laser_scans = h->laser_slots = h->laser_bins = 0;
    h->has_laser = h->has_cloud = h->laser_pending = false;
}

void free_all(alore_backend_handle h)
{
    end_map(h);
    end_laser(h);
    if (h->ev_laser) (void)hipEventDestroy(h->ev_laser);
    if (h->ev_scan) (void)hipEventDestroy(h->ev_scan);
    if (h->ev_scan_done) (void)hipEventDestroy(h->ev_scan_done);
    if (h->d_stamps) {
        long long st[64];
        if (hipMemcpy(st, h->d_stamps, sizeof(st), hipMemcpyDeviceToHost) == hipSuccess) {
            std::fprintf(stderr, "[alore_backend stamps] workgroup 0, cycles per phase of eval_cost (slot 0 also holds the time outside it):");
            for (int i = 0; i < 44; ++i) std::fprintf(stderr, " %lld", st[i]);
            std::fprintf(stderr, "\n");
        }
        (void)hipFree(h->d_stamps);
    }
    void* ptrs[] = {h->d_map, h->d_M, h->d_cut, h->d_inner, h->d_initT, h->d_pos, h->d_head, h->d_tail, h->d_sxy, h->d_fxy, h->d_sxyt,
                    h->r_inner, h->r_T, h->r_coef, h->r_tail, h->r_ok, h->r_status, h->d_hist, h->d_gram, h->d_pcr, h->d_x, h->d_g, h->d_lam, h->d_rho,
                    h->d_cost, h->d_err, h->d_ret, h->d_params, h->d_order, h->d_check_in, h->d_check, h->d_build_in, h->d_build_status,
                    h->d_search_in, h->d_path_n, h->d_path_cost, h->d_search_status, h->d_search_sweeps, h->d_path_xy,
                    h->d_task_in, h->t_status, h->t_matrix, h->t_order, h->t_n_order, h->t_total, h->t_fields, h->t_sweeps, h->t_src_fields,
                    h->t_src_sweeps, h->t_src_range, h->d_task_wide, h->d_task_ticks, h->t_assignment, h->t_assign_total, h->t_leg_start, h->t_leg_goal, h->p_desc, h->p_counters, h->p_host_edits, h->m_slab_mem, h->m_stage, h->m_edits,
                    h->g_mem, h->g_stage, h->k_table, h->k_fe, h->k_class_of, h->k_clamped, h->k_stage, h->k_xv, h->k_stats, h->k_params};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (h->h_task) (void)hipHostFree(h->h_task);
    if (h->ev_task) (void)hipEventDestroy(h->ev_task);
    if (h->ev_task_wide) (void)hipEventDestroy(h->ev_task_wide);
    if (h->h_stage) (void)hipHostFree(h->h_stage);
    if (h->h_check) (void)hipHostFree(h->h_check);
    if (h->h_build) (void)hipHostFree(h->h_build);
    if (h->h_params) (void)hipHostFree(h->h_params);
    if (h->h_search) (void)hipHostFree(h->h_search);
    if (h->ev_search) (void)hipEventDestroy(h->ev_search);
    if (h->d_wide) (void)hipFree(h->d_wide);
    if (h->d_wide_ticks) (void)hipFree(h->d_wide_ticks);
    if (h->ev_wide) (void)hipEventDestroy(h->ev_wide);
    if (h->ev_build) (void)hipEventDestroy(h->ev_build);
    if (h->ev_params) (void)hipEventDestroy(h->ev_params);
    if (h->ev_check) (void)hipEventDestroy(h->ev_check);
    if (h->ev_check_done) (void)hipEventDestroy(h->ev_check_done);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
}

backend::Params base_params(alore_backend_handle h, int count, int mode)
{
    backend::Params p{};
    p.cfg = h->cfg;
    p.map = h->map;
    p.prob = backend::ProblemStore{h->P, h->d_M, h->d_inner, h->d_initT, h->d_pos, h->d_head, h->d_tail, h->d_sxy, h->d_fxy, h->d_cut};
    p.res = backend::ResultStore{h->r_inner, h->r_T, h->r_coef, h->r_tail, h->r_ok, h->r_status};
    p.hist = h->d_hist;
    p.gram = h->d_gram;
    p.pcr = h->d_pcr;
    p.count = count;
    p.mode = mode;
    p.x_io = h->d_x;
    p.g_out = h->d_g;
    p.cost_out = h->d_cost;
    p.err_out = h->d_err;
    p.ret_out = h->d_ret;
    p.stamps = h->d_stamps;
    if (h->n_classes) { p.classes = h->k_table; p.class_of = h->k_class_of; p.class_params = h->k_params; p.n_classes = h->n_classes; }
    return p;
}

constexpr size_t CHECK_ARGS_BYTES = (sizeof(backend::CheckArgs) + 15) & ~size_t(15);
size_t check_in_bytes(size_t B) { return CHECK_ARGS_BYTES + sizeof(double) * 2 * B; }

// the block of alore_backend_set_paths: arguments, then (host route) the inputs of up to B paths of flat_traj::MAX_POINTS points
constexpr size_t BUILD_ARGS_BYTES = (sizeof(backend::BuildArgs) + 15) & ~size_t(15);
struct BuildLayout {
    size_t n_points, xy, start_yaw, end_yaw, vaj, oaj, mask, bytes;
};
BuildLayout build_layout(size_t n, size_t K)
{
    BuildLayout l{};
    size_t at = BUILD_ARGS_BYTES;
    auto take = [&](size_t bytes) { const size_t p = at; at += (bytes + 15) & ~size_t(15); return p; };
    l.n_points = take(sizeof(int) * n);
    l.xy = take(sizeof(double) * n * K * 2);
    l.start_yaw = take(sizeof(double) * n);
    l.end_yaw = take(sizeof(double) * n);
    l.vaj = take(sizeof(double) * n * 3);
    l.oaj = take(sizeof(double) * n * 3);
    l.mask = take(sizeof(int) * n);
    l.bytes = at;
    return l;
}

// the block of alore_backend_search_paths: arguments, then (host route) starts [n][2], goals [n][2] and the mask [n]
constexpr size_t SEARCH_ARGS_BYTES = (sizeof(backend::SearchArgs) + 15) & ~size_t(15);
size_t search_in_bytes(size_t n) { return SEARCH_ARGS_BYTES + sizeof(double) * 4 * n + sizeof(int) * n; }

// the block of alore_backend_laser_scan: arguments, then (host route) the poses [n][3]
constexpr size_t LASER_ARGS_BYTES = (sizeof(backend::LaserArgs) + 15) & ~size_t(15);
size_t laser_in_bytes(size_t n) { return LASER_ARGS_BYTES + sizeof(double) * 3 * n; }

// the block of alore_backend_task_plan: arguments, then (host route) points [n][1 + 2 T][2], n_tasks [n], assignment [n][T], mask [n]
constexpr size_t TASK_ARGS_BYTES = (sizeof(backend::TaskArgs) + 15) & ~size_t(15);
constexpr size_t TASK_MATRIX_INTS = (size_t)tplan::P_MAX * tplan::P_MAX * 2;
size_t task_in_bytes(size_t n, size_t T) { return TASK_ARGS_BYTES + sizeof(double) * 2 * (1 + 2 * T) * n + sizeof(int) * (n + n * T + n); }

} // namespace

extern "C" {

void alore_backend_default_config(alore_backend_config* c)
{
    std::memset(c, 0, sizeof(*c));
    // plan_manager/config/car3ms.yaml
    c->max_vel = 3.0; c->min_vel = 0.0; c->max_acc = 2.0; c->max_omega = 3.0; c->max_domega = 4.0; c->max_cen_acc = 50.0;
    c->direct_v_omega = 0;
    c->n_check = 2;
    c->check_pts[0][0] = 0.3; c->check_pts[1][0] = -0.3;
    // back_end/config/global_planning3ms.yaml
    c->smooth_eps = 0.01;
    c->path_lbfgs = alore_lbfgs_param{256, 2, 8000, 64, 0.0, 5.0e-2, 0.0, 1.0e20, 1.0e-4, 0.9, 1.0e-6, 1.0e-16};
    c->shot_path_past = 8; c->shot_path_horizon = 0.5;
    c->p_time = 20; c->p_bigpath = 200000; c->p_mean_time = 100; c->p_moment = 1000; c->p_acc = 100; c->p_domega = 100;
    c->energy_w[0] = 0.33; c->energy_w[1] = 1.0;
    c->lbfgs = alore_lbfgs_param{256, 3, 8000, 64, 0.0, 5.0e-4, 1.0e-32, 1.0e20, 1.0e-4, 0.9, 1.0e-6, 1.0e-16};
    c->mean_lo = 0.5; c->mean_hi = 2.0;
    c->w_time = 50; c->w_acc = 300; c->w_domega = 300; c->w_collision = 500000; c->w_moment = 300; c->w_mean_time = 300; c->w_cen_acc = 300;
    for (int k = 0; k < 2; ++k) {
        c->lam0[k] = 0; c->rho0[k] = 1.0e4; c->rho_max[k] = 1.0e10; c->gamma[k] = 9.0;
        c->cut_lam0[k] = 0; c->cut_rho0[k] = 1.0e3; c->cut_rho_max[k] = 1.0e10; c->cut_gamma[k] = 5.0;
    }
    c->tol = 0.01; c->cut_tol = 0.5;
    c->sparse_res = 8;
    c->safe_dis = 0.6; c->final_min_safe_dis = 0.10; c->final_check_num = 16; c->safe_replan_max = 3;
    c->icr_xv = 0.2; c->standard_diff = 1; // planner_sim.launch:41-46
    c->max_alm_rounds = 64;
}

int alore_backend_create(const alore_backend_config* cfg, int device, int max_pieces, int max_problems, alore_backend_handle* out)
{
    if (!cfg || !out || max_pieces < 1 || max_problems < 1) return ALORE_BE_E_INVALID;
    *out = nullptr;
    static_assert(bclass::MEM_MAX == backend::MEM_MAX, "backend_classes.h checks mem_size against the history the kernel has");
    if (bclass::invalid_field(*cfg)) return ALORE_BE_E_UNSUPPORTED;
    if (max_pieces > 64) return ALORE_BE_E_UNSUPPORTED;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ALORE_BE_E_NO_DEVICE;
    if (device < 0 || device >= ndev) return ALORE_BE_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return ALORE_BE_E_NO_DEVICE;
    alore_backend_planner* h = new (std::nothrow) alore_backend_planner;
    if (!h) return ALORE_BE_E_NOMEM;
    h->cfg = *cfg;
    h->device = device;
    h->P = max_pieces <= 16 ? 16 : max_pieces <= 32 ? 32 : 64; // three kernel instantiations: piece capacity 16, 32 or 64
    h->B = max_problems;
    const size_t B = (size_t)max_problems, P = (size_t)h->P, ns = 3 * P;
    hipError_t e = hipSuccess;
    auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    A(dalloc(&h->d_M, B)); A(dalloc(&h->d_cut, B)); A(dalloc(&h->d_inner, B * (P - 1) * 2)); A(dalloc(&h->d_initT, B));
    A(dalloc(&h->d_pos, B * P * 2)); A(dalloc(&h->d_head, B * 6)); A(dalloc(&h->d_tail, B * 6)); A(dalloc(&h->d_sxy, B * 2));
    A(dalloc(&h->d_fxy, B * 2)); A(dalloc(&h->d_sxyt, B * 3));
    A(dalloc(&h->r_inner, B * (P - 1) * 2)); A(dalloc(&h->r_T, B * P)); A(dalloc(&h->r_coef, B * P * 12)); A(dalloc(&h->r_tail, B * 6));
    A(dalloc(&h->r_ok, B)); A(dalloc(&h->r_status, B));
    A(dalloc(&h->d_hist, B * backend::MEM_MAX * 2 * ns));
    A(dalloc(&h->d_gram, B * (size_t)backend::GRAM_DOUBLES));
    A(dalloc(&h->d_pcr, B * (size_t)backend::ws_doubles(h->P)));
    if (std::getenv("ALORE_BE_STAMPS")) A(dalloc(&h->d_stamps, (size_t)64));
    A(dalloc(&h->d_x, B * ns)); A(dalloc(&h->d_g, B * ns)); A(dalloc(&h->d_lam, B * 2)); A(dalloc(&h->d_rho, B * 2));
    A(dalloc(&h->d_cost, B)); A(dalloc(&h->d_err, B * 2)); A(dalloc(&h->d_ret, B * 3)); A(dalloc(&h->d_params, 1)); A(dalloc(&h->d_order, B));
    // staging: the largest single transfer is the problem upload / the result download
    h->stage_bytes = B * (sizeof(int) * 2 + sizeof(double) * ((P - 1) * 2 + 1 + P * 2 + 6 + 6 + 2 + 2 + 3 + P * 12 + P + 2 * ns + 8) +
                          sizeof(backend::Status)) + 4096;
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_stage, h->stage_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreate(&h->ev0);
    if (e == hipSuccess) e = hipEventCreate(&h->ev1);
    A(dalloc(&h->d_check, B)); A(dalloc(&h->d_check_in, check_in_bytes(B)));
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_check, check_in_bytes(B), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_check, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_check_done, hipEventDisableTiming);
    const size_t build_bytes = build_layout(B, flat_traj::MAX_POINTS).bytes;
    A(dalloc(&h->d_build_status, B)); A(dalloc(&h->d_build_in, build_bytes));
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_build, build_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_params, sizeof(backend::Params), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_build, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_params, hipEventDisableTiming);
    A(dalloc(&h->d_path_n, B)); A(dalloc(&h->d_path_cost, B * 2)); A(dalloc(&h->d_search_status, B)); A(dalloc(&h->d_search_sweeps, B));
    A(dalloc(&h->d_path_xy, B * psearch::MAX_POINTS * 2)); A(dalloc(&h->d_search_in, search_in_bytes(B)));
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_search, search_in_bytes(B), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_search, hipEventDisableTiming);
    if (e == hipSuccess) e = backend::search_configure();
    if (e == hipSuccess) e = backend::search_wide_configure();
    A(dalloc(&h->t_status, B)); A(dalloc(&h->t_matrix, B * TASK_MATRIX_INTS)); A(dalloc(&h->t_order, B * tplan::MAX_LEGS));
    A(dalloc(&h->t_n_order, B)); A(dalloc(&h->t_total, B * 2)); A(dalloc(&h->t_fields, B)); A(dalloc(&h->t_sweeps, B));
    A(dalloc(&h->t_src_fields, B * tplan::MAX_LEGS)); A(dalloc(&h->t_src_sweeps, B * tplan::MAX_LEGS)); A(dalloc(&h->t_src_range, B * tplan::MAX_LEGS));
    A(dalloc(&h->t_leg_start, B * tplan::MAX_LEGS * 2)); A(dalloc(&h->t_leg_goal, B * tplan::MAX_LEGS * 2));
    A(dalloc(&h->t_assignment, B * tplan::MAX_TASKS)); A(dalloc(&h->t_assign_total, B * 2));
    A(dalloc(&h->d_task_in, task_in_bytes(B, tplan::MAX_TASKS)));
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_task, task_in_bytes(B, tplan::MAX_TASKS), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_task, hipEventDisableTiming);
    if (e == hipSuccess) e = backend::task_configure();
    if (e != hipSuccess) {
        free_all(h);
        delete h;
        return e == hipErrorOutOfMemory ? ALORE_BE_E_NOMEM : ALORE_BE_E_HIP;
    }
    *out = h;
    return ALORE_BE_OK;
}

int alore_backend_destroy(alore_backend_handle h)
{
    if (!h) return ALORE_BE_E_INVALID;
    (void)hipSetDevice(h->device);
    free_all(h);
    delete h;
    return ALORE_BE_OK;
}

const char* alore_backend_last_error(alore_backend_handle h) { return h ? h->err.c_str() : "null handle"; }

int alore_backend_set_map(alore_backend_handle h, const double* dist, int nx, int ny, double x_lo, double y_lo, double res)
{
    if (!h || !dist || nx < 2 || ny < 2 || !(res > 0.0)) return fail(h, ALORE_BE_E_INVALID, "set_map: bad argument");
    BE_TRY(h, hipSetDevice(h->device));
    end_map(h);
    if (h->d_map) { (void)hipFree(h->d_map); h->d_map = nullptr; }
    BE_TRY(h, hipMalloc((void**)&h->d_map, sizeof(double) * (size_t)nx * ny));
    BE_TRY(h, hipMemcpy(h->d_map, dist, sizeof(double) * (size_t)nx * ny, hipMemcpyHostToDevice));
    h->map = backend::MapView{h->d_map, nx, ny, x_lo, y_lo, x_lo + nx * res, y_lo + ny * res, res};
    return ALORE_BE_OK;
}

int alore_backend_build_esdf(alore_backend_handle h, const unsigned char* grid, int nx, int ny, double x_lo, double y_lo, double res,
                             double odom_x, double odom_y, double detection_range, double* dist_out)
{
    if (!h || !grid || nx < 2 || ny < 2 || !(res > 0.0) || !(detection_range > 0.0)) return fail(h, ALORE_BE_E_INVALID, "build_esdf: bad argument");
    BE_TRY(h, hipSetDevice(h->device));
    end_map(h);
    const size_t n = (size_t)nx * ny;
    const bool same = h->d_map && h->map.nx == nx && h->map.ny == ny && h->map.x_lo == x_lo && h->map.y_lo == y_lo && h->map.res == res;
    if (!same) {
        if (h->d_map) { (void)hipFree(h->d_map); h->d_map = nullptr; }
        BE_TRY(h, hipMalloc((void**)&h->d_map, sizeof(double) * n));
        BE_TRY(h, backend::esdf_fill_max(h->d_map, n, nullptr));
        h->map = backend::MapView{h->d_map, nx, ny, x_lo, y_lo, x_lo + nx * res, y_lo + ny * res, res};
    }
    // the window can end one cell past the map (esdf_window.h): esdf_rows then reads up to cell n + ny.  Cells past the grid are
    // unknown (0), as in the resident map, not whatever follows the allocation
    unsigned char* d_grid = nullptr;
    BE_TRY(h, hipMalloc((void**)&d_grid, n + (size_t)ny + 1));
    hipError_t e = hipMemset(d_grid + n, 0, (size_t)ny + 1);
    if (e == hipSuccess) e = hipMemcpy(d_grid, grid, n, hipMemcpyHostToDevice);
    int empty = 0;
    if (e == hipSuccess) e = backend::esdf_update(d_grid, nx, ny, res, x_lo, y_lo, odom_x, odom_y, detection_range, h->d_map, nullptr, &empty);
    (void)hipFree(d_grid);
    if (e != hipSuccess) return fail(h, ALORE_BE_E_HIP, "build_esdf", e);
    if (empty) return fail(h, ALORE_BE_E_INVALID, "build_esdf: the window around the odometry does not intersect the map");
    if (dist_out) BE_TRY(h, hipMemcpy(dist_out, h->d_map, sizeof(double) * n, hipMemcpyDeviceToHost));
    return ALORE_BE_OK;
}

int alore_backend_predicted_state(alore_backend_handle h, int count, double resolution, const double* start_time, const double* time,
                                  const double* start_xytheta, double* xytheta, double* vaj, double* oaj, int* forward)
{
    if (!h || count < 1 || count > h->B || !time || !(resolution > 0.0)) return fail(h, ALORE_BE_E_INVALID, "predicted_state: bad argument");
    if (!h->timed || count > h->count) return fail(h, ALORE_BE_E_INVALID, "predicted_state: no finished plan for these slots (alore_backend_plan first)");
    BE_TRY(h, hipSetDevice(h->device));
    const size_t n = count;
    double *d_in = nullptr, *d_out = nullptr;
    int* d_fwd = nullptr;
    BE_TRY(h, hipMalloc((void**)&d_in, sizeof(double) * n * 5));
    hipError_t e = hipMalloc((void**)&d_out, sizeof(double) * n * 9);
    if (e == hipSuccess) e = hipMalloc((void**)&d_fwd, sizeof(int) * n);
    if (e == hipSuccess) e = hipMemcpy(d_in, time, sizeof(double) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess && start_time) e = hipMemcpy(d_in + n, start_time, sizeof(double) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess && start_xytheta) e = hipMemcpy(d_in + 2 * n, start_xytheta, sizeof(double) * n * 3, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        backend::PredictArgs g{count, h->P, h->d_M, h->r_T, h->r_coef, h->d_sxyt, start_time ? d_in + n : nullptr, d_in,
                               start_xytheta ? d_in + 2 * n : nullptr, resolution, h->cfg.icr_xv, h->cfg.standard_diff != 0,
                               d_out, d_out + 3 * n, d_out + 6 * n, d_fwd};
        if (h->n_classes) { g.classes = h->k_table; g.class_of = h->k_class_of; }
        e = backend::predicted_state(g, nullptr);
    }
    if (e == hipSuccess && xytheta) e = hipMemcpy(xytheta, d_out, sizeof(double) * n * 3, hipMemcpyDeviceToHost);
    if (e == hipSuccess && vaj) e = hipMemcpy(vaj, d_out + 3 * n, sizeof(double) * n * 3, hipMemcpyDeviceToHost);
    if (e == hipSuccess && oaj) e = hipMemcpy(oaj, d_out + 6 * n, sizeof(double) * n * 3, hipMemcpyDeviceToHost);
    if (e == hipSuccess && forward) e = hipMemcpy(forward, d_fwd, sizeof(int) * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_fwd);
    if (e != hipSuccess) return fail(h, ALORE_BE_E_HIP, "predicted_state", e);
    return ALORE_BE_OK;
}

int alore_backend_predicted_state_device(alore_backend_handle h, int count, double resolution, const double* d_start_time,
                                         const double* d_time, const double* d_start_xytheta, double* d_xytheta, double* d_vaj,
                                         double* d_oaj, int* d_forward, void* stream)
{
    if (!h || count < 1 || count > h->B || !d_time || !d_xytheta || !d_vaj || !d_oaj || !d_forward || !(resolution > 0.0))
        return fail(h, ALORE_BE_E_INVALID, "predicted_state_device: bad argument");
    if (!h->timed || count > h->count) return fail(h, ALORE_BE_E_INVALID, "predicted_state_device: no plan for these slots (alore_backend_plan first)");
    BE_TRY(h, hipSetDevice(h->device));
    backend::PredictArgs g{count, h->P, h->d_M, h->r_T, h->r_coef, h->d_sxyt, d_start_time, d_time, d_start_xytheta, resolution,
                           h->cfg.icr_xv, h->cfg.standard_diff != 0, d_xytheta, d_vaj, d_oaj, d_forward};
    if (h->n_classes) { g.classes = h->k_table; g.class_of = h->k_class_of; }
    BE_TRY(h, backend::predicted_state(g, (hipStream_t)stream));
    return ALORE_BE_OK;
}

int alore_backend_path_points(alore_backend_handle h, int count, int panels_per_piece, double* xy, double* yaw, int* n_points)
{
    if (!h || count < 1 || count > h->B || panels_per_piece < 1 || !xy || !n_points)
        return fail(h, ALORE_BE_E_INVALID, "path_points: bad argument");
    if (!h->timed || count > h->count) return fail(h, ALORE_BE_E_INVALID, "path_points: no finished plan for these slots (alore_backend_plan first)");
    BE_TRY(h, hipSetDevice(h->device));
    const size_t n = count, per = (size_t)h->P * (panels_per_piece + 1);
    double *d_xy = nullptr, *d_yaw = nullptr;
    int* d_n = nullptr;
    hipError_t e = hipMalloc((void**)&d_xy, sizeof(double) * n * per * 2);
    if (e == hipSuccess) e = hipMemset(d_xy, 0, sizeof(double) * n * per * 2);
    if (e == hipSuccess && yaw) e = hipMalloc((void**)&d_yaw, sizeof(double) * n * h->P * panels_per_piece);
    if (e == hipSuccess && yaw) e = hipMemset(d_yaw, 0, sizeof(double) * n * h->P * panels_per_piece);
    if (e == hipSuccess) e = hipMalloc((void**)&d_n, sizeof(int) * n);
    if (e == hipSuccess) {
        backend::PathArgs g{count, h->P, panels_per_piece, h->d_M, h->r_ok, h->r_T, h->r_coef, h->d_sxyt, h->cfg.icr_xv, h->cfg.standard_diff != 0,
                            d_xy, d_yaw, d_n};
        if (h->n_classes) { g.classes = h->k_table; g.class_of = h->k_class_of; }
        e = backend::path_points(g, nullptr);
    }
    if (e == hipSuccess) e = hipMemcpy(xy, d_xy, sizeof(double) * n * per * 2, hipMemcpyDeviceToHost);
    if (e == hipSuccess && yaw) e = hipMemcpy(yaw, d_yaw, sizeof(double) * n * h->P * panels_per_piece, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(n_points, d_n, sizeof(int) * n, hipMemcpyDeviceToHost);
    (void)hipFree(d_xy); (void)hipFree(d_yaw); (void)hipFree(d_n);
    if (e != hipSuccess) return fail(h, ALORE_BE_E_HIP, "path_points", e);
    return ALORE_BE_OK;
}

int alore_backend_path_points_device(alore_backend_handle h, int count, int panels_per_piece, double* d_xy, double* d_yaw, int* d_n_points, void* stream)
{
    if (!h || count < 1 || count > h->B || panels_per_piece < 1 || !d_xy || !d_n_points)
        return fail(h, ALORE_BE_E_INVALID, "path_points_device: bad argument");
    if (!h->timed || count > h->count) return fail(h, ALORE_BE_E_INVALID, "path_points_device: no plan for these slots (alore_backend_plan first)");
    BE_TRY(h, hipSetDevice(h->device));
    backend::PathArgs g{count, h->P, panels_per_piece, h->d_M, h->r_ok, h->r_T, h->r_coef, h->d_sxyt, h->cfg.icr_xv, h->cfg.standard_diff != 0,
                        d_xy, d_yaw, d_n_points};
    if (h->n_classes) { g.classes = h->k_table; g.class_of = h->k_class_of; }
    BE_TRY(h, backend::path_points(g, (hipStream_t)stream));
    return ALORE_BE_OK;
}

int alore_backend_set_problems(alore_backend_handle h, int count, const alore_flat_traj* pr, void* stream)
{
    if (!h || count < 1 || count > h->B || !pr) return fail(h, ALORE_BE_E_INVALID, "set_problems: bad argument");
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t P = h->P, n = count;
    // carve the pinned slab
    char* base = h->h_stage;
    auto take = [&](size_t bytes) { char* p = base; base += (bytes + 15) & ~size_t(15); return p; };
    int* hM = (int*)take(sizeof(int) * n);
    int* hcut = (int*)take(sizeof(int) * n);
    double* hin = (double*)take(sizeof(double) * n * (P - 1) * 2);
    double* hT = (double*)take(sizeof(double) * n);
    double* hpos = (double*)take(sizeof(double) * n * P * 2);
    double* hhead = (double*)take(sizeof(double) * n * 6);
    double* htail = (double*)take(sizeof(double) * n * 6);
    double* hs = (double*)take(sizeof(double) * n * 2);
    double* hf = (double*)take(sizeof(double) * n * 2);
    double* hst = (double*)take(sizeof(double) * n * 3);
    std::memset(h->h_stage, 0, (size_t)(base - h->h_stage));
    for (int b = 0; b < count; ++b) {
        const alore_flat_traj& f = pr[b];
        const int M = f.n_pieces;
        if (M < 1) return fail(h, ALORE_BE_E_INVALID, "set_problems: a problem has no pieces");
        if (M > h->P) return fail(h, ALORE_BE_E_UNSUPPORTED, "set_problems: more pieces than the handle was created for");
        if (M > 1 && (!f.traj_pts || !f.positions)) return fail(h, ALORE_BE_E_INVALID, "set_problems: null array");
        hM[b] = M;
        hcut[b] = f.if_cut;
        hT[b] = f.init_T;
        for (int i = 0; i < M - 1; ++i) {
            hin[(size_t)b * (P - 1) * 2 + 2 * i] = f.traj_pts[3 * i];
            hin[(size_t)b * (P - 1) * 2 + 2 * i + 1] = f.traj_pts[3 * i + 1];
            hpos[(size_t)b * P * 2 + 2 * i] = f.positions[3 * i];
            hpos[(size_t)b * P * 2 + 2 * i + 1] = f.positions[3 * i + 1];
        }
        hpos[(size_t)b * P * 2 + 2 * (M - 1)] = f.final_xytheta[0];
        hpos[(size_t)b * P * 2 + 2 * (M - 1) + 1] = f.final_xytheta[1];
        for (int d = 0; d < 2; ++d)
            for (int k = 0; k < 3; ++k) { hhead[(size_t)b * 6 + d * 3 + k] = f.start_state[d][k]; htail[(size_t)b * 6 + d * 3 + k] = f.final_state[d][k]; }
        for (int k = 0; k < 2; ++k) { hs[(size_t)b * 2 + k] = f.start_xytheta[k]; hf[(size_t)b * 2 + k] = f.final_xytheta[k]; }
        for (int k = 0; k < 3; ++k) hst[(size_t)b * 3 + k] = f.start_xytheta[k];
    }
    {   // launch order: most pieces first.  The number of cost evaluations grows with the number of pieces (correlation 0.5
        // on the Monte-Carlo goals) and a launch ends with its slowest wavefront: the long problems must not start last
        // (measured on 2048 problems: 45 -> 37 ms; with the evaluation counts known in advance 35 ms).
        std::vector<int> ord(n);
        for (size_t b = 0; b < n; ++b) ord[b] = (int)b;
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b2) { return hM[a] > hM[b2]; });
        BE_TRY(h, hipMemcpy(h->d_order, ord.data(), sizeof(int) * n, hipMemcpyHostToDevice));
    }
    BE_TRY(h, hipMemcpyAsync(h->d_M, hM, sizeof(int) * n, hipMemcpyHostToDevice, s));
    BE_TRY(h, hipMemcpyAsync(h->d_cut, hcut, sizeof(int) * n, hipMemcpyHostToDevice, s));
    BE_TRY(h, hipMemcpyAsync(h->d_inner, hin, sizeof(double) * n * (P - 1) * 2, hipMemcpyHostToDevice, s));
    BE_TRY(h, hipMemcpyAsync(h->d_initT, hT, sizeof(double) * n, hipMemcpyHostToDevice, s));
    BE_TRY(h, hipMemcpyAsync(h->d_pos, hpos, sizeof(double) * n * P * 2, hipMemcpyHostToDevice, s));
    BE_TRY(h, hipMemcpyAsync(h->d_head, hhead, sizeof(double) * n * 6, hipMemcpyHostToDevice, s));
    BE_TRY(h, hipMemcpyAsync(h->d_tail, htail, sizeof(double) * n * 6, hipMemcpyHostToDevice, s));
    BE_TRY(h, hipMemcpyAsync(h->d_sxy, hs, sizeof(double) * n * 2, hipMemcpyHostToDevice, s));
    BE_TRY(h, hipMemcpyAsync(h->d_fxy, hf, sizeof(double) * n * 2, hipMemcpyHostToDevice, s));
    BE_TRY(h, hipMemcpyAsync(h->d_sxyt, hst, sizeof(double) * n * 3, hipMemcpyHostToDevice, s));
    BE_TRY(h, hipStreamSynchronize(s)); // the slab is reused by the next call
    h->count = count;
    return ALORE_BE_OK;
}

void alore_front_end_default_params(alore_front_end_params* p)
{
    std::memset(p, 0, sizeof(*p));
    flat_traj::default_params(p);
}

int alore_backend_set_paths(alore_backend_handle h, int count, const alore_backend_paths* p, const alore_front_end_params* fe,
                            int device_pointers, const int* mask, int mask_stride_bytes, void* stream)
{
    if (!h || count < 1 || count > h->B || !p || !p->n_points || !p->xy || !p->start_yaw || !p->end_yaw)
        return fail(h, ALORE_BE_E_INVALID, "set_paths: bad argument");
    if (p->max_points < 2 || p->max_points > flat_traj::MAX_POINTS) return fail(h, ALORE_BE_E_UNSUPPORTED, "set_paths: max_points must be 2 .. 31");
    if (mask && (mask_stride_bytes < (int)sizeof(int) || mask_stride_bytes % (int)sizeof(int)))
        return fail(h, ALORE_BE_E_INVALID, "set_paths: the mask stride must be a positive multiple of sizeof(int)");
    alore_front_end_params prm;
    if (fe) prm = *fe; else alore_front_end_default_params(&prm);
    if (!(prm.sample_time > 0.0) || !(prm.max_vel > 0.0) || !(prm.max_acc > 0.0) || prm.min_traj_num < 1)
        return fail(h, ALORE_BE_E_INVALID, "set_paths: sample_time, max_vel, max_acc and min_traj_num must be positive");
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->build_pending) BE_TRY(h, hipEventSynchronize(h->ev_build)); // the pinned block is free again
    h->build_pending = false;
    const size_t n = count, K = p->max_points;
    backend::BuildArgs g{};
    g.count = count; g.P = h->P; g.K = p->max_points;
    g.fe = prm;
    if (!fe && h->n_classes && h->class_fe) { g.fe_classes = h->k_fe; g.class_of = h->k_class_of; } // the slot's class's parameters
    size_t up = BUILD_ARGS_BYTES;
    if (device_pointers) {
        g.n_points = p->n_points; g.xy = p->xy; g.start_yaw = p->start_yaw; g.end_yaw = p->end_yaw;
        g.start_vaj = p->start_vaj; g.start_oaj = p->start_oaj;
        g.mask = mask; g.mask_stride = mask ? mask_stride_bytes : 0;
    } else {
        const BuildLayout l = build_layout(n, K);
        char *hb = h->h_build, *db = h->d_build_in;
        std::memcpy(hb + l.n_points, p->n_points, sizeof(int) * n);
        std::memcpy(hb + l.xy, p->xy, sizeof(double) * n * K * 2);
        std::memcpy(hb + l.start_yaw, p->start_yaw, sizeof(double) * n);
        std::memcpy(hb + l.end_yaw, p->end_yaw, sizeof(double) * n);
        if (p->start_vaj) std::memcpy(hb + l.vaj, p->start_vaj, sizeof(double) * n * 3);
        if (p->start_oaj) std::memcpy(hb + l.oaj, p->start_oaj, sizeof(double) * n * 3);
        if (mask)
            for (size_t b = 0; b < n; ++b) ((int*)(hb + l.mask))[b] = *(const int*)((const char*)mask + b * (size_t)mask_stride_bytes);
        g.n_points = (const int*)(db + l.n_points); g.xy = (const double*)(db + l.xy);
        g.start_yaw = (const double*)(db + l.start_yaw); g.end_yaw = (const double*)(db + l.end_yaw);
        g.start_vaj = p->start_vaj ? (const double*)(db + l.vaj) : nullptr;
        g.start_oaj = p->start_oaj ? (const double*)(db + l.oaj) : nullptr;
        g.mask = mask ? (const int*)(db + l.mask) : nullptr;
        g.mask_stride = mask ? (int)sizeof(int) : 0;
        up = l.bytes;
    }
    g.M = h->d_M; g.if_cut = h->d_cut; g.inner = h->d_inner; g.init_T = h->d_initT; g.positions = h->d_pos; g.head = h->d_head;
    g.tail = h->d_tail; g.start_xy = h->d_sxy; g.final_xy = h->d_fxy; g.sxyt = h->d_sxyt;
    g.status = h->d_build_status; g.order = h->d_order;
    std::memcpy(h->h_build, &g, sizeof(g));
    BE_TRY(h, hipMemcpyAsync(h->d_build_in, h->h_build, up, hipMemcpyHostToDevice, s));
    BE_TRY(h, hipEventRecord(h->ev_build, s));
    h->build_pending = true;
    BE_TRY(h, backend::build_problems((const backend::BuildArgs*)h->d_build_in, count, h->P, s));
    h->count = count;
    if (!device_pointers) {
        int* hst = (int*)h->h_stage;
        BE_TRY(h, hipMemcpyAsync(hst, h->d_build_status, sizeof(int) * n, hipMemcpyDeviceToHost, s));
        BE_TRY(h, hipStreamSynchronize(s));
        for (size_t b = 0; b < n; ++b) {
            if (hst[b] == flat_traj::E_POINTS) return fail(h, ALORE_BE_E_INVALID, "set_paths: a path has fewer than 2 or more than max_points way-points");
            if (hst[b] == flat_traj::E_PIECES) return fail(h, ALORE_BE_E_UNSUPPORTED, "set_paths: more pieces than the handle was created for");
        }
    }
    return ALORE_BE_OK;
}

int alore_backend_device_build_status(alore_backend_handle h, const int** out)
{
    if (!h || !out) return fail(h, ALORE_BE_E_INVALID, "device_build_status: bad argument");
    *out = h->d_build_status;
    return ALORE_BE_OK;
}

int alore_backend_build_status(alore_backend_handle h, int count, int* out)
{
    if (!h || count < 1 || count > h->B || !out) return fail(h, ALORE_BE_E_INVALID, "build_status: bad argument");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize());
    BE_TRY(h, hipMemcpy(out, h->d_build_status, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost));
    return ALORE_BE_OK;
}

int alore_backend_launch_order(alore_backend_handle h, int count, int* out)
{
    if (!h || count < 1 || count > h->B || !out) return fail(h, ALORE_BE_E_INVALID, "launch_order: bad argument");
    if (count != h->count) return fail(h, ALORE_BE_E_INVALID, "launch_order: the order covers the slots of the last set_problems / set_paths, all of them");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize());
    BE_TRY(h, hipMemcpy(out, h->d_order, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost));
    return ALORE_BE_OK;
}

int alore_backend_get_problems(alore_backend_handle h, int count, int* n_pieces, double* inner, double* init_T, double* positions,
                               double* head, double* tail, double* start_xytheta, double* final_xy, int* if_cut)
{
    if (!h || count < 1 || count > h->B) return fail(h, ALORE_BE_E_INVALID, "get_problems: bad argument");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize());
    const size_t n = count, P = h->P;
    if (n_pieces) BE_TRY(h, hipMemcpy(n_pieces, h->d_M, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (inner) BE_TRY(h, hipMemcpy(inner, h->d_inner, sizeof(double) * n * (P - 1) * 2, hipMemcpyDeviceToHost));
    if (init_T) BE_TRY(h, hipMemcpy(init_T, h->d_initT, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (positions) BE_TRY(h, hipMemcpy(positions, h->d_pos, sizeof(double) * n * P * 2, hipMemcpyDeviceToHost));
    if (head) BE_TRY(h, hipMemcpy(head, h->d_head, sizeof(double) * n * 6, hipMemcpyDeviceToHost));
    if (tail) BE_TRY(h, hipMemcpy(tail, h->d_tail, sizeof(double) * n * 6, hipMemcpyDeviceToHost));
    if (start_xytheta) BE_TRY(h, hipMemcpy(start_xytheta, h->d_sxyt, sizeof(double) * n * 3, hipMemcpyDeviceToHost));
    if (final_xy) BE_TRY(h, hipMemcpy(final_xy, h->d_fxy, sizeof(double) * n * 2, hipMemcpyDeviceToHost));
    if (if_cut) BE_TRY(h, hipMemcpy(if_cut, h->d_cut, sizeof(int) * n, hipMemcpyDeviceToHost));
    return ALORE_BE_OK;
}

int alore_backend_plan(alore_backend_handle h, int count, void* stream)
{
    if (!h || count < 1 || count > h->count) return fail(h, ALORE_BE_E_INVALID, "plan: upload the problems first");
    if (!h->d_map) return fail(h, ALORE_BE_E_INVALID, "plan: no map (alore_backend_set_map)");
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    backend::Params p = base_params(h, count, backend::MODE_PLAN);
    if (count == h->count) p.order = h->d_order; // the whole uploaded set: longest problems first
    BE_TRY(h, hipEventRecord(h->ev0, s));
    BE_TRY(h, backend::launch(p, h->d_params, h->P, s));
    BE_TRY(h, hipEventRecord(h->ev1, s));
    h->timed = true;
    return ALORE_BE_OK;
}

int alore_backend_plan_masked(alore_backend_handle h, int count, const int* mask, int mask_stride_bytes, void* stream)
{
    if (!h || count < 1 || count > h->count) return fail(h, ALORE_BE_E_INVALID, "plan_masked: upload the problems first");
    if (!h->d_map) return fail(h, ALORE_BE_E_INVALID, "plan_masked: no map (alore_backend_set_map)");
    if (mask && (mask_stride_bytes < (int)sizeof(int) || mask_stride_bytes % (int)sizeof(int)))
        return fail(h, ALORE_BE_E_INVALID, "plan_masked: the mask stride must be a positive multiple of sizeof(int)");
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->params_pending) BE_TRY(h, hipEventSynchronize(h->ev_params)); // the pinned block is free again
    h->params_pending = false;
    *h->h_params = base_params(h, count, backend::MODE_PLAN);
    if (count == h->count) h->h_params->order = h->d_order;
    h->h_params->mask = mask;
    h->h_params->mask_stride = mask ? mask_stride_bytes : 0;
    BE_TRY(h, hipEventRecord(h->ev0, s));
    BE_TRY(h, backend::launch(*h->h_params, h->d_params, h->P, s));
    BE_TRY(h, hipEventRecord(h->ev_params, s));
    h->params_pending = true;
    BE_TRY(h, hipEventRecord(h->ev1, s));
    h->timed = true;
    return ALORE_BE_OK;
}

// out[b] = 1 where the last check flags a collision AND the slot was searched, built and planned with success: the slots whose plan is
// NEW and may be delivered.  (alore_backend_plan_masked plans a flagged slot whose search or build failed again from its old problem:
// that plan must not go out under a new start time.)
static __global__ void replan_mask_kernel(const alore_backend_check* check, const int* search_status, const int* build_status, const int* ok,
                                          int count, int* out)
{
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= count) return;
    out[b] = (check[b].collision != 0 && search_status[b] == ALORE_BE_SEARCH_OK && build_status[b] == ALORE_BE_BUILD_OK && ok[b] != 0) ? 1 : 0;
}

int alore_backend_replan_mask(alore_backend_handle h, int count, int* out_mask, void* stream)
{
    if (!h || count < 1 || count > h->B || !out_mask) return fail(h, ALORE_BE_E_INVALID, "replan_mask: bad argument");
    BE_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(replan_mask_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->d_check,
                       h->d_search_status, h->d_build_status, h->r_ok, count, out_mask);
    BE_TRY(h, hipGetLastError());
    return ALORE_BE_OK;
}

// ---- object classes ----------------------------------------------------------------------------------------------------------
// Slot b takes the index in[b] (in null: keeps its own), brought into the table of n classes: an index read from `in` is clamped
// and counted, a kept one that the table no longer holds becomes class 0.  xv[b] is the effective ICR offset of the slot's class
// (table null: xv0, the handle's config's).
static __global__ void class_assign_kernel(const int* in, int count, int n, const alore_backend_config* table, double xv0, int* class_of,
                                           double* xv, int* clamped)
{
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= count) return;
    int k = in ? in[b] : class_of[b];
    if (in) {
        const int c = bclass::clamp_class(k, n);
        if (c != k) atomicAdd(clamped, 1);
        k = c;
    } else if (k < 0 || k >= n) k = 0;
    class_of[b] = k;
    xv[b] = table ? bclass::effective_xv(table[k]) : xv0;
}

// One workgroup per class: every thread folds the slots of the class in its stride (bclass::stat_add), the workgroup folds its
// threads in a tree (bclass::stat_merge).  Integer sums, minima and maxima: the result does not depend on either order.
static __global__ __launch_bounds__(256) void class_stats_kernel(const int* class_of, const alore_backend_status* status, const double* T, int P,
                                                                 int count, alore_backend_class_stat* out)
{
    __shared__ alore_backend_class_stat sh[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    alore_backend_class_stat s;
    bclass::stat_init(s);
    for (int b = tid; b < count; b += 256) {
        if ((class_of ? class_of[b] : 0) != k) continue;
        const alore_backend_status st = status[b];
        bclass::stat_add(s, st, bclass::plan_duration(T + (size_t)b * P, bclass::pieces_of(st, P)));
    }
    sh[tid] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) bclass::stat_merge(sh[tid], sh[tid + w]);
        __syncthreads();
    }
    if (tid == 0) out[k] = sh[0];
}

// the buffers of this section, once: every slot class 0 with the xv of the handle's config
static int ensure_classes(alore_backend_handle h)
{
    if (h->k_class_of) return ALORE_BE_OK;
    BE_TRY(h, hipSetDevice(h->device));
    const size_t B = (size_t)h->B;
    hipError_t e = hipSuccess;
    auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    A(dalloc(&h->k_table, (size_t)bclass::MAX_CLASSES)); A(dalloc(&h->k_fe, (size_t)bclass::MAX_CLASSES)); A(dalloc(&h->k_clamped, 1));
    A(dalloc(&h->k_stage, B)); A(dalloc(&h->k_xv, B)); A(dalloc(&h->k_stats, (size_t)bclass::MAX_CLASSES)); A(dalloc(&h->k_class_of, B));
    A(dalloc(&h->k_params, (size_t)bclass::MAX_CLASSES));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(class_assign_kernel, dim3((unsigned)((h->B + 255) / 256)), dim3(256), 0, nullptr, (const int*)nullptr, h->B,
                           bclass::MAX_CLASSES, (const alore_backend_config*)nullptr, bclass::effective_xv(h->cfg), h->k_class_of, h->k_xv, h->k_clamped);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        void* ptrs[] = {h->k_table, h->k_fe, h->k_clamped, h->k_stage, h->k_xv, h->k_stats, h->k_class_of, h->k_params};
        for (void* p : ptrs)
            if (p) (void)hipFree(p);
        h->k_table = nullptr; h->k_fe = nullptr; h->k_clamped = h->k_stage = h->k_class_of = nullptr; h->k_xv = nullptr; h->k_stats = nullptr; h->k_params = nullptr;
        return fail(h, e == hipErrorOutOfMemory ? ALORE_BE_E_NOMEM : ALORE_BE_E_HIP, "classes: allocation", e);
    }
    return ALORE_BE_OK;
}

int alore_backend_set_classes(alore_backend_handle h, int n_classes, const alore_backend_config* classes, const alore_front_end_params* fe)
{
    if (!h || n_classes < 0 || n_classes > bclass::MAX_CLASSES || (n_classes > 0 && !classes))
        return fail(h, ALORE_BE_E_INVALID, "set_classes: n_classes must be 0 .. 256, with a table");
    for (int k = 0; k < n_classes; ++k) {
        if (const char* f = bclass::class_error(classes[k], h->cfg)) {
            const bool sizing = bclass::sizing_mismatch(classes[k], h->cfg) != nullptr;
            h->err = "set_classes: class " + std::to_string(k) + ": " + f + (sizing ? " must equal the handle's" : " is outside what this build supports");
            return ALORE_BE_E_INVALID;
        }
        if (fe && (!(fe[k].sample_time > 0.0) || !(fe[k].max_vel > 0.0) || !(fe[k].max_acc > 0.0) || fe[k].min_traj_num < 1)) {
            h->err = "set_classes: class " + std::to_string(k) + ": front-end sample_time, max_vel, max_acc and min_traj_num must be positive";
            return ALORE_BE_E_INVALID;
        }
    }
    if (int rc = ensure_classes(h)) return rc;
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize()); // a launch in flight may still read the table
    if (n_classes) BE_TRY(h, hipMemcpy(h->k_table, classes, sizeof(alore_backend_config) * (size_t)n_classes, hipMemcpyHostToDevice));
    if (n_classes && fe) BE_TRY(h, hipMemcpy(h->k_fe, fe, sizeof(alore_front_end_params) * (size_t)n_classes, hipMemcpyHostToDevice));
    h->n_classes = n_classes;
    h->class_fe = n_classes > 0 && fe != nullptr;
    // without a table the indices stay as they are (nothing reads them) and every xv is the handle's config's
    hipLaunchKernelGGL(class_assign_kernel, dim3((unsigned)((h->B + 255) / 256)), dim3(256), 0, nullptr, (const int*)nullptr, h->B,
                       n_classes ? n_classes : bclass::MAX_CLASSES, n_classes ? (const alore_backend_config*)h->k_table : nullptr,
                       bclass::effective_xv(h->cfg), h->k_class_of, h->k_xv, h->k_clamped);
    BE_TRY(h, hipGetLastError());
    BE_TRY(h, hipDeviceSynchronize());
    return ALORE_BE_OK;
}

int alore_backend_set_problem_classes(alore_backend_handle h, int count, const int* class_of, int device_pointer, void* stream)
{
    if (!h || count < 1 || count > h->B || !class_of) return fail(h, ALORE_BE_E_INVALID, "set_problem_classes: bad argument");
    const int n = h->n_classes ? h->n_classes : 1;
    if (!device_pointer)
        for (int b = 0; b < count; ++b)
            if (class_of[b] < 0 || class_of[b] >= n) {
                h->err = "set_problem_classes: slot " + std::to_string(b) + " has class " + std::to_string(class_of[b]) + ", outside the table of " +
                         std::to_string(n);
                return ALORE_BE_E_INVALID;
            }
    if (int rc = ensure_classes(h)) return rc;
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int* src = class_of;
    if (!device_pointer) {
        BE_TRY(h, hipMemcpyAsync(h->k_stage, class_of, sizeof(int) * (size_t)count, hipMemcpyHostToDevice, s));
        src = h->k_stage;
    }
    hipLaunchKernelGGL(class_assign_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, src, count, n,
                       h->n_classes ? (const alore_backend_config*)h->k_table : nullptr, bclass::effective_xv(h->cfg), h->k_class_of, h->k_xv,
                       h->k_clamped);
    BE_TRY(h, hipGetLastError());
    if (!device_pointer) BE_TRY(h, hipStreamSynchronize(s));
    return ALORE_BE_OK;
}

int alore_backend_device_classes(alore_backend_handle h, alore_backend_class_view* out)
{
    if (!h || !out) return fail(h, ALORE_BE_E_INVALID, "device_classes: bad argument");
    if (int rc = ensure_classes(h)) return rc;
    out->n_classes = h->n_classes;
    out->pad = 0;
    out->class_of = h->k_class_of;
    out->xv = h->k_xv;
    out->clamped = h->k_clamped;
    out->classes = h->n_classes ? h->k_table : nullptr;
    out->stats = h->k_stats;
    return ALORE_BE_OK;
}

int alore_backend_class_stats(alore_backend_handle h, int count, alore_backend_class_stat* out, void* stream)
{
    if (!h || count < 1 || count > h->B) return fail(h, ALORE_BE_E_INVALID, "class_stats: bad argument");
    if (!h->timed || count > h->count) return fail(h, ALORE_BE_E_INVALID, "class_stats: no plan has run for these slots (alore_backend_plan first)");
    if (int rc = ensure_classes(h)) return rc;
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int n = h->n_classes ? h->n_classes : 1;
    hipLaunchKernelGGL(class_stats_kernel, dim3((unsigned)n), dim3(256), 0, s, h->n_classes ? (const int*)h->k_class_of : nullptr,
                       (const alore_backend_status*)h->r_status, (const double*)h->r_T, h->P, count, h->k_stats);
    BE_TRY(h, hipGetLastError());
    if (out) {
        BE_TRY(h, hipMemcpyAsync(out, h->k_stats, sizeof(alore_backend_class_stat) * (size_t)n, hipMemcpyDeviceToHost, s));
        BE_TRY(h, hipStreamSynchronize(s));
    }
    return ALORE_BE_OK;
}

int alore_backend_last_plan_ms(alore_backend_handle h, float* ms)
{
    if (!h || !ms || !h->timed) return fail(h, ALORE_BE_E_INVALID, "last_plan_ms: no plan yet");
    BE_TRY(h, hipEventSynchronize(h->ev1));
    BE_TRY(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
    return ALORE_BE_OK;
}

int alore_backend_results(alore_backend_handle h, int count, alore_backend_status* status, double* inner, double* T, double* coef,
                          void* stream)
{
    if (!h || count < 1 || count > h->B) return fail(h, ALORE_BE_E_INVALID, "results: bad argument");
    if (!h->timed || count > h->count) return fail(h, ALORE_BE_E_INVALID, "results: no plan has run for these slots (alore_backend_plan first)");
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t P = h->P, n = count;
    char* base = h->h_stage;
    auto take = [&](size_t bytes) { char* p = base; base += (bytes + 15) & ~size_t(15); return p; };
    backend::Status* hs = (backend::Status*)take(sizeof(backend::Status) * n);
    double* hin = (double*)take(sizeof(double) * n * (P - 1) * 2);
    double* hT = (double*)take(sizeof(double) * n * P);
    double* hc = (double*)take(sizeof(double) * n * P * 12);
    if (status) BE_TRY(h, hipMemcpyAsync(hs, h->r_status, sizeof(backend::Status) * n, hipMemcpyDeviceToHost, s));
    if (inner) BE_TRY(h, hipMemcpyAsync(hin, h->r_inner, sizeof(double) * n * (P - 1) * 2, hipMemcpyDeviceToHost, s));
    if (T) BE_TRY(h, hipMemcpyAsync(hT, h->r_T, sizeof(double) * n * P, hipMemcpyDeviceToHost, s));
    if (coef) BE_TRY(h, hipMemcpyAsync(hc, h->r_coef, sizeof(double) * n * P * 12, hipMemcpyDeviceToHost, s));
    BE_TRY(h, hipStreamSynchronize(s));
    if (status) std::memcpy(status, hs, sizeof(backend::Status) * n);
    if (inner) std::memcpy(inner, hin, sizeof(double) * n * (P - 1) * 2);
    if (T) std::memcpy(T, hT, sizeof(double) * n * P);
    if (coef) std::memcpy(coef, hc, sizeof(double) * n * P * 12);
    return ALORE_BE_OK;
}

int alore_backend_device_results(alore_backend_handle h, alore_backend_device_view* out)
{
    if (!h || !out) return ALORE_BE_E_INVALID;
    out->max_pieces = h->P;
    out->n_pieces = h->d_M;
    out->inner = h->r_inner;
    out->T = h->r_T;
    out->coef = h->r_coef;
    out->head = h->d_head;
    out->tail = h->r_tail;
    out->start_xytheta = h->d_sxyt;
    out->ok = h->r_ok;
    return ALORE_BE_OK;
}

int alore_backend_check_plans(alore_backend_handle h, int count, const double* t_from, const double* t_to, double min_safe_dis, int body,
                              alore_backend_check* out, void* stream)
{
    if (!h) return ALORE_BE_E_INVALID;
    if (count < 1 || count > h->B) return fail(h, ALORE_BE_E_INVALID, "check_plans: count out of range");
    if (!std::isfinite(min_safe_dis)) return fail(h, ALORE_BE_E_INVALID, "check_plans: min_safe_dis is not finite");
    if (body && !h->n_classes && h->cfg.n_check == 0) return fail(h, ALORE_BE_E_INVALID, "check_plans: body check asked for, but the configuration has no check points");
    if (!h->d_map) return fail(h, ALORE_BE_E_INVALID, "check_plans: no map (alore_backend_set_map / alore_backend_build_esdf)");
    if (!h->timed || count > h->count) return fail(h, ALORE_BE_E_INVALID, "check_plans: no finished plan for these slots (alore_backend_plan first)");
    for (int b = 0; b < count; ++b) { // the caller's arrays last: only a call that can run reads them
        if ((t_from && !std::isfinite(t_from[b])) || (t_to && !std::isfinite(t_to[b]))) return fail(h, ALORE_BE_E_INVALID, "check_plans: a window bound is not finite");
        if (t_to && t_to[b] < (t_from ? t_from[b] : 0.0)) return fail(h, ALORE_BE_E_INVALID, "check_plans: a window ends before it begins");
    }
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->check_pending) {
        BE_TRY(h, hipEventSynchronize(h->ev_check));         // the pinned block is free again
        BE_TRY(h, hipStreamWaitEvent(s, h->ev_check_done, 0)); // the previous check (on whatever stream) has read its arguments and written its records
    }
    h->check_pending = false;
    const size_t n = count;
    double *h_win = (double*)(h->h_check + CHECK_ARGS_BYTES), *d_win = (double*)(h->d_check_in + CHECK_ARGS_BYTES);
    backend::CheckArgs g{};
    g.count = count; g.P = h->P; g.R = h->cfg.final_check_num; g.n_check = h->cfg.n_check; g.body = body != 0;
    g.n_pieces = h->d_M; g.T = h->r_T; g.coef = h->r_coef; g.plan_start_xyt = h->d_sxyt;
    g.map = h->map;
    g.t_from = t_from ? d_win : nullptr;
    g.t_to = t_to ? d_win + n : nullptr;
    g.min_safe_dis = min_safe_dis > 0.0 ? min_safe_dis : h->cfg.final_min_safe_dis;
    g.xv = h->cfg.standard_diff ? 0.0 : h->cfg.icr_xv;
    std::memcpy(g.check_pts, h->cfg.check_pts, sizeof(g.check_pts));
    g.out = h->d_check;
    if (h->n_classes) { g.classes = h->k_table; g.class_of = h->k_class_of; g.use_class_thr = min_safe_dis > 0.0 ? 0 : 1; }
    std::memcpy(h->h_check, &g, sizeof(g));
    if (t_from) std::memcpy(h_win, t_from, sizeof(double) * n);
    if (t_to) std::memcpy(h_win + n, t_to, sizeof(double) * n);
    BE_TRY(h, hipMemcpyAsync(h->d_check_in, h->h_check, CHECK_ARGS_BYTES + sizeof(double) * 2 * n, hipMemcpyHostToDevice, s));
    BE_TRY(h, hipEventRecord(h->ev_check, s));
    h->check_pending = true;
    BE_TRY(h, backend::check_plans((const backend::CheckArgs*)h->d_check_in, count, s));
    BE_TRY(h, hipEventRecord(h->ev_check_done, s));
    if (out) {
        BE_TRY(h, hipMemcpyAsync(h->h_stage, h->d_check, sizeof(alore_backend_check) * n, hipMemcpyDeviceToHost, s));
        BE_TRY(h, hipStreamSynchronize(s));
        std::memcpy(out, h->h_stage, sizeof(alore_backend_check) * n);
    }
    return ALORE_BE_OK;
}

int alore_backend_device_check(alore_backend_handle h, const alore_backend_check** out)
{
    if (!h || !out) return fail(h, ALORE_BE_E_INVALID, "device_check: bad argument");
    *out = h->d_check;
    return ALORE_BE_OK;
}

static int run_piece(alore_backend_handle h, int count, int mode, int stage, double* x, const double* lam, const double* rho,
                     double safe_dis, double time_weight, int max_iter, double* cost, double* grad, int* ret, int* iters, int* evals,
                     double* xy_err, void* stream)
{
    if (!h || count < 1 || count > h->count || !x || (stage != 1 && stage != 2))
        return fail(h, ALORE_BE_E_INVALID, "eval/lbfgs: bad argument (upload the problems first)");
    if (!h->d_map) return fail(h, ALORE_BE_E_INVALID, "eval/lbfgs: no map");
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t ns = 3 * (size_t)h->P, n = count;
    BE_TRY(h, hipMemcpyAsync(h->d_x, x, sizeof(double) * n * ns, hipMemcpyHostToDevice, s));
    if (lam) BE_TRY(h, hipMemcpyAsync(h->d_lam, lam, sizeof(double) * n * 2, hipMemcpyHostToDevice, s));
    if (rho) BE_TRY(h, hipMemcpyAsync(h->d_rho, rho, sizeof(double) * n * 2, hipMemcpyHostToDevice, s));
    backend::Params p = base_params(h, count, mode);
    p.stage = stage;
    p.max_iter = max_iter;
    p.lam_in = lam ? h->d_lam : nullptr;
    p.rho_in = rho ? h->d_rho : nullptr;
    // NaN: the configured value.  Without a table that is the handle's config, here; with one the slot's class's, which
    // class_params_kernel writes into the class's copy of the block (backend::launch)
    p.safe_dis = std::isnan(safe_dis) && !h->n_classes ? h->cfg.safe_dis : safe_dis;
    p.time_weight = std::isnan(time_weight) && !h->n_classes ? h->cfg.w_time : time_weight;
    BE_TRY(h, backend::launch(p, h->d_params, h->P, s));
    std::vector<int> r3((size_t)n * 3);
    if (cost) BE_TRY(h, hipMemcpyAsync(cost, h->d_cost, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    if (grad) BE_TRY(h, hipMemcpyAsync(grad, h->d_g, sizeof(double) * n * ns, hipMemcpyDeviceToHost, s));
    if (xy_err) BE_TRY(h, hipMemcpyAsync(xy_err, h->d_err, sizeof(double) * n * 2, hipMemcpyDeviceToHost, s));
    BE_TRY(h, hipMemcpyAsync(r3.data(), h->d_ret, sizeof(int) * n * 3, hipMemcpyDeviceToHost, s));
    if (mode == backend::MODE_LBFGS) BE_TRY(h, hipMemcpyAsync(x, h->d_x, sizeof(double) * n * ns, hipMemcpyDeviceToHost, s));
    BE_TRY(h, hipStreamSynchronize(s));
    for (size_t b = 0; b < n; ++b) {
        if (ret) ret[b] = r3[b * 3];
        if (iters) iters[b] = r3[b * 3 + 1];
        if (evals) evals[b] = r3[b * 3 + 2];
    }
    return ALORE_BE_OK;
}

int alore_backend_eval(alore_backend_handle h, int count, int stage, const double* x, const double* lam, const double* rho,
                       double safe_dis, double time_weight, double* cost, double* grad, double* xy_err, void* stream)
{
    return run_piece(h, count, backend::MODE_EVAL, stage, const_cast<double*>(x), lam, rho, safe_dis, time_weight, 0, cost, grad, nullptr,
                     nullptr, nullptr, xy_err, stream);
}

int alore_backend_lbfgs(alore_backend_handle h, int count, int stage, double* x, const double* lam, const double* rho, double safe_dis,
                        double time_weight, int max_iter, double* cost, int* ret, int* iters, int* evals, double* xy_err, void* stream)
{
    return run_piece(h, count, backend::MODE_LBFGS, stage, x, lam, rho, safe_dis, time_weight, max_iter, cost, nullptr, ret, iters, evals,
                     xy_err, stream);
}

// ---- the resident occupancy map ----------------------------------------------------------------------------------------------
void alore_backend_map_default_params(alore_backend_map_params* p)
{
    std::memset(p, 0, sizeof(*p));
    p->p_hit = 0.99; p->p_miss = 0.35; p->p_min = 0.12; p->p_max = 0.90; p->p_occ = 0.80; // plan_env/config/mapsim.yaml
    p->detection_range = 27.0; p->perspective = 1;                                           // planner_sim.launch
}

int alore_backend_map_create(alore_backend_handle h, int nx, int ny, double x_lo, double y_lo, double res, const alore_backend_map_params* params)
{
    if (!h) return ALORE_BE_E_INVALID;
    alore_backend_map_params prm;
    if (params) prm = *params; else alore_backend_map_default_params(&prm);
    auto prob = [](double p) { return p > 0.0 && p < 1.0; };
    if (nx < 2 || ny < 2 || nx > 32768 || ny > 32768 || !(res > 0.0) || !std::isfinite(res) || !std::isfinite(x_lo) || !std::isfinite(y_lo))
        return fail(h, ALORE_BE_E_INVALID, "map_create: bad geometry");
    if (!prob(prm.p_hit) || !prob(prm.p_miss) || !prob(prm.p_min) || !prob(prm.p_max) || !prob(prm.p_occ) || !(prm.p_min < prm.p_max) ||
        !(prm.detection_range > 0.0) || !std::isfinite(prm.detection_range) || !(prm.detection_range / res < 1.0e6))
        return fail(h, ALORE_BE_E_INVALID, "map_create: probabilities must lie in (0, 1) with p_min < p_max, detection_range must be positive");
    BE_TRY(h, hipSetDevice(h->device));
    end_map(h);
    if (h->d_map) { (void)hipFree(h->d_map); h->d_map = nullptr; }
    h->map = backend::MapView{};
    const size_t n = (size_t)nx * ny;
    backend::OccMap& m = h->omap;
    m.nx = nx; m.ny = ny; m.x_lo = x_lo; m.y_lo = y_lo; m.res = res; m.range = prm.detection_range; m.perspective = prm.perspective != 0;
    backend::occ_log_odds(prm, m.log_odds5);
    m.h_row = new (std::nothrow) double[(size_t)backend::occ_lattice_cap(m.range, res)];
    backend::EsdfWorkspace& w = h->esdf_ws;
    backend::esdf_workspace_size(nx, ny, res, m.range, &w.cells, &w.lines);
    h->scan_block = backend::occ_block_bytes(nx, ny);
    hipError_t e = m.h_row ? hipSuccess : hipErrorOutOfMemory;
    auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    // the ESDF's window can end one cell past the map where ceil((nx res) / res) or ceil((ny res) / res) rounds up (as in the
    // reference): esdf_rows then reads up to the whole row nx, cells n .. n + ny.  They are zeros (unknown) here, not whatever
    // follows the allocation
    A(dalloc(&m.grid, n + (size_t)ny + 1)); A(dalloc(&m.count_hit, n)); A(dalloc(&m.count_all, n));
    if (e == hipSuccess) e = hipMalloc((void**)&m.log_odds, sizeof(double) * n);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_map, sizeof(double) * n);
    if (e == hipSuccess) e = hipMalloc((void**)&w.tmp, sizeof(double) * w.cells);
    if (e == hipSuccess) e = hipMalloc((void**)&w.pos, sizeof(double) * w.cells);
    if (e == hipSuccess) e = hipMalloc((void**)&w.neg, sizeof(double) * w.cells);
    if (e == hipSuccess) e = hipMalloc((void**)&w.v, sizeof(int) * (size_t)w.lines * (w.lines + 2));
    if (e == hipSuccess) e = hipMalloc((void**)&w.z, sizeof(double) * (size_t)w.lines * (w.lines + 3));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_scan, h->scan_block * MAP_SCANS);
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_scan, h->scan_block * MAP_SCANS, hipHostMallocDefault);
    if (e == hipSuccess && !h->ev_scan) e = hipEventCreateWithFlags(&h->ev_scan, hipEventDisableTiming);
    if (e == hipSuccess && !h->ev_scan_done) e = hipEventCreateWithFlags(&h->ev_scan_done, hipEventDisableTiming);
    if (e == hipSuccess) e = backend::occ_fill(m.log_odds, n, m.log_odds5[2] - 0.01, nullptr);
    if (e == hipSuccess) e = backend::esdf_fill_max(h->d_map, n, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    h->resident = true; // end_map frees what was allocated
    if (e != hipSuccess) {
        end_map(h);
        if (h->d_map) { (void)hipFree(h->d_map); h->d_map = nullptr; }
        return fail(h, e == hipErrorOutOfMemory ? ALORE_BE_E_NOMEM : ALORE_BE_E_HIP, "map_create", e);
    }
    h->map = backend::MapView{h->d_map, nx, ny, x_lo, y_lo, x_lo + nx * res, y_lo + ny * res, res};
    return ALORE_BE_OK;
}

#define BE_MAP(h, what)                                                                                                   \
    do {                                                                                                                  \
        if (!h) return ALORE_BE_E_INVALID;                                                                                \
        if (!h->resident) return fail(h, ALORE_BE_E_INVALID, what ": no resident map (alore_backend_map_create; alore_backend_set_map and alore_backend_build_esdf end it)"); \
    } while (0)

int alore_backend_map_logodds(alore_backend_handle h, double out[5])
{
    BE_MAP(h, "map_logodds");
    if (!out) return fail(h, ALORE_BE_E_INVALID, "map_logodds: bad argument");
    std::memcpy(out, h->omap.log_odds5, sizeof(double) * 5);
    return ALORE_BE_OK;
}

int alore_backend_map_set_grid(alore_backend_handle h, const unsigned char* grid)
{
    BE_MAP(h, "map_set_grid");
    if (!grid) return fail(h, ALORE_BE_E_INVALID, "map_set_grid: bad argument");
    const size_t n = (size_t)h->omap.nx * h->omap.ny;
    for (size_t c = 0; c < n; ++c)
        if (grid[c] > 2) return fail(h, ALORE_BE_E_INVALID, "map_set_grid: a cell state is not 0, 1 or 2");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize());
    BE_TRY(h, hipMemcpy(h->omap.grid, grid, n, hipMemcpyHostToDevice));
    return ALORE_BE_OK;
}

int alore_backend_map_integrate(alore_backend_handle h, int n_scans, const alore_backend_scan* scans, int device_points, int update_esdf,
                                void* stream)
{
    BE_MAP(h, "map_integrate");
    if (n_scans < 1 || !scans) return fail(h, ALORE_BE_E_INVALID, "map_integrate: bad argument");
    const backend::OccMap& m = h->omap;
    size_t stage = 0;
    for (int k = 0; k < n_scans; ++k) {
        const alore_backend_scan& sc = scans[k];
        if (sc.n_points < 0 || (sc.n_points > 0 && !sc.points) || sc.point_stride_bytes < 8 || sc.point_stride_bytes % 4)
            return fail(h, ALORE_BE_E_INVALID, "map_integrate: a scan needs n_points >= 0, points, and a stride that is a multiple of 4 and at least 8");
        if (!(sc.odom[0] > m.x_lo && sc.odom[0] < m.x_lo + m.nx * m.res && sc.odom[1] > m.y_lo && sc.odom[1] < m.y_lo + m.ny * m.res))
            return fail(h, ALORE_BE_E_INVALID, "map_integrate: the sensor position of a scan is not strictly inside the map");
        if (sc.n_points > 0) stage += (((size_t)(sc.n_points - 1) * sc.point_stride_bytes + 8) + 15) & ~size_t(15);
    }
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (!device_points && stage > h->points_bytes) {
        BE_TRY(h, hipDeviceSynchronize()); // an earlier call on another stream may still read the old buffer
        if (h->d_points) { (void)hipFree(h->d_points); h->d_points = nullptr; h->points_bytes = 0; }
        BE_TRY(h, hipMalloc((void**)&h->d_points, stage));
        h->points_bytes = stage;
    }
    // the map_integrate and map_update_esdf calls before (on whatever stream) have read their blocks and left the ESDF workspace;
    // an event that was never recorded does not hold the stream
    BE_TRY(h, hipStreamWaitEvent(s, h->ev_scan_done, 0));
    size_t at = 0;
    for (int first = 0; first < n_scans; first += MAP_SCANS) {
        const int chunk = std::min(MAP_SCANS, n_scans - first);
        if (h->scan_pending) BE_TRY(h, hipEventSynchronize(h->ev_scan)); // the pinned blocks are free again
        h->scan_pending = false;
        for (int k = 0; k < chunk; ++k) {
            const alore_backend_scan& sc = scans[first + k];
            const char* pts = (const char*)sc.points;
            if (!device_points && sc.n_points > 0) {
                const size_t bytes = (size_t)(sc.n_points - 1) * sc.point_stride_bytes + 8;
                BE_TRY(h, hipMemcpyAsync(h->d_points + at, sc.points, bytes, hipMemcpyHostToDevice, s));
                pts = h->d_points + at;
                at += (bytes + 15) & ~size_t(15);
            }
            if (!backend::occ_prepare_scan(m, sc.odom[0], sc.odom[1], pts, sc.n_points, sc.point_stride_bytes, h->h_scan + k * h->scan_block,
                                           h->d_scan + k * h->scan_block))
                return fail(h, ALORE_BE_E_INVALID, "map_integrate: the sensor position of a scan is not strictly inside the map");
        }
        BE_TRY(h, hipMemcpyAsync(h->d_scan, h->h_scan, h->scan_block * chunk, hipMemcpyHostToDevice, s));
        BE_TRY(h, hipEventRecord(h->ev_scan, s));
        h->scan_pending = true;
        for (int k = 0; k < chunk; ++k) {
            const alore_backend_scan& sc = scans[first + k];
            BE_TRY(h, backend::occ_enqueue_scan(h->h_scan + k * h->scan_block, h->d_scan + k * h->scan_block, s));
            if (update_esdf) {
                int empty = 0;
                BE_TRY(h, backend::esdf_enqueue(m.grid, m.nx, m.ny, m.res, m.x_lo, m.y_lo, sc.odom[0], sc.odom[1], m.range, h->d_map, h->esdf_ws, s, &empty));
            }
        }
        BE_TRY(h, hipEventRecord(h->ev_scan_done, s));
    }
    if (!device_points) BE_TRY(h, hipStreamSynchronize(s));
    return ALORE_BE_OK;
}

int alore_backend_map_update_esdf(alore_backend_handle h, double odom_x, double odom_y, double detection_range, void* stream)
{
    BE_MAP(h, "map_update_esdf");
    if (!std::isfinite(odom_x) || !std::isfinite(odom_y) || !(detection_range > 0.0) || !std::isfinite(detection_range))
        return fail(h, ALORE_BE_E_INVALID, "map_update_esdf: bad argument");
    BE_TRY(h, hipSetDevice(h->device));
    const backend::OccMap& m = h->omap;
    int empty = 0;
    // one ESDF workspace serves every call: wait for the map_integrate or map_update_esdf before, on whatever stream it ran
    BE_TRY(h, hipStreamWaitEvent((hipStream_t)stream, h->ev_scan_done, 0));
    const hipError_t e = backend::esdf_enqueue(m.grid, m.nx, m.ny, m.res, m.x_lo, m.y_lo, odom_x, odom_y, detection_range, h->d_map, h->esdf_ws,
                                               (hipStream_t)stream, &empty);
    if (e == hipErrorInvalidValue) return fail(h, ALORE_BE_E_INVALID, "map_update_esdf: the window is larger than the map's detection range allows");
    if (e != hipSuccess) return fail(h, ALORE_BE_E_HIP, "map_update_esdf", e);
    if (empty) return fail(h, ALORE_BE_E_INVALID, "map_update_esdf: the window around the odometry does not intersect the map");
    BE_TRY(h, hipEventRecord(h->ev_scan_done, (hipStream_t)stream));
    return ALORE_BE_OK;
}

int alore_backend_map_get(alore_backend_handle h, unsigned char* grid, double* log_odds, double* dist)
{
    BE_MAP(h, "map_get");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize());
    const size_t n = (size_t)h->omap.nx * h->omap.ny;
    if (grid) BE_TRY(h, hipMemcpy(grid, h->omap.grid, n, hipMemcpyDeviceToHost));
    if (log_odds) BE_TRY(h, hipMemcpy(log_odds, h->omap.log_odds, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (dist) BE_TRY(h, hipMemcpy(dist, h->d_map, sizeof(double) * n, hipMemcpyDeviceToHost));
    return ALORE_BE_OK;
}

int alore_backend_map_device(alore_backend_handle h, alore_backend_map_view* out)
{
    BE_MAP(h, "map_device");
    if (!out) return fail(h, ALORE_BE_E_INVALID, "map_device: bad argument");
    const backend::OccMap& m = h->omap;
    *out = alore_backend_map_view{m.grid, m.log_odds, h->d_map, m.count_hit, m.count_all, m.nx, m.ny, m.x_lo, m.y_lo, m.res};
    return ALORE_BE_OK;
}

void alore_backend_laser_default_params(alore_backend_laser_params* p)
{
    laser::Params d;
    laser::default_params(&d);
    *p = alore_backend_laser_params{d.sensing_horizon, d.pc_resolution, d.hrz_laser_line_num, d.vtc_laser_line_num, d.vtc_laser_range_dgr,
                                    d.hrz_limited, d.hrz_laser_range_dgr, d.use_resolution_filter, d.if_perspective};
}

int alore_backend_laser_create(alore_backend_handle h, const alore_backend_laser_params* params, int max_scans, int max_points_per_scan)
{
    if (!h) return ALORE_BE_E_INVALID;
    alore_backend_laser_params prm;
    if (params) prm = *params; else alore_backend_laser_default_params(&prm);
    const laser::Params lp{prm.sensing_horizon, prm.pc_resolution, prm.hrz_laser_line_num, prm.vtc_laser_line_num, prm.vtc_laser_range_dgr,
                           prm.hrz_limited, prm.hrz_laser_range_dgr, prm.use_resolution_filter, prm.if_perspective};
    if (!laser::valid(lp))
        return fail(h, ALORE_BE_E_INVALID, "laser_create: needs vtc_laser_line_num >= 2, hrz_laser_line_num >= 1, at most 8192 bins, a positive horizon and resolution, vtc_laser_range_dgr in (0, 180)");
    if (max_scans < 1 || (lp.if_perspective && max_points_per_scan < 1))
        return fail(h, ALORE_BE_E_INVALID, "laser_create: max_scans and, in perspective mode, max_points_per_scan must be at least 1");
    BE_TRY(h, hipSetDevice(h->device));
    end_laser(h);
    const laser::Derived d = laser::derive(lp);
    const size_t S = (size_t)max_scans, bins = (size_t)d.hrz * d.vtc, slots = d.perspective ? (size_t)max_points_per_scan : bins;
    std::vector<double> tables((size_t)laser::table_doubles(d));
    laser::make_tables(d, tables.data());
    hipError_t e = hipSuccess;
    auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    h->has_laser = true; // end_laser frees what was allocated
    A(hipMalloc((void**)&h->l_tables, sizeof(double) * tables.size()));
    A(hipMalloc((void**)&h->l_laser, sizeof(float) * S * slots * 3));
    A(hipMalloc((void**)&h->l_world, sizeof(float) * S * slots * 3));
    A(hipMalloc((void**)&h->l_index, sizeof(int) * S * slots));
    if (!d.perspective) {
        A(hipMalloc((void**)&h->l_image, sizeof(double) * S * bins));
        A(hipMalloc((void**)&h->l_compact, sizeof(float) * S * slots * 3));
    }
    A(dalloc(&h->l_n, S)); A(dalloc(&h->l_status, S));
    A(hipMalloc((void**)&h->d_laser_in, laser_in_bytes(S)));
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_laser, laser_in_bytes(S), hipHostMallocDefault);
    if (e == hipSuccess && !h->ev_laser) e = hipEventCreateWithFlags(&h->ev_laser, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemcpy(h->l_tables, tables.data(), sizeof(double) * tables.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = backend::laser_configure();
    if (e != hipSuccess) {
        end_laser(h);
        return fail(h, e == hipErrorOutOfMemory ? ALORE_BE_E_NOMEM : ALORE_BE_E_HIP, "laser_create", e);
    }
    h->laser_d = d;
    h->laser_scans = max_scans; h->laser_slots = (int)slots; h->laser_bins = (int)bins;
    return ALORE_BE_OK;
}

int alore_backend_laser_set_cloud(alore_backend_handle h, const float* points, int n, int stride_bytes, int device_points, void* stream)
{
    if (!h) return ALORE_BE_E_INVALID;
    if (!h->has_laser) return fail(h, ALORE_BE_E_INVALID, "laser_set_cloud: no sensor (alore_backend_laser_create)");
    if (n < 0 || n > (1 << 30) || (n > 0 && !points) || stride_bytes < 12 || stride_bytes % 4)
        return fail(h, ALORE_BE_E_INVALID, "laser_set_cloud: needs 0 <= n <= 2^30, points, and a stride that is a multiple of 4 and at least 12");
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if ((size_t)n > h->cloud_cap || !h->d_cloud) {
        BE_TRY(h, hipDeviceSynchronize()); // a scan on another stream may still read the old cloud
        if (h->d_cloud) { (void)hipFree(h->d_cloud); h->d_cloud = nullptr; h->cloud_cap = 0; }
        h->has_cloud = false;
        BE_TRY(h, hipMalloc((void**)&h->d_cloud, sizeof(float) * 3 * (size_t)(n ? n : 1)));
        h->cloud_cap = (size_t)(n ? n : 1);
    }
    if (n > 0 && device_points) {
        BE_TRY(h, hipMemcpy2DAsync(h->d_cloud, 12, points, (size_t)stride_bytes, 12, (size_t)n, hipMemcpyDeviceToDevice, s));
    } else if (n > 0) {
        std::vector<float> packed(3 * (size_t)n);
        for (size_t i = 0; i < (size_t)n; ++i) std::memcpy(&packed[3 * i], (const char*)points + i * (size_t)stride_bytes, 12);
        BE_TRY(h, hipMemcpyAsync(h->d_cloud, packed.data(), sizeof(float) * packed.size(), hipMemcpyHostToDevice, s));
        BE_TRY(h, hipStreamSynchronize(s));
    }
    h->n_cloud = n;
    h->has_cloud = true;
    return ALORE_BE_OK;
}

int alore_backend_laser_scan(alore_backend_handle h, int count, const double* poses, int pose_stride_bytes, int device_poses, void* stream)
{
    if (!h) return ALORE_BE_E_INVALID;
    if (!h->has_laser) return fail(h, ALORE_BE_E_INVALID, "laser_scan: no sensor (alore_backend_laser_create)");
    if (!h->has_cloud) return fail(h, ALORE_BE_E_INVALID, "laser_scan: no world cloud (alore_backend_laser_set_cloud)");
    if (count < 1 || count > h->laser_scans || !poses) return fail(h, ALORE_BE_E_INVALID, "laser_scan: count must be 1 .. max_scans, poses not NULL");
    const int three = 3 * (int)sizeof(double);
    if (pose_stride_bytes < three || pose_stride_bytes % (int)sizeof(double))
        return fail(h, ALORE_BE_E_INVALID, "laser_scan: the pose stride must be a multiple of 8, at least 24");
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->laser_pending) BE_TRY(h, hipEventSynchronize(h->ev_laser)); // the pinned block is free again
    h->laser_pending = false;
    const size_t n = count;
    backend::LaserArgs g{};
    g.count = count; g.n_cloud = h->n_cloud; g.slots = h->laser_slots;
    g.d = h->laser_d;
    g.cloud = h->d_cloud;
    g.tables = h->l_tables;
    size_t up = LASER_ARGS_BYTES;
    if (device_poses) {
        g.poses = poses; g.pose_stride = pose_stride_bytes;
    } else {
        double* hp = (double*)(h->h_laser + LASER_ARGS_BYTES);
        for (size_t i = 0; i < n; ++i) std::memcpy(hp + 3 * i, (const char*)poses + i * (size_t)pose_stride_bytes, three);
        g.poses = (const double*)(h->d_laser_in + LASER_ARGS_BYTES); g.pose_stride = three;
        up = laser_in_bytes(n);
    }
    g.image = h->l_image; g.laser_pts = h->l_laser; g.world_pts = h->l_world; g.index = h->l_index; g.compact = h->l_compact;
    g.n_points = h->l_n; g.status = h->l_status;
    std::memcpy(h->h_laser, &g, sizeof(g));
    BE_TRY(h, hipMemcpyAsync(h->d_laser_in, h->h_laser, up, hipMemcpyHostToDevice, s));
    BE_TRY(h, hipEventRecord(h->ev_laser, s));
    h->laser_pending = true;
    BE_TRY(h, backend::laser_scan((const backend::LaserArgs*)h->d_laser_in, count, h->laser_d.perspective, h->laser_bins, s));
    if (!device_poses) BE_TRY(h, hipStreamSynchronize(s));
    return ALORE_BE_OK;
}

int alore_backend_device_laser(alore_backend_handle h, alore_backend_laser_view* out)
{
    if (!h || !out) return fail(h, ALORE_BE_E_INVALID, "device_laser: bad argument");
    if (!h->has_laser) return fail(h, ALORE_BE_E_INVALID, "device_laser: no sensor (alore_backend_laser_create)");
    *out = alore_backend_laser_view{h->l_image, h->l_laser, h->l_world, h->l_index, h->laser_d.perspective ? h->l_laser : h->l_compact,
                                    h->l_n, h->l_status, h->laser_slots, h->laser_bins, h->laser_scans};
    return ALORE_BE_OK;
}

int alore_backend_get_laser(alore_backend_handle h, int count, double* range_image, float* laser_points, float* world_points, int* index,
                            float* compact_points, int* n_points, int* status)
{
    if (!h) return ALORE_BE_E_INVALID;
    if (!h->has_laser) return fail(h, ALORE_BE_E_INVALID, "get_laser: no sensor (alore_backend_laser_create)");
    if (count < 1 || count > h->laser_scans) return fail(h, ALORE_BE_E_INVALID, "get_laser: count must be 1 .. max_scans");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize());
    const size_t n = count, pts = n * (size_t)h->laser_slots;
    if (range_image && h->l_image) BE_TRY(h, hipMemcpy(range_image, h->l_image, sizeof(double) * n * (size_t)h->laser_bins, hipMemcpyDeviceToHost));
    if (laser_points) BE_TRY(h, hipMemcpy(laser_points, h->l_laser, sizeof(float) * pts * 3, hipMemcpyDeviceToHost));
    if (world_points) BE_TRY(h, hipMemcpy(world_points, h->l_world, sizeof(float) * pts * 3, hipMemcpyDeviceToHost));
    if (index) BE_TRY(h, hipMemcpy(index, h->l_index, sizeof(int) * pts, hipMemcpyDeviceToHost));
    if (compact_points)
        BE_TRY(h, hipMemcpy(compact_points, h->laser_d.perspective ? h->l_laser : h->l_compact, sizeof(float) * pts * 3, hipMemcpyDeviceToHost));
    if (n_points) BE_TRY(h, hipMemcpy(n_points, h->l_n, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (status) BE_TRY(h, hipMemcpy(status, h->l_status, sizeof(int) * n, hipMemcpyDeviceToHost));
    return ALORE_BE_OK;
}

void alore_backend_search_default_params(alore_backend_search_params* p)
{
    psearch::Params d;
    psearch::default_params(&d);
    p->safe_dis = d.safe_dis;
    p->window_margin = d.window_margin;
}

int alore_backend_search_paths(alore_backend_handle h, int count, const double* start_xy, int start_stride_bytes, const double* goal_xy,
                               int goal_stride_bytes, const alore_backend_search_params* params, int device_pointers, const int* mask,
                               int mask_stride_bytes, void* stream)
{
    if (!h || count < 1 || count > h->B || !start_xy || !goal_xy) return fail(h, ALORE_BE_E_INVALID, "search_paths: bad argument");
    const int two = 2 * (int)sizeof(double);
    if (start_stride_bytes < two || start_stride_bytes % (int)sizeof(double) || goal_stride_bytes < two || goal_stride_bytes % (int)sizeof(double))
        return fail(h, ALORE_BE_E_INVALID, "search_paths: the strides of start and goal must be multiples of 8, at least 16");
    if (mask && (mask_stride_bytes < (int)sizeof(int) || mask_stride_bytes % (int)sizeof(int)))
        return fail(h, ALORE_BE_E_INVALID, "search_paths: the mask stride must be a positive multiple of sizeof(int)");
    alore_backend_search_params prm;
    if (params) prm = *params; else alore_backend_search_default_params(&prm);
    if (!std::isfinite(prm.safe_dis) || !std::isfinite(prm.window_margin) || prm.window_margin < 0.0)
        return fail(h, ALORE_BE_E_INVALID, "search_paths: safe_dis must be finite, window_margin finite and not negative");
    if (!h->d_map) return fail(h, ALORE_BE_E_INVALID, "search_paths: no map (alore_backend_set_map / alore_backend_build_esdf / alore_backend_map_create)");
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->search_pending) BE_TRY(h, hipEventSynchronize(h->ev_search)); // the pinned block is free again
    h->search_pending = false;
    const size_t n = count;
    backend::SearchArgs g{};
    g.count = count;
    g.map = h->map;
    g.safe_dis = prm.safe_dis;
    g.window_margin = prm.window_margin;
    size_t up = SEARCH_ARGS_BYTES;
    if (device_pointers) {
        g.start = start_xy; g.start_stride = start_stride_bytes;
        g.goal = goal_xy; g.goal_stride = goal_stride_bytes;
        g.mask = mask; g.mask_stride = mask ? mask_stride_bytes : 0;
    } else {
        double *hs = (double*)(h->h_search + SEARCH_ARGS_BYTES), *hg = hs + 2 * n;
        int* hm = (int*)(hg + 2 * n);
        for (size_t b = 0; b < n; ++b) {
            const double* ps = (const double*)((const char*)start_xy + b * (size_t)start_stride_bytes);
            const double* pg = (const double*)((const char*)goal_xy + b * (size_t)goal_stride_bytes);
            hs[2 * b] = ps[0]; hs[2 * b + 1] = ps[1];
            hg[2 * b] = pg[0]; hg[2 * b + 1] = pg[1];
            if (mask) hm[b] = *(const int*)((const char*)mask + b * (size_t)mask_stride_bytes);
        }
        double* ds = (double*)(h->d_search_in + SEARCH_ARGS_BYTES);
        g.start = ds; g.start_stride = two;
        g.goal = ds + 2 * n; g.goal_stride = two;
        g.mask = mask ? (const int*)(ds + 4 * n) : nullptr;
        g.mask_stride = mask ? (int)sizeof(int) : 0;
        up = search_in_bytes(n);
    }
    const long long map_cells = (long long)h->map.nx * h->map.ny;
    g.lds_cells = map_cells < psearch::MAX_CELLS ? (int)map_cells : psearch::MAX_CELLS;
    g.n_points = h->d_path_n; g.xy = h->d_path_xy; g.cost_ab = h->d_path_cost; g.status = h->d_search_status; g.sweeps = h->d_search_sweeps;
    g.wide_slabs = h->d_wide; g.wide_cells = h->wide_cells; g.wide_slots = h->wide_slots; g.wide_ticks = h->d_wide_ticks;
    std::memcpy(h->h_search, &g, sizeof(g));
    BE_TRY(h, hipMemcpyAsync(h->d_search_in, h->h_search, up, hipMemcpyHostToDevice, s));
    BE_TRY(h, hipEventRecord(h->ev_search, s));
    h->search_pending = true;
    BE_TRY(h, backend::search_paths((const backend::SearchArgs*)h->d_search_in, count, g.lds_cells, s));
    if (h->d_wide) { // the slots that the first kernel left at E_WINDOW, on the reservation's slabs
        BE_TRY(h, backend::search_paths_wide((const backend::SearchArgs*)h->d_search_in, h->wide_slots, s));
        BE_TRY(h, hipEventRecord(h->ev_wide, s));
        h->wide_pending = true;
    }
    if (!device_pointers) {
        int* hst = (int*)h->h_stage;
        BE_TRY(h, hipMemcpyAsync(hst, h->d_search_status, sizeof(int) * n, hipMemcpyDeviceToHost, s));
        BE_TRY(h, hipStreamSynchronize(s));
        for (size_t b = 0; b < n; ++b) {
            if (hst[b] == psearch::E_ENDPOINT) return fail(h, ALORE_BE_E_INVALID, "search_paths: an end point is not finite or outside the map");
            if (hst[b] == psearch::E_SAME_CELL) return fail(h, ALORE_BE_E_INVALID, "search_paths: start and goal lie in one cell");
            if (hst[b] == psearch::E_NO_PATH) return fail(h, ALORE_BE_E_INVALID, "search_paths: no path inside the window");
            if (hst[b] == psearch::E_WINDOW)
                return fail(h, ALORE_BE_E_UNSUPPORTED, "search_paths: the window has more than 32768 cells, or more than the reservation");
            if (hst[b] == psearch::E_RANGE)
                return fail(h, ALORE_BE_E_UNSUPPORTED, "search_paths: a cost in the window has a component of 32767 or more");
            if (hst[b] == psearch::E_POINTS) return fail(h, ALORE_BE_E_UNSUPPORTED, "search_paths: more than 1024 raw nodes or 31 way-points");
        }
    }
    return ALORE_BE_OK;
}

int alore_backend_search_reserve(alore_backend_handle h, int max_cells, int slots)
{
    if (!h) return ALORE_BE_E_INVALID;
    const bool release = max_cells == 0;
    if (!release && (max_cells <= psearch::MAX_CELLS || max_cells > psearch::WIDE_MAX_CELLS || slots < 1 || slots > 1024 ||
                     (long long)slots * max_cells * (long long)sizeof(unsigned) > (1ll << 30)))
        return fail(h, ALORE_BE_E_INVALID, "search_reserve: max_cells in (32768, 1 << 22], slots in [1, 1024], slots * max_cells * 4 <= 1 GiB");
    BE_TRY(h, hipSetDevice(h->device));
    if (h->wide_pending) BE_TRY(h, hipEventSynchronize(h->ev_wide)); // the last search has left the slabs
    h->wide_pending = false;
    if (h->d_wide) BE_TRY(h, hipFree(h->d_wide));
    h->d_wide = nullptr;
    if (h->d_wide_ticks) BE_TRY(h, hipFree(h->d_wide_ticks));
    h->d_wide_ticks = nullptr;
    h->wide_cells = h->wide_slots = 0;
    if (release) return ALORE_BE_OK;
    if (!h->ev_wide) BE_TRY(h, hipEventCreateWithFlags(&h->ev_wide, hipEventDisableTiming));
    BE_TRY(h, dalloc(&h->d_wide_ticks, (size_t)h->B * 2));
    BE_TRY(h, hipMalloc((void**)&h->d_wide, sizeof(unsigned) * (size_t)slots * (size_t)max_cells));
    h->wide_cells = max_cells;
    h->wide_slots = slots;
    return ALORE_BE_OK;
}

int alore_backend_search_reserved(alore_backend_handle h, int* max_cells, int* slots)
{
    if (!h || !max_cells || !slots) return fail(h, ALORE_BE_E_INVALID, "search_reserved: bad argument");
    *max_cells = h->wide_cells;
    *slots = h->wide_slots;
    return ALORE_BE_OK;
}

int alore_backend_search_wide_ticks(alore_backend_handle h, int count, long long* out)
{
    if (!h || count < 1 || count > h->B || !out) return fail(h, ALORE_BE_E_INVALID, "search_wide_ticks: bad argument");
    if (!h->d_wide_ticks) return fail(h, ALORE_BE_E_INVALID, "search_wide_ticks: no reservation (alore_backend_search_reserve)");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize());
    BE_TRY(h, hipMemcpy(out, h->d_wide_ticks, sizeof(long long) * 2 * (size_t)count, hipMemcpyDeviceToHost));
    return ALORE_BE_OK;
}

int alore_backend_device_paths(alore_backend_handle h, alore_backend_paths* out)
{
    if (!h || !out) return fail(h, ALORE_BE_E_INVALID, "device_paths: bad argument");
    *out = alore_backend_paths{psearch::MAX_POINTS, h->d_path_n, h->d_path_xy, nullptr, nullptr, nullptr, nullptr};
    return ALORE_BE_OK;
}

int alore_backend_device_search_status(alore_backend_handle h, const int** out)
{
    if (!h || !out) return fail(h, ALORE_BE_E_INVALID, "device_search_status: bad argument");
    *out = h->d_search_status;
    return ALORE_BE_OK;
}

int alore_backend_search_status(alore_backend_handle h, int count, int* out)
{
    if (!h || count < 1 || count > h->B || !out) return fail(h, ALORE_BE_E_INVALID, "search_status: bad argument");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize());
    BE_TRY(h, hipMemcpy(out, h->d_search_status, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost));
    return ALORE_BE_OK;
}

int alore_backend_search_sweeps(alore_backend_handle h, int count, int* out)
{
    if (!h || count < 1 || count > h->B || !out) return fail(h, ALORE_BE_E_INVALID, "search_sweeps: bad argument");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize());
    BE_TRY(h, hipMemcpy(out, h->d_search_sweeps, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost));
    return ALORE_BE_OK;
}

int alore_backend_get_paths(alore_backend_handle h, int count, int* n_points, double* xy, int* cost_ab)
{
    if (!h || count < 1 || count > h->B) return fail(h, ALORE_BE_E_INVALID, "get_paths: bad argument");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize());
    const size_t n = count;
    if (n_points) BE_TRY(h, hipMemcpy(n_points, h->d_path_n, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (xy) BE_TRY(h, hipMemcpy(xy, h->d_path_xy, sizeof(double) * n * psearch::MAX_POINTS * 2, hipMemcpyDeviceToHost));
    if (cost_ab) BE_TRY(h, hipMemcpy(cost_ab, h->d_path_cost, sizeof(int) * n * 2, hipMemcpyDeviceToHost));
    return ALORE_BE_OK;
}

void alore_backend_task_default_params(alore_backend_task_params* p)
{
    tplan::Params d;
    tplan::default_params(&d);
    p->safe_dis = d.safe_dis;
    p->window_margin = d.window_margin;
    p->mode = d.mode;
}

int alore_backend_task_plan(alore_backend_handle h, int count, int max_tasks, const int* n_tasks, const double* points,
                            int point_row_stride_bytes, const int* assignment_or_null, const alore_backend_task_params* params,
                            int device_pointers, const int* mask, int mask_stride_bytes, void* stream)
{
    if (!h || count < 1 || count > h->B || !n_tasks || !points) return fail(h, ALORE_BE_E_INVALID, "task_plan: bad argument");
    if (max_tasks < 1 || max_tasks > tplan::MAX_TASKS) return fail(h, ALORE_BE_E_INVALID, "task_plan: max_tasks must be 1 .. 10");
    const int row = 2 * (int)sizeof(double) * (1 + 2 * max_tasks);
    if (point_row_stride_bytes < row || point_row_stride_bytes % (int)sizeof(double))
        return fail(h, ALORE_BE_E_INVALID, "task_plan: the row stride of the points must be a multiple of 8, at least 16 (1 + 2 max_tasks)");
    if (mask && (mask_stride_bytes < (int)sizeof(int) || mask_stride_bytes % (int)sizeof(int)))
        return fail(h, ALORE_BE_E_INVALID, "task_plan: the mask stride must be a positive multiple of sizeof(int)");
    alore_backend_task_params prm;
    if (params) prm = *params; else alore_backend_task_default_params(&prm);
    if (!std::isfinite(prm.safe_dis) || !std::isfinite(prm.window_margin) || prm.window_margin < 0.0)
        return fail(h, ALORE_BE_E_INVALID, "task_plan: safe_dis must be finite, window_margin finite and not negative");
    if (prm.mode < tplan::GREEDY || prm.mode > tplan::JOINT) return fail(h, ALORE_BE_E_INVALID, "task_plan: unknown mode");
    if (prm.mode != tplan::OPTIMAL) assignment_or_null = nullptr; // read in the optimal mode only
    if (!h->d_map) return fail(h, ALORE_BE_E_INVALID, "task_plan: no map (alore_backend_set_map / alore_backend_build_esdf / alore_backend_map_create)");
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->task_pending) BE_TRY(h, hipEventSynchronize(h->ev_task)); // the pinned block is free again
    h->task_pending = false;
    const size_t n = count, T = max_tasks;
    backend::TaskArgs g{};
    g.count = count;
    g.max_tasks = tplan::task_limit(prm.mode, max_tasks); // the rows of the caller keep their stride; an assignment is not read then
    g.mode = prm.mode;
    g.map = h->map;
    g.safe_dis = prm.safe_dis;
    g.window_margin = prm.window_margin;
    size_t up = TASK_ARGS_BYTES;
    if (device_pointers) {
        g.n_tasks = n_tasks;
        g.points = points; g.point_row_stride = point_row_stride_bytes;
        g.assign = assignment_or_null;
        g.mask = mask; g.mask_stride = mask ? mask_stride_bytes : 0;
    } else {
        double* hp = (double*)(h->h_task + TASK_ARGS_BYTES);
        int *hn = (int*)(hp + 2 * (1 + 2 * T) * n), *ha = hn + n, *hm = ha + n * T;
        for (size_t b = 0; b < n; ++b) {
            std::memcpy(hp + 2 * (1 + 2 * T) * b, (const char*)points + b * (size_t)point_row_stride_bytes, (size_t)row);
            hn[b] = n_tasks[b];
            for (size_t i = 0; i < T; ++i) ha[b * T + i] = assignment_or_null ? assignment_or_null[b * T + i] : (int)i;
            hm[b] = mask ? *(const int*)((const char*)mask + b * (size_t)mask_stride_bytes) : 1;
        }
        const double* dp = (const double*)(h->d_task_in + TASK_ARGS_BYTES);
        const int* dn = (const int*)(dp + 2 * (1 + 2 * T) * n);
        g.points = dp; g.point_row_stride = row;
        g.n_tasks = dn;
        g.assign = assignment_or_null ? dn + n : nullptr;
        g.mask = mask ? dn + n + n * T : nullptr;
        g.mask_stride = mask ? (int)sizeof(int) : 0;
        up = task_in_bytes(n, T);
    }
    const long long map_cells = (long long)h->map.nx * h->map.ny;
    g.lds_cells = map_cells < psearch::MAX_CELLS ? (int)map_cells : psearch::MAX_CELLS;
    g.status = h->t_status; g.matrix = h->t_matrix; g.order = h->t_order; g.n_order = h->t_n_order; g.total = h->t_total;
    g.leg_start_xy = h->t_leg_start; g.leg_goal_xy = h->t_leg_goal; g.fields = h->t_fields; g.sweeps = h->t_sweeps;
    g.src_fields = h->t_src_fields; g.src_sweeps = h->t_src_sweeps;
    g.assignment = h->t_assignment; g.assign_total = h->t_assign_total;
    g.wide_slabs = h->d_task_wide; g.wide_cells = h->task_cells; g.wide_slots = h->task_slots; g.src_range = h->t_src_range; g.src_ticks = h->d_task_ticks;
    std::memcpy(h->h_task, &g, sizeof(g));
    BE_TRY(h, hipMemcpyAsync(h->d_task_in, h->h_task, up, hipMemcpyHostToDevice, s));
    BE_TRY(h, hipEventRecord(h->ev_task, s));
    h->task_pending = true;
    BE_TRY(h, backend::task_plan((const backend::TaskArgs*)h->d_task_in, count, g.max_tasks, prm.mode, g.lds_cells, h->task_slots, s));
    h->task_last_count = count;
    h->task_last_mode = prm.mode;
    if (h->d_task_wide) {
        BE_TRY(h, hipEventRecord(h->ev_task_wide, s));
        h->task_wide_pending = true;
    }
    if (!device_pointers) {
        int* hst = (int*)h->h_stage;
        BE_TRY(h, hipMemcpyAsync(hst, h->t_status, sizeof(int) * n, hipMemcpyDeviceToHost, s));
        BE_TRY(h, hipStreamSynchronize(s));
        for (size_t b = 0; b < n; ++b) {
            if (hst[b] == tplan::E_TASKS) return fail(h, ALORE_BE_E_INVALID, "task_plan: mission failed: a task count is outside 1..max_tasks (joint mode: 1..5), or an assignment is no permutation");
            if (hst[b] == tplan::E_ENDPOINT) return fail(h, ALORE_BE_E_INVALID, "task_plan: mission failed: a point is not finite or outside the map");
            if (hst[b] == tplan::E_NO_ORDER) return fail(h, ALORE_BE_E_INVALID, "task_plan: mission failed: no order has a finite cost");
            if (hst[b] == tplan::E_WINDOW)
                return fail(h, ALORE_BE_E_UNSUPPORTED, "task_plan: mission failed: the window has more than 32768 cells, or more than the reservation");
            if (hst[b] == tplan::E_RANGE)
                return fail(h, ALORE_BE_E_UNSUPPORTED, "task_plan: mission failed: a cost in the window has a component of 32767 or more");
        }
    }
    return ALORE_BE_OK;
}

int alore_backend_task_reorder(alore_backend_handle h, void* stream)
{
    if (!h || h->task_last_count < 1) return fail(h, ALORE_BE_E_INVALID, "task_reorder: no alore_backend_task_plan launch on this handle");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, backend::task_order((const backend::TaskArgs*)h->d_task_in, h->task_last_count, h->task_last_mode, (hipStream_t)stream));
    return ALORE_BE_OK;
}

int alore_backend_task_reserve(alore_backend_handle h, int max_cells, int slots)
{
    if (!h) return ALORE_BE_E_INVALID;
    const bool release = max_cells == 0;
    if (!release && (max_cells <= psearch::MAX_CELLS || max_cells > psearch::WIDE_MAX_CELLS || slots < 1 || slots > 1024 ||
                     (long long)slots * max_cells * (long long)sizeof(unsigned) > (1ll << 30)))
        return fail(h, ALORE_BE_E_INVALID, "task_reserve: max_cells in (32768, 1 << 22], slots in [1, 1024], slots * max_cells * 4 <= 1 GiB");
    BE_TRY(h, hipSetDevice(h->device));
    if (h->task_wide_pending) BE_TRY(h, hipEventSynchronize(h->ev_task_wide)); // the last task launch has left the slabs
    h->task_wide_pending = false;
    if (h->d_task_wide) BE_TRY(h, hipFree(h->d_task_wide));
    h->d_task_wide = nullptr;
    if (h->d_task_ticks) BE_TRY(h, hipFree(h->d_task_ticks));
    h->d_task_ticks = nullptr;
    h->task_cells = h->task_slots = 0;
    if (release) return ALORE_BE_OK;
    if (!h->ev_task_wide) BE_TRY(h, hipEventCreateWithFlags(&h->ev_task_wide, hipEventDisableTiming));
    BE_TRY(h, dalloc(&h->d_task_ticks, (size_t)h->B * tplan::MAX_LEGS));
    BE_TRY(h, hipMalloc((void**)&h->d_task_wide, sizeof(unsigned) * (size_t)slots * (size_t)max_cells));
    h->task_cells = max_cells;
    h->task_slots = slots;
    return ALORE_BE_OK;
}

int alore_backend_task_wide_ticks(alore_backend_handle h, int count, long long* out)
{
    if (!h || count < 1 || count > h->B || !out) return fail(h, ALORE_BE_E_INVALID, "task_wide_ticks: bad argument");
    if (!h->d_task_ticks) return fail(h, ALORE_BE_E_INVALID, "task_wide_ticks: no reservation (alore_backend_task_reserve)");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize());
    BE_TRY(h, hipMemcpy(out, h->d_task_ticks, sizeof(long long) * tplan::MAX_LEGS * (size_t)count, hipMemcpyDeviceToHost));
    return ALORE_BE_OK;
}

int alore_backend_task_reserved(alore_backend_handle h, int* max_cells, int* slots)
{
    if (!h || !max_cells || !slots) return fail(h, ALORE_BE_E_INVALID, "task_reserved: bad argument");
    *max_cells = h->task_cells;
    *slots = h->task_slots;
    return ALORE_BE_OK;
}

int alore_backend_device_task(alore_backend_handle h, alore_backend_task_view* out)
{
    if (!h || !out) return fail(h, ALORE_BE_E_INVALID, "device_task: bad argument");
    *out = alore_backend_task_view{tplan::P_MAX, tplan::MAX_LEGS, h->t_status, h->t_matrix, h->t_order, h->t_n_order, h->t_total,
                                   h->t_leg_start, h->t_leg_goal, h->t_fields, h->t_sweeps};
    return ALORE_BE_OK;
}

int alore_backend_get_task(alore_backend_handle h, int count, int* status, int* matrix, int* order, int* n_order, int* total,
                           double* leg_start_xy, double* leg_goal_xy, int* fields, int* sweeps)
{
    if (!h || count < 1 || count > h->B) return fail(h, ALORE_BE_E_INVALID, "get_task: bad argument");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize());
    const size_t n = count, L = tplan::MAX_LEGS;
    if (status) BE_TRY(h, hipMemcpy(status, h->t_status, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (matrix) BE_TRY(h, hipMemcpy(matrix, h->t_matrix, sizeof(int) * n * TASK_MATRIX_INTS, hipMemcpyDeviceToHost));
    if (order) BE_TRY(h, hipMemcpy(order, h->t_order, sizeof(int) * n * L, hipMemcpyDeviceToHost));
    if (n_order) BE_TRY(h, hipMemcpy(n_order, h->t_n_order, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (total) BE_TRY(h, hipMemcpy(total, h->t_total, sizeof(int) * n * 2, hipMemcpyDeviceToHost));
    if (leg_start_xy) BE_TRY(h, hipMemcpy(leg_start_xy, h->t_leg_start, sizeof(double) * n * L * 2, hipMemcpyDeviceToHost));
    if (leg_goal_xy) BE_TRY(h, hipMemcpy(leg_goal_xy, h->t_leg_goal, sizeof(double) * n * L * 2, hipMemcpyDeviceToHost));
    if (fields) BE_TRY(h, hipMemcpy(fields, h->t_fields, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (sweeps) BE_TRY(h, hipMemcpy(sweeps, h->t_sweeps, sizeof(int) * n, hipMemcpyDeviceToHost));
    return ALORE_BE_OK;
}

static_assert(ALORE_BE_TASK_ASSIGNED == tplan::ASSIGNED && ALORE_BE_TASK_JOINT == tplan::JOINT &&
              ALORE_BE_TASK_JOINT_MAX_TASKS == tplan::JOINT_MAX_TASKS && ALORE_BE_TASK_MAX_TASKS == tplan::MAX_TASKS, "task_plan.h");

int alore_backend_device_task_assign(alore_backend_handle h, alore_backend_task_assign_view* out)
{
    if (!h || !out) return fail(h, ALORE_BE_E_INVALID, "device_task_assign: bad argument");
    *out = alore_backend_task_assign_view{h->t_assignment, h->t_assign_total};
    return ALORE_BE_OK;
}

int alore_backend_get_task_assign(alore_backend_handle h, int count, int* assignment, int* assign_total)
{
    if (!h || count < 1 || count > h->B) return fail(h, ALORE_BE_E_INVALID, "get_task_assign: bad argument");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize());
    const size_t n = count;
    if (assignment) BE_TRY(h, hipMemcpy(assignment, h->t_assignment, sizeof(int) * n * tplan::MAX_TASKS, hipMemcpyDeviceToHost));
    if (assign_total) BE_TRY(h, hipMemcpy(assign_total, h->t_assign_total, sizeof(int) * n * 2, hipMemcpyDeviceToHost));
    return ALORE_BE_OK;
}

// ---- the edits of missions in the resident map ---------------------------------------------------------------------------------
static_assert(sizeof(alore_backend_map_edit) == sizeof(mission::Edit) && sizeof(alore_backend_map_edit) == 40, "alore_backend_map_edit");
static_assert(sizeof(alore_backend_mission_params) == sizeof(mission::Params), "alore_backend_mission_params");

// the descriptors and counters of the paint kernels; `need`: a list that must fit into one launch (a host list, the missions' list)
static int paint_buffers(alore_backend_handle h, int need)
{
    const int want = std::max(need, (int)mission::PAINT_CHUNK);
    if (want > h->p_desc_cap) {
        if (h->p_desc) {
            BE_TRY(h, hipDeviceSynchronize()); // an earlier call on another stream may still read the old descriptors
            (void)hipFree(h->p_desc);
            h->p_desc = nullptr;
            h->p_desc_cap = 0;
        }
        BE_TRY(h, hipMalloc((void**)&h->p_desc, sizeof(mission::Desc) * (size_t)want));
        h->p_desc_cap = want;
    }
    if (!h->p_counters) {
        BE_TRY(h, dalloc(&h->p_counters, 8));
        const mission::Counters c = mission::no_change(h->omap.nx, h->omap.ny);
        BE_TRY(h, hipMemcpy(h->p_counters, &c, sizeof(c), hipMemcpyHostToDevice));
    }
    return ALORE_BE_OK;
}
static occ::Geom paint_geom(alore_backend_handle h) { return occ::make_geom(h->omap.nx, h->omap.ny, h->omap.x_lo, h->omap.y_lo, h->omap.res); }

int alore_backend_map_paint(alore_backend_handle h, const alore_backend_map_edit* edits, int n_or_capacity, const int* d_count, int device_edits,
                            void* stream)
{
    BE_MAP(h, "map_paint");
    if (n_or_capacity < 0 || (n_or_capacity > 0 && !edits) || (device_edits && !d_count))
        return fail(h, ALORE_BE_E_INVALID, "map_paint: a list needs edits and a length that is not negative, a device list its device count");
    const mission::Edit* list = (const mission::Edit*)edits;
    if (!device_edits) {
        const long bad = mission::first_invalid(list, n_or_capacity, h->omap.res);
        if (bad >= 0)
            return fail(h, ALORE_BE_E_INVALID, "map_paint: an edit has a field that is not finite, a negative half size or more than 64 lattice points on an axis");
    }
    BE_TRY(h, hipSetDevice(h->device));
    if (const int rc = paint_buffers(h, device_edits ? 0 : n_or_capacity)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (!device_edits) {
        if ((size_t)n_or_capacity > h->p_host_cap) {
            BE_TRY(h, hipDeviceSynchronize()); // an earlier call on another stream may still read the old buffer
            if (h->p_host_edits) { (void)hipFree(h->p_host_edits); h->p_host_edits = nullptr; h->p_host_cap = 0; }
            BE_TRY(h, hipMalloc((void**)&h->p_host_edits, sizeof(mission::Edit) * (size_t)n_or_capacity));
            h->p_host_cap = (size_t)n_or_capacity;
        }
        if (n_or_capacity > 0)
            BE_TRY(h, hipMemcpyAsync(h->p_host_edits, edits, sizeof(mission::Edit) * (size_t)n_or_capacity, hipMemcpyHostToDevice, s));
        list = h->p_host_edits;
        d_count = nullptr;
    }
    BE_TRY(h, mission::paint_enqueue(paint_geom(h), h->omap.grid, list, d_count, n_or_capacity, h->p_desc, h->p_desc_cap, h->p_counters, s));
    if (!device_edits) BE_TRY(h, hipStreamSynchronize(s));
    return ALORE_BE_OK;
}

int alore_backend_device_paint_counters(alore_backend_handle h, const int** out)
{
    if (!h || !out) return fail(h, ALORE_BE_E_INVALID, "device_paint_counters: bad argument");
    if (!h->p_counters) return fail(h, ALORE_BE_E_INVALID, "device_paint_counters: nothing was painted yet (alore_backend_map_paint / alore_backend_mission_create)");
    *out = h->p_counters;
    return ALORE_BE_OK;
}

int alore_backend_map_paint_counters(alore_backend_handle h, int out[6])
{
    if (!h || !out) return fail(h, ALORE_BE_E_INVALID, "map_paint_counters: bad argument");
    if (!h->p_counters) return fail(h, ALORE_BE_E_INVALID, "map_paint_counters: nothing was painted yet (alore_backend_map_paint / alore_backend_mission_create)");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize());
    BE_TRY(h, hipMemcpy(out, h->p_counters, sizeof(int) * 6, hipMemcpyDeviceToHost));
    return ALORE_BE_OK;
}

void alore_backend_mission_default_params(alore_backend_mission_params* p)
{
    mission::Params d;
    mission::default_params(&d);
    std::memcpy(p, &d, sizeof(d));
}

namespace {
// the staging of the host routes of alore_backend_mission_*: rows of points, then n_tasks, kinds and a mask
size_t mission_stage_bytes(size_t B) { return B * (sizeof(double) * 2 * ALORE_BE_TASK_MAX_POINTS + sizeof(int) * (ALORE_BE_TASK_MAX_TASKS + 2)); }
bool stride_ok(int stride, int least, int unit) { return stride >= least && stride % unit == 0; }
} // namespace

int alore_backend_mission_create(alore_backend_handle h, const alore_backend_mission_params* params)
{
    BE_MAP(h, "mission_create");
    mission::Params prm;
    if (params) std::memcpy(&prm, params, sizeof(prm)); else mission::default_params(&prm);
    const double v[7] = {prm.item_half, prm.free_half, prm.item_free_dist, prm.target_lock_half, prm.target_lock_dist, prm.left_target_half, prm.left_target_dist};
    for (double x : v)
        if (!std::isfinite(x) || x < 0.0) return fail(h, ALORE_BE_E_INVALID, "mission_create: half sizes and distances must be finite and not negative");
    BE_TRY(h, hipSetDevice(h->device));
    if (const int rc = paint_buffers(h, h->B * mission::MAX_TASKS)) return rc;
    h->m_params = prm;
    if (h->has_mission) return ALORE_BE_OK; // the slab is sized by the handle, not by the parameters
    const size_t B = h->B, T = mission::MAX_TASKS;
    const size_t doubles = B * T * 4, ints = B * 7 + 2 + B * T;
    std::vector<char> init(sizeof(double) * doubles + sizeof(int) * ints, 0);
    int* hi = (int*)(init.data() + sizeof(double) * doubles);
    for (size_t b = 0; b < B; ++b) {
        hi[b] = mission::MASKED; // never set
        hi[2 * B + b] = hi[3 * B + b] = -1;
    }
    hipError_t e = hipMalloc((void**)&h->m_slab_mem, init.size());
    if (e == hipSuccess) e = hipMemcpy(h->m_slab_mem, init.data(), init.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&h->m_edits, sizeof(mission::Edit) * B * T);
    if (e == hipSuccess) e = hipMalloc((void**)&h->m_stage, mission_stage_bytes(B));
    if (e != hipSuccess) {
        void* ptrs[] = {h->m_slab_mem, h->m_edits, h->m_stage};
        for (void* p : ptrs)
            if (p) (void)hipFree(p);
        h->m_slab_mem = h->m_stage = nullptr;
        h->m_edits = nullptr;
        return fail(h, e == hipErrorOutOfMemory ? ALORE_BE_E_NOMEM : ALORE_BE_E_HIP, "mission_create", e);
    }
    double* dd = (double*)h->m_slab_mem;
    int* di = (int*)(dd + doubles);
    h->m_slab = mission::Slab{di, di + B, di + 2 * B, di + 3 * B, di + 4 * B, di + 5 * B, di + 7 * B + 2, dd, dd + B * T * 2};
    h->m_was_set = di + 6 * B;
    h->m_n_edits = di + 7 * B;
    h->has_mission = true;
    return ALORE_BE_OK;
}

#define BE_MISSION(h, what)                                                                                       \
    do {                                                                                                          \
        BE_MAP(h, what);                                                                                          \
        if (!h->has_mission) return fail(h, ALORE_BE_E_INVALID, what ": no missions (alore_backend_mission_create)"); \
    } while (0)

int alore_backend_mission_set(alore_backend_handle h, int count, int max_tasks, const int* n_tasks, const double* points,
                              int point_row_stride_bytes, const int* kinds_or_null, int device_pointers, const int* mask,
                              int mask_stride_bytes, void* stream)
{
    BE_MISSION(h, "mission_set");
    if (count < 1 || count > h->B || !n_tasks || !points) return fail(h, ALORE_BE_E_INVALID, "mission_set: bad argument");
    if (max_tasks < 1 || max_tasks > mission::MAX_TASKS) return fail(h, ALORE_BE_E_INVALID, "mission_set: max_tasks must be 1 .. 10");
    const int row = 2 * (int)sizeof(double) * (1 + 2 * max_tasks);
    if (!stride_ok(point_row_stride_bytes, row, 8))
        return fail(h, ALORE_BE_E_INVALID, "mission_set: the row stride of the points must be a multiple of 8, at least 16 (1 + 2 max_tasks)");
    if (mask && !stride_ok(mask_stride_bytes, 4, 4)) return fail(h, ALORE_BE_E_INVALID, "mission_set: the mask stride must be a positive multiple of sizeof(int)");
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n = count, T = max_tasks;
    std::vector<char> pack;
    if (!device_pointers) {
        pack.resize((size_t)row * n + sizeof(int) * (n + n * T + n));
        int *hn = (int*)(pack.data() + (size_t)row * n), *hk = hn + n, *hm = hk + n * T;
        for (size_t b = 0; b < n; ++b) {
            std::memcpy(pack.data() + (size_t)row * b, (const char*)points + b * (size_t)point_row_stride_bytes, (size_t)row);
            hn[b] = n_tasks[b];
            for (size_t i = 0; i < T; ++i) hk[b * T + i] = kinds_or_null ? kinds_or_null[b * T + i] : mission::KIND_SQUARE;
            hm[b] = mask ? *(const int*)((const char*)mask + b * (size_t)mask_stride_bytes) : 1;
        }
        BE_TRY(h, hipMemcpyAsync(h->m_stage, pack.data(), pack.size(), hipMemcpyHostToDevice, s));
        points = (const double*)h->m_stage;
        point_row_stride_bytes = row;
        n_tasks = (const int*)(h->m_stage + (size_t)row * n);
        kinds_or_null = n_tasks + n;
        mask = kinds_or_null + n * T;
        mask_stride_bytes = (int)sizeof(int);
    }
    BE_TRY(h, mission::set_enqueue(h->m_slab, count, max_tasks, n_tasks, points, point_row_stride_bytes, kinds_or_null, mask, mask ? mask_stride_bytes : 0,
                                   h->m_was_set, s));
    BE_TRY(h, mission::edits_enqueue(h->m_slab, h->m_params, count, h->m_was_set, nullptr, 0, nullptr, 0, h->m_edits, h->m_n_edits, s));
    BE_TRY(h, mission::paint_enqueue(paint_geom(h), h->omap.grid, h->m_edits, h->m_n_edits, count * mission::MAX_TASKS, h->p_desc, h->p_desc_cap, h->p_counters, s));
    if (!device_pointers) BE_TRY(h, hipStreamSynchronize(s));
    return ALORE_BE_OK;
}

int alore_backend_mission_set_goals(alore_backend_handle h, int count, const double* goal_xy, int goal_stride_bytes, int device_pointers,
                                    const int* mask, int mask_stride_bytes, void* stream)
{
    BE_MISSION(h, "mission_set_goals");
    if (count < 1 || count > h->B || !goal_xy || !stride_ok(goal_stride_bytes, 16, 8))
        return fail(h, ALORE_BE_E_INVALID, "mission_set_goals: needs 1 .. max_problems goals with a stride that is a multiple of 8, at least 16");
    if (mask && !stride_ok(mask_stride_bytes, 4, 4)) return fail(h, ALORE_BE_E_INVALID, "mission_set_goals: the mask stride must be a positive multiple of sizeof(int)");
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n = count;
    std::vector<char> pack;
    if (!device_pointers) {
        pack.resize(16 * n + sizeof(int) * n);
        int* hm = (int*)(pack.data() + 16 * n);
        for (size_t b = 0; b < n; ++b) {
            std::memcpy(pack.data() + 16 * b, (const char*)goal_xy + b * (size_t)goal_stride_bytes, 16);
            hm[b] = mask ? *(const int*)((const char*)mask + b * (size_t)mask_stride_bytes) : 1;
        }
        BE_TRY(h, hipMemcpyAsync(h->m_stage, pack.data(), pack.size(), hipMemcpyHostToDevice, s));
        goal_xy = (const double*)h->m_stage;
        goal_stride_bytes = 16;
        mask = (const int*)(h->m_stage + 16 * n);
        mask_stride_bytes = (int)sizeof(int);
    }
    BE_TRY(h, mission::goals_enqueue(h->m_slab, count, goal_xy, goal_stride_bytes, mask, mask ? mask_stride_bytes : 0, s));
    if (!device_pointers) BE_TRY(h, hipStreamSynchronize(s));
    return ALORE_BE_OK;
}

int alore_backend_mission_step(alore_backend_handle h, int count, const double* poses, int pose_stride_bytes, int device_pointers,
                               const int* after_plan_mask, int mask_stride_bytes, void* stream)
{
    BE_MISSION(h, "mission_step");
    if (count < 1 || count > h->B || !poses || !stride_ok(pose_stride_bytes, 16, 8))
        return fail(h, ALORE_BE_E_INVALID, "mission_step: needs 1 .. max_problems poses with a stride that is a multiple of 8, at least 16");
    if (after_plan_mask && !stride_ok(mask_stride_bytes, 4, 4))
        return fail(h, ALORE_BE_E_INVALID, "mission_step: the mask stride must be a positive multiple of sizeof(int)");
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n = count;
    std::vector<char> pack;
    if (!device_pointers) {
        pack.resize(16 * n + sizeof(int) * n);
        int* hm = (int*)(pack.data() + 16 * n);
        for (size_t b = 0; b < n; ++b) {
            std::memcpy(pack.data() + 16 * b, (const char*)poses + b * (size_t)pose_stride_bytes, 16);
            hm[b] = after_plan_mask ? *(const int*)((const char*)after_plan_mask + b * (size_t)mask_stride_bytes) : 0;
        }
        BE_TRY(h, hipMemcpyAsync(h->m_stage, pack.data(), pack.size(), hipMemcpyHostToDevice, s));
        poses = (const double*)h->m_stage;
        pose_stride_bytes = 16;
        after_plan_mask = (const int*)(h->m_stage + 16 * n);
        mask_stride_bytes = (int)sizeof(int);
    }
    BE_TRY(h, mission::edits_enqueue(h->m_slab, h->m_params, count, h->m_was_set, poses, pose_stride_bytes, after_plan_mask,
                                     after_plan_mask ? mask_stride_bytes : 0, h->m_edits, h->m_n_edits, s));
    BE_TRY(h, mission::paint_enqueue(paint_geom(h), h->omap.grid, h->m_edits, h->m_n_edits, 2 * count, h->p_desc, h->p_desc_cap, h->p_counters, s));
    if (!device_pointers) BE_TRY(h, hipStreamSynchronize(s));
    return ALORE_BE_OK;
}

int alore_backend_device_mission(alore_backend_handle h, alore_backend_mission_view* out)
{
    if (!h || !out) return fail(h, ALORE_BE_E_INVALID, "device_mission: bad argument");
    if (!h->has_mission) return fail(h, ALORE_BE_E_INVALID, "device_mission: no missions (alore_backend_mission_create)");
    const mission::Slab& s = h->m_slab;
    *out = alore_backend_mission_view{mission::MAX_TASKS, h->B * mission::MAX_TASKS, s.status, s.phase, s.goal_item, s.goal_target, s.goal_status,
                                      s.n, s.kinds, s.items, s.targets, (const alore_backend_map_edit*)h->m_edits, h->m_n_edits, h->p_counters};
    return ALORE_BE_OK;
}

int alore_backend_get_mission(alore_backend_handle h, int count, int* status, int* phase, int* goal_item, int* goal_target, int* goal_status,
                              alore_backend_map_edit* edits, int* n_edits, int counters[6])
{
    if (!h || count < 1 || count > h->B) return fail(h, ALORE_BE_E_INVALID, "get_mission: bad argument");
    if (!h->has_mission) return fail(h, ALORE_BE_E_INVALID, "get_mission: no missions (alore_backend_mission_create)");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize());
    const size_t n = count;
    const mission::Slab& s = h->m_slab;
    if (status) BE_TRY(h, hipMemcpy(status, s.status, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (phase) BE_TRY(h, hipMemcpy(phase, s.phase, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (goal_item) BE_TRY(h, hipMemcpy(goal_item, s.goal_item, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (goal_target) BE_TRY(h, hipMemcpy(goal_target, s.goal_target, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (goal_status) BE_TRY(h, hipMemcpy(goal_status, s.goal_status, sizeof(int) * n, hipMemcpyDeviceToHost));
    int ne = 0;
    BE_TRY(h, hipMemcpy(&ne, h->m_n_edits, sizeof(int), hipMemcpyDeviceToHost));
    if (n_edits) *n_edits = ne;
    if (edits && ne > 0) BE_TRY(h, hipMemcpy(edits, h->m_edits, sizeof(mission::Edit) * (size_t)ne, hipMemcpyDeviceToHost));
    if (counters) BE_TRY(h, hipMemcpy(counters, h->p_counters, sizeof(int) * 6, hipMemcpyDeviceToHost));
    return ALORE_BE_OK;
}

// ---- plan_manager's state machine for the fleet -----------------------------------------------------------------------------------
static_assert(sizeof(alore_backend_manager_params) == sizeof(fleet::Params) && sizeof(alore_backend_manager_params) == 32, "alore_backend_manager_params");
static_assert(ALORE_BE_TASK_MAX_LEGS == fleet::MAX_LEGS && ALORE_BE_SEARCH_OK == fleet::SEARCH_OK && ALORE_BE_BUILD_OK == fleet::BUILD_OK, "fleet_manager.h");

void alore_backend_manager_default_params(alore_backend_manager_params* p)
{
    fleet::Params d;
    fleet::default_params(&d);
    std::memcpy(p, &d, sizeof(d));
}

namespace {
// the staging of the host routes of alore_backend_manager_*: starts and goals [n][3] and a mask, or poses [n][2] and a mask
size_t manager_stage_bytes(size_t B) { return B * (sizeof(double) * 6 + sizeof(int)); }
} // namespace

int alore_backend_manager_create(alore_backend_handle h, const alore_backend_manager_params* params)
{
    if (!h) return ALORE_BE_E_INVALID;
    fleet::Params prm;
    if (params) std::memcpy(&prm, params, sizeof(prm)); else fleet::default_params(&prm);
    if (!std::isfinite(prm.replan_time) || !std::isfinite(prm.max_replan_time) || prm.max_replan_time < 0.0)
        return fail(h, ALORE_BE_E_INVALID, "manager_create: the times must be finite and max_replan_time not negative");
    BE_TRY(h, hipSetDevice(h->device));
    if (h->has_manager) { // the slab is sized by the handle, not by the parameters
        h->g_params = prm;
        return ALORE_BE_OK;
    }
    const size_t B = h->B, doubles = B * fleet::SLAB_DOUBLE_ROWS, ints = B * fleet::SLAB_INT_ROWS + fleet::N_COUNTERS;
    std::vector<char> init(sizeof(double) * doubles + sizeof(int) * ints, 0);
    double* hd = (double*)init.data();
    int* hi = (int*)(init.data() + sizeof(double) * doubles);
    const fleet::Robot r0 = fleet::initial();
    for (size_t b = 0; b < B; ++b) {
        hi[b] = r0.state;
        hi[5 * B + b] = r0.returned;
        hd[10 * B + b] = r0.plan_start_time;
        hd[13 * B + b] = r0.time;
    }
    hipError_t e = hipMalloc((void**)&h->g_mem, init.size());
    if (e == hipSuccess) e = hipMemcpy(h->g_mem, init.data(), init.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&h->g_stage, manager_stage_bytes(B));
    if (e != hipSuccess) {
        if (h->g_mem) (void)hipFree(h->g_mem);
        if (h->g_stage) (void)hipFree(h->g_stage);
        h->g_mem = h->g_stage = nullptr;
        return fail(h, e == hipErrorOutOfMemory ? ALORE_BE_E_NOMEM : ALORE_BE_E_HIP, "manager_create", e);
    }
    double* dd = (double*)h->g_mem;
    int* di = (int*)(dd + doubles);
    fleet::Slab& s = h->g_slab;
    s.B = h->B;
    s.state = di; s.have_goal = di + B; s.have_start = di + 2 * B; s.leg = di + 3 * B; s.action = di + 4 * B; s.returned = di + 5 * B;
    s.plan_mask = di + 6 * B; s.fresh_mask = di + 7 * B; s.replan_mask = di + 8 * B; s.stop_mask = di + 9 * B; s.after_plan_mask = di + 10 * B;
    s.counters = di + 11 * B;
    s.goal = dd; s.start = dd + 3 * B; s.plan_start_xytheta = dd + 6 * B;
    s.loop_start_time = dd + 9 * B; s.plan_start_time = dd + 10 * B; s.traj_start_time = dd + 11 * B; s.traj_total_time = dd + 12 * B;
    s.time = dd + 13 * B;
    h->g_params = prm;
    h->g_begun = false;
    h->has_manager = true;
    return ALORE_BE_OK;
}

#define BE_MANAGER(h, what)                                                                                        \
    do {                                                                                                           \
        if (!h) return ALORE_BE_E_INVALID;                                                                         \
        if (!h->has_manager) return fail(h, ALORE_BE_E_INVALID, what ": no manager (alore_backend_manager_create)"); \
    } while (0)

int alore_backend_manager_request(alore_backend_handle h, int count, const double* start_xytheta, const double* goal_xytheta, int stride_bytes,
                                  int device_pointers, const int* mask, int mask_stride_bytes, void* stream)
{
    BE_MANAGER(h, "manager_request");
    if (count < 1 || count > h->B || (!start_xytheta && !goal_xytheta) || !stride_ok(stride_bytes, 24, 8))
        return fail(h, ALORE_BE_E_INVALID, "manager_request: needs 1 .. max_problems robots, a start or a goal, and a stride that is a multiple of 8, at least 24");
    if (mask && !stride_ok(mask_stride_bytes, 4, 4)) return fail(h, ALORE_BE_E_INVALID, "manager_request: the mask stride must be a positive multiple of sizeof(int)");
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n = count;
    std::vector<char> pack;
    if (!device_pointers) {
        pack.resize(48 * n + sizeof(int) * n, 0);
        int* hm = (int*)(pack.data() + 48 * n);
        for (size_t b = 0; b < n; ++b) {
            if (start_xytheta) std::memcpy(pack.data() + 24 * b, (const char*)start_xytheta + b * (size_t)stride_bytes, 24);
            if (goal_xytheta) std::memcpy(pack.data() + 24 * (n + b), (const char*)goal_xytheta + b * (size_t)stride_bytes, 24);
            hm[b] = mask ? *(const int*)((const char*)mask + b * (size_t)mask_stride_bytes) : 1;
        }
        BE_TRY(h, hipMemcpyAsync(h->g_stage, pack.data(), pack.size(), hipMemcpyHostToDevice, s));
        if (start_xytheta) start_xytheta = (const double*)h->g_stage;
        if (goal_xytheta) goal_xytheta = (const double*)(h->g_stage + 24 * n);
        stride_bytes = 24;
        mask = (const int*)(h->g_stage + 48 * n);
        mask_stride_bytes = (int)sizeof(int);
    }
    BE_TRY(h, fleet::request_enqueue(h->g_slab, count, start_xytheta, goal_xytheta, stride_bytes, mask, mask ? mask_stride_bytes : 0, s));
    if (!device_pointers) BE_TRY(h, hipStreamSynchronize(s));
    return ALORE_BE_OK;
}

int alore_backend_manager_begin(alore_backend_handle h, int count, double now, const double* poses, int pose_stride_bytes,
                                const int* collision_mask_or_null, int mask_stride_bytes, int device_pointers, void* stream)
{
    BE_MANAGER(h, "manager_begin");
    if (count < 1 || count > h->B || !poses || !stride_ok(pose_stride_bytes, 16, 8) || !std::isfinite(now))
        return fail(h, ALORE_BE_E_INVALID, "manager_begin: needs 1 .. max_problems poses with a stride that is a multiple of 8, at least 16, and a finite time");
    if (collision_mask_or_null && !stride_ok(mask_stride_bytes, 4, 4))
        return fail(h, ALORE_BE_E_INVALID, "manager_begin: the mask stride must be a positive multiple of sizeof(int)");
    BE_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n = count;
    std::vector<char> pack;
    if (!device_pointers) {
        pack.resize(16 * n + sizeof(int) * n);
        int* hm = (int*)(pack.data() + 16 * n);
        for (size_t b = 0; b < n; ++b) {
            std::memcpy(pack.data() + 16 * b, (const char*)poses + b * (size_t)pose_stride_bytes, 16);
            hm[b] = collision_mask_or_null ? *(const int*)((const char*)collision_mask_or_null + b * (size_t)mask_stride_bytes) : 0;
        }
        BE_TRY(h, hipMemcpyAsync(h->g_stage, pack.data(), pack.size(), hipMemcpyHostToDevice, s));
        poses = (const double*)h->g_stage;
        pose_stride_bytes = 16;
        collision_mask_or_null = (const int*)(h->g_stage + 16 * n);
        mask_stride_bytes = (int)sizeof(int);
    }
    const fleet::Map m{h->d_map ? h->map.dist : nullptr, h->map.nx, h->map.ny, h->map.x_lo, h->map.y_lo, h->map.x_hi, h->map.y_hi, h->map.res};
    BE_TRY(h, fleet::begin_enqueue(h->g_slab, h->g_params, m, count, now, poses, pose_stride_bytes, collision_mask_or_null,
                                   collision_mask_or_null ? mask_stride_bytes : 0, s));
    h->g_now = now;
    h->g_begun = true;
    if (!device_pointers) BE_TRY(h, hipStreamSynchronize(s));
    return ALORE_BE_OK;
}

int alore_backend_manager_starts(alore_backend_handle h, int count, double* d_xytheta, double* d_vaj, double* d_oaj, double* d_start_yaw,
                                 double* d_end_yaw, void* stream)
{
    BE_MANAGER(h, "manager_starts");
    if (count < 1 || count > h->B || !d_xytheta || !d_vaj || !d_oaj) return fail(h, ALORE_BE_E_INVALID, "manager_starts: bad argument");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, fleet::starts_enqueue(h->g_slab, count, d_xytheta, d_vaj, d_oaj, d_start_yaw, d_end_yaw, (hipStream_t)stream));
    return ALORE_BE_OK;
}

int alore_backend_manager_end(alore_backend_handle h, int count, const int* search_status, const int* build_status, const int* plan_ok,
                              const double* T, const int* n_pieces, void* stream)
{
    BE_MANAGER(h, "manager_end");
    if (count < 1 || count > h->B) return fail(h, ALORE_BE_E_INVALID, "manager_end: needs 1 .. max_problems robots");
    if (!h->g_begun) return fail(h, ALORE_BE_E_INVALID, "manager_end: no alore_backend_manager_begin before it");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, fleet::end_enqueue(h->g_slab, h->g_params, count, h->g_now, search_status ? search_status : h->d_search_status,
                                 build_status ? build_status : h->d_build_status, plan_ok ? plan_ok : h->r_ok, T ? T : h->r_T, h->P,
                                 n_pieces ? n_pieces : h->d_M, (hipStream_t)stream));
    h->g_begun = false;
    return ALORE_BE_OK;
}

int alore_backend_manager_next_legs(alore_backend_handle h, int count, const double* poses, int pose_stride_bytes, const double* leg_yaw, int reset_legs,
                                    void* stream)
{
    BE_MANAGER(h, "manager_next_legs");
    if (count < 1 || count > h->B || !poses || !leg_yaw || !stride_ok(pose_stride_bytes, 24, 8))
        return fail(h, ALORE_BE_E_INVALID, "manager_next_legs: needs 1 .. max_problems poses with a stride that is a multiple of 8, at least 24, and the legs' yaws");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, fleet::next_legs_enqueue(h->g_slab, count, poses, pose_stride_bytes, h->t_status, h->t_n_order, h->t_leg_goal, leg_yaw, reset_legs,
                                       (hipStream_t)stream));
    return ALORE_BE_OK;
}

int alore_backend_device_manager(alore_backend_handle h, alore_backend_manager_view* out)
{
    BE_MANAGER(h, "device_manager");
    if (!out) return fail(h, ALORE_BE_E_INVALID, "device_manager: bad argument");
    const fleet::Slab& s = h->g_slab;
    *out = alore_backend_manager_view{h->B, fleet::N_COUNTERS, s.state, s.have_goal, s.have_start, s.leg, s.action, s.returned, s.plan_mask, s.fresh_mask,
                                      s.replan_mask, s.stop_mask, s.after_plan_mask, s.goal, s.start, s.plan_start_xytheta, s.loop_start_time,
                                      s.plan_start_time, s.traj_start_time, s.traj_total_time, s.time, s.counters};
    return ALORE_BE_OK;
}

int alore_backend_get_manager(alore_backend_handle h, int count, int* ints, double* doubles, int* counters)
{
    BE_MANAGER(h, "get_manager");
    if (count < 1 || count > h->B) return fail(h, ALORE_BE_E_INVALID, "get_manager: bad argument");
    BE_TRY(h, hipSetDevice(h->device));
    BE_TRY(h, hipDeviceSynchronize());
    const size_t n = count, B = h->B;
    const fleet::Slab& s = h->g_slab;
    if (ints) BE_TRY(h, hipMemcpy2D(ints, sizeof(int) * n, s.state, sizeof(int) * B, sizeof(int) * n, fleet::SLAB_INT_ROWS, hipMemcpyDeviceToHost));
    if (doubles) BE_TRY(h, hipMemcpy2D(doubles, sizeof(double) * n, s.goal, sizeof(double) * B, sizeof(double) * n, fleet::SLAB_DOUBLE_ROWS, hipMemcpyDeviceToHost));
    if (counters) BE_TRY(h, hipMemcpy(counters, s.counters, sizeof(int) * fleet::N_COUNTERS, hipMemcpyDeviceToHost));
    return ALORE_BE_OK;
}

} // extern "C"
