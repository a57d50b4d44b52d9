// backend_kernels.h -- launch interface between backend_capi.hip and backend_kernels.hip
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/alore_backend.h"

namespace backend {

using Config = alore_backend_config;
using LbfgsParam = alore_lbfgs_param;
using Status = alore_backend_status;

constexpr int MEM_MAX = 256; // L-BFGS history slots per problem (global_planning3ms.yaml: mem_size 256)
// per problem, next to the history: for every aligned chunk of 8 slots the 8 x 8 block G[k][l] = s_k . y_l (k < l; the rest stays
// zero) row by row, its transpose, then y's and 1 / y's per slot (backend_kernels.hip: two_loop_gram)
constexpr int GRAM_G = 0, GRAM_GT = (MEM_MAX / 8) * 64, GRAM_YS = 2 * GRAM_GT, GRAM_RYS = GRAM_YS + MEM_MAX, GRAM_DOUBLES = GRAM_RYS + MEM_MAX;
// The per-problem workspace of an evaluation is sized by the build's capacity P (16, 32 or 64 pieces): the 16 and 32 builds share
// the layout for 32 knots and 5 elimination steps, the 64 build has 64 knots and 6 steps
constexpr int ws_knots(int P) { return P <= 32 ? 32 : 64; }
constexpr int ws_steps(int P) { return P <= 32 ? 5 : 6; }
constexpr int pcr_doubles(int P) { return ws_steps(P) * ws_knots(P) * 8 + ws_knots(P) * 4; } // per problem: [step][knot][alpha, gamma (2 x 2 each)], then [knot][D^-1]
// ... followed in the same per-problem workspace by two node arrays of an evaluation that are written and read once or twice and so need
// no LDS: the order-2 node terms of the even nodes [knots * 9][2] and the duration-gradient terms per node [knots * 17]
constexpr int ws_eb(int P) { return pcr_doubles(P); }
constexpr int ws_nodet(int P) { return ws_eb(P) + ws_knots(P) * 9 * 2; }
constexpr int ws_cs(int P) { return ws_nodet(P) + ws_knots(P) * 17; }
constexpr int ws_doubles(int P) { return ws_cs(P) + 2 * ws_knots(P) * 17; } // ... and cos / sin of the heading per node [node][2]
static_assert(ws_doubles(16) == 3616 && ws_doubles(32) == 3616 && ws_eb(32) == 1408 && ws_nodet(32) == 1984 && ws_cs(32) == 2528,
              "the workspace of the 16 and 32 builds keeps its layout");

enum Mode { MODE_PLAN = 0, MODE_EVAL = 1, MODE_LBFGS = 2 };

struct MapView {
    const double* dist;
    int nx, ny;
    double x_lo, y_lo, x_hi, y_hi, res;
};

// device copy of the FlatTrajData batch; P = piece capacity
struct ProblemStore {
    int P;
    const int* M;            // [B]
    const double* inner;     // [B][(P-1)*2]  (yaw, s)
    const double* init_T;    // [B]
    const double* positions; // [B][P*2]      way-points (x, y) then final (x, y)
    const double* head;      // [B][6]        [d][p v a]
    const double* tail;      // [B][6]
    const double* start_xy;  // [B][2]
    const double* final_xy;  // [B][2]
    const int* if_cut;       // [B]
};

struct ResultStore {
    double* inner; // [B][(P-1)*2]
    double* T;     // [B][P]
    double* coef;  // [B][P*12]
    double* tail;  // [B][6]
    int* ok;       // [B]
    Status* status;
};

struct Params {
    Config cfg;
    MapView map;
    ProblemStore prob;
    ResultStore res;
    double* hist; // [B][MEM_MAX][2][3P]
    double* gram; // [B][GRAM_DOUBLES], zero-initialised once (the lower triangles are never written)
    double* pcr;  // [B][ws_doubles(P)] per-problem workspace of an evaluation: elimination factors of the knot system of the current evaluation (spline solve -> adjoint solve)
    int count, mode;
    // MODE_EVAL / MODE_LBFGS
    int stage, max_iter;
    double* x_io;         // [B][3P]
    double* g_out;        // [B][3P]
    const double* lam_in; // [B][2] or null
    const double* rho_in;
    double safe_dis, time_weight;
    double* cost_out; // [B]
    double* err_out;  // [B][2]
    int* ret_out;     // [B][3]: ret, iterations, evaluations
    const int* order;  // optional: workgroup w works on problem order[w] (longest problems first: a launch ends with its slowest wavefront)
    long long* stamps; // diagnostic (ALORE_BE_STAMPS=1): [64] cycles per phase of workgroup 0, [63] = last stamp
    // alore_backend_plan_masked: a workgroup whose slot b has the int at (char*)mask + b * mask_stride equal to 0 returns at entry
    const int* mask; // null: every slot is planned
    int mask_stride; // bytes
    // object classes (alore_backend_set_classes): slot b is planned with classes[class_of[b]]; all null: with cfg.  class_params:
    // [n_classes] copies of this block, block k with cfg = classes[k], written on the device in front of the launch (launch()); the
    // workgroup of slot b reads its parameters from block class_of[b].  Nothing of this is written by the optimiser kernel
    const Config* classes;
    const int* class_of; // [B]
    const Params* class_params;
    int n_classes;
};

size_t lds_bytes(int P);
// the parameter block is copied (asynchronously, stream-ordered) into d_params and read from there by the kernel;
// `p` must stay alive until the copy has been issued from pinned memory or has completed (callers keep it in the handle)
hipError_t launch(const Params& p, const Params* d_params, int P, hipStream_t s);

// the final collision check again, on the stored plans of the last launch against the map of now (backend_kernels.hip:
// check_plans_kernel): one wavefront per plan, a time window per plan, the threshold an argument, optionally the body points
struct CheckArgs {
    int count, P, R, n_check, body;
    const int* n_pieces;          // [B]
    const double *T, *coef;       // ResultStore
    const double* plan_start_xyt; // [B][3]
    MapView map;
    const double *t_from, *t_to;  // [count] or null (0, +infinity)
    double min_safe_dis, xv;      // xv: 0 for the standard differential model
    double check_pts[8][2];
    alore_backend_check* out;     // [count]
    // object classes: R, n_check, xv, check_pts and (use_class_thr) the threshold of slot b from classes[class_of[b]]; null: the above
    const Config* classes;
    const int* class_of;          // [B]
    int use_class_thr;            // min_safe_dis <= 0 was asked for: the class's final_min_safe_dis
};
// the kernel reads its arguments from d_args (device memory, filled in stream order before the launch)
hipError_t check_plans(const CheckArgs* d_args, int count, hipStream_t s);

// FlatTrajData from way-point paths (flat_traj_build.hip: build_problems_kernel, one wavefront per path, then launch_order_kernel)
struct BuildArgs {
    int count, P, K; // K: way-points per path in xy (<= 31)
    alore_front_end_params fe;
    const int* n_points;                   // [count]
    const double* xy;                      // [count][K][2]
    const double *start_yaw, *end_yaw;     // [count]
    const double *start_vaj, *start_oaj;   // [count][3] or null (zeros)
    const int* mask;                       // null, or slot b is rebuilt when the int at (char*)mask + b * mask_stride is not 0
    int mask_stride;
    // the problem slots (ProblemStore) and the plan start pose
    int *M, *if_cut;
    double *inner, *init_T, *positions, *head, *tail, *start_xy, *final_xy, *sxyt;
    int* status; // [count] build status: 0 built, 1 masked out, -1 bad point count, -2 more pieces than the slot holds
    int* order;  // [count] launch order: most pieces first, stable in the slot index
    // object classes: slot b is built with fe_classes[class_of[b]]; null: with fe
    const alore_front_end_params* fe_classes;
    const int* class_of; // [B]
};
// both kernels read their arguments from d_args (device memory, filled in stream order before the launch)
// (P: the handle's piece capacity, BuildArgs::P -- it selects the shape of launch_order_kernel)
hipError_t build_problems(const BuildArgs* d_args, int count, int P, hipStream_t s);

// path_search.hip: way-point paths by grid search on the handle's distance field (arithmetic in path_search.h): one workgroup per
// problem, the cost-to-goal field of the search window in LDS, then the walk and the pruning of removeCornerPts
struct SearchArgs {
    int count;
    MapView map;
    double safe_dis, window_margin;
    const double *start, *goal;    // x, y of problem b at (char*)p + b * stride (bytes)
    int start_stride, goal_stride;
    const int* mask;               // null, or slot b is searched when the int at (char*)mask + b * mask_stride is not 0
    int mask_stride;
    int lds_cells;                 // capacity of the field in LDS: min(nx ny, the largest window)
    int* n_points;                 // [count]
    double* xy;                    // [count][31][2]
    int* cost_ab;                  // [count][2]: the unpruned path costs a + b sqrt(2)
    int* status;                   // [count]
    int* sweeps;                   // [count] sweeps until the field stood still (diagnostic); visits of tiles for a wide slot
    // the reservation for windows of more than psearch::MAX_CELLS cells (read by search_paths_wide_kernel only); null without one
    unsigned* wide_slabs;          // [wide_slots][wide_cells] words
    int wide_cells, wide_slots;
    long long* wide_ticks;         // [count][2] diagnostic: ticks of the 100 MHz clock a wide slot took, and its walk and pruning of them
};
// the kernel reads its arguments from d_args (device memory, filled in stream order before the launch)
hipError_t search_paths(const SearchArgs* d_args, int count, int lds_cells, hipStream_t s);
// registers the field's LDS size with the runtime (once per device, not in stream order: call before the first search)
hipError_t search_configure();
// path_search_wide.hip: behind search_paths on the same stream, the slots that it left at E_WINDOW and whose window has at most
// wide_cells cells (arithmetic in path_search_wide.h): `slots` workgroups, workgroup j owns slab j and takes the slots j, j + slots,
// ... in turn; the field in the slab, relaxed tile by tile in LDS
hipError_t search_paths_wide(const SearchArgs* d_args, int slots, hipStream_t s);
hipError_t search_wide_configure();

// task_plan.hip: the visit order of rearrangement missions from path costs on the handle's distance field (arithmetic and contract
// in task_plan.h): task_costs_kernel, one workgroup per (mission, source point), fills the cost matrices; task_order_kernel, one
// workgroup per mission behind it on the same stream, the orders, totals and legs
struct TaskArgs {
    int count, max_tasks, mode;
    MapView map;
    double safe_dis, window_margin;
    const int* n_tasks;            // [count]
    const double* points;          // point p of mission m at (char*)points + m * point_row_stride + 16 p
    int point_row_stride;
    const int* assign;             // null, or [count][max_tasks]
    const int* mask;               // null, or mission m is planned when the int at (char*)mask + m * mask_stride is not 0
    int mask_stride;
    int lds_cells;                 // capacity of the field in LDS: min(nx ny, the largest window)
    int* status;                   // [count]
    int* matrix;                   // [count][21][21][2]
    int* order;                    // [count][20]
    int* n_order;                  // [count]
    int* total;                    // [count][2]
    double *leg_start_xy, *leg_goal_xy; // [count][20][2]
    int *fields, *sweeps;          // [count]
    int *src_fields, *src_sweeps;  // [count][20] per source point: what task_order_kernel adds up (no atomics)
    int* assignment;               // [count][10], modes ASSIGNED and JOINT: the target of item i
    int* assign_total;             // [count][2], the sum of its carry legs
    // the reservation for missions whose window has more than lds_cells cells (alore_backend_task_reserve); null without one, and
    // then nothing below is read
    unsigned* wide_slabs;          // [wide_slots][wide_cells] words
    int wide_cells, wide_slots;
    int* src_range;                // [count][20] per source point of a wide mission: a field of it has a word out of range
    long long* src_ticks;          // [count][20] diagnostic: ticks of the 100 MHz clock that the fields of such a source took
};
// the largest window a launch with these arguments plans: what LDS holds, or the reservation's slab
__host__ __device__ inline long long task_window_cap(const TaskArgs& a)
{
    const long long wide = !a.wide_slabs ? 0 : a.wide_cells < (1 << 22) ? a.wide_cells : (1 << 22);
    return wide > a.lds_cells ? wide : a.lds_cells;
}
// task_assign_order_kernel (mode ASSIGNED) and task_joint_kernel (mode JOINT) stand in for task_order_kernel in a launch of their mode.
// The kernels read their arguments from d_args (device memory, filled in stream order before the launch)
// wide_slots > 0 (a reservation, whose fields d_args holds): task_costs_wide_kernel, wide_slots workgroups, between the two
hipError_t task_plan(const TaskArgs* d_args, int count, int max_tasks, int mode, int lds_cells, int wide_slots, hipStream_t s);
// the order phase alone, on the matrices that lie in the slab: the second launch of task_plan
hipError_t task_order(const TaskArgs* d_args, int count, int mode, hipStream_t s);
// registers the LDS sizes with the runtime (once per device, not in stream order: call before the first task_plan)
hipError_t task_configure();

// MSPlanner::get_the_predicted_state[_and_path] on the plans of the last launch (esdf_build.hip)
struct PredictArgs {
    int count, P;
    const int* n_pieces;
    const double *T, *coef;          // ResultStore
    const double* plan_start_xyt;    // [B][3] start pose of the plan (final_initStateXYTheta_)
    const double *start_time, *time; // [B] (start_time may be null = 0)
    const double* start_xyt;         // [B][3] or null (= plan start pose)
    double step, xv;
    bool standard_diff;
    double *xyt_out, *vaj_out, *oaj_out;
    int* forward_out;
    // object classes: xv and standard_diff of slot b from classes[class_of[b]]; null: the above
    const Config* classes;
    const int* class_of;
};
hipError_t predicted_state(const PredictArgs& g, hipStream_t s);
// MSPlanner::mincoPointPub on the plans of the last launch (esdf_build.hip)
struct PathArgs {
    int count, P, res;
    const int* n_pieces;
    const int* ok;                 // [B] or null: plans the optimiser rejected have no path
    const double *T, *coef;        // ResultStore
    const double* plan_start_xyt;  // [B][3]
    double xv;
    bool standard_diff;
    double* xy_out;                // [B][P (res + 1)][2]
    double* yaw_out;               // [B][P res] or null
    int* n_out;                    // [B] points written
    // object classes: xv and standard_diff of slot b from classes[class_of[b]]; null: the above
    const Config* classes;
    const int* class_of;
};
hipError_t path_points(const PathArgs& g, hipStream_t s);

// esdf_build.hip: SDFmap::updateESDF2d on the device
hipError_t esdf_fill_max(double* p, size_t n, hipStream_t s);
hipError_t esdf_update(const unsigned char* d_grid, int GLX, int GLY, double res, double x_lo, double y_lo, double odom_x, double odom_y,
                       double range, double* d_dist, hipStream_t s, int* empty_window);
// the same five kernels with a caller-owned workspace: enqueues and returns (no allocation, no wait)
struct EsdfWorkspace {
    double *tmp, *pos, *neg, *z; // tmp, pos, neg: [cells]; z: [lines (lines + 3)]
    int* v;                      // [lines (lines + 2)]
    size_t cells;                // capacity: (X + 1) (Y + 1) of the largest window
    int lines;                   // capacity: max(X, Y) + 1
};
// esdf_workspace_size(GLX, GLY, res, range, &cells, &lines): esdf_window.h, with the window's arithmetic
hipError_t esdf_enqueue(const unsigned char* d_grid, int GLX, int GLY, double res, double x_lo, double y_lo, double odom_x, double odom_y,
                        double range, double* d_dist, const EsdfWorkspace& w, hipStream_t s, int* empty_window);

// occupancy_map.hip: the resident occupancy map (plan_env::SDFmap before updateESDF2d), arithmetic in occupancy_update.h
struct OccMap {
    int nx, ny;
    double x_lo, y_lo, res, range; // range: detection_range
    int perspective;
    double log_odds5[5];           // hit, miss, min, max, occ
    unsigned char* grid;           // [nx][ny] cell states (device)
    double* log_odds;              // [nx][ny] (device)
    int *count_hit, *count_all;    // [nx][ny], zero between scans (device)
    double* h_row;                 // host scratch: one coordinate row of the RemoveOutliers lattice, occ_lattice_cap doubles
};
void occ_log_odds(const alore_backend_map_params& p, double out[5]);
int occ_lattice_cap(double range, double res);
// the argument block of one scan: the kernels' arguments, then the marks of the lattice's columns [nx] and rows [ny]
size_t occ_block_bytes(int nx, int ny);
// fills the host copy of a scan's block (device addresses refer to d_block); false: the sensor is not strictly inside the map
bool occ_prepare_scan(const OccMap& m, double odom_x, double odom_y, const char* d_points, int n_points, int stride_bytes, char* h_block,
                      const char* d_block);
// launches the kernels of the scan whose block has been copied to d_block in stream order
hipError_t occ_enqueue_scan(const char* h_block, const char* d_block, hipStream_t s);
hipError_t occ_fill(double* p, size_t n, double value, hipStream_t s);

} // namespace backend
