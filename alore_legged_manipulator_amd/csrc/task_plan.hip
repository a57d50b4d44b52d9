// task_plan.hip -- the visit order of rearrangement missions from path costs on the device map (alore_backend_task_plan); the
// contract and the arithmetic in task_plan.h.
//
// task_costs_kernel: one workgroup of 1024 threads per (mission, source point k), for the targets j > k.  Every thread repeats the
// mission's checks (uniform, scalar); a workgroup that is masked out, surplus (k >= P - 1) or whose mission fails returns there,
// before any LDS access or barrier, and workgroup k = 0 alone writes the status of such a mission.  The others use the search
// kernel's field machinery (path_search.hip): psearch::first_word and psearch::relax_cell, one word per window cell in LDS, gather
// sweeps with one writer per word, alternating direction, an odd run length per thread, a workgroup-wide OR to stop.  The goal of
// the field is the SOURCE's cell, so after the fixed point the words at the target cells are d(k, j) for every j at once: thread
// j writes (k, j) and (j, k).  Targets whose safe_kj are equal share a field; a source whose targets differ in it runs one field
// per distinct value, in order of first appearance.  Every matrix entry has one writer: workgroup k writes row and column k
// beyond the diagonal and (k, k), workgroup P - 2 also (P - 1, P - 1).  No atomics: the per-source field and sweep counts go to
// src_fields / src_sweeps, which task_order_kernel adds up.
// LDS: 512 bytes of tables (the cells of the points, safe_kj) and 4 bytes per cell of the largest window the map allows,
// min(nx ny, 32768): up to 128.5 KiB, one workgroup per CU then.
//
// task_order_kernel: one workgroup of 256 threads per mission, behind the first kernel on the same stream.  The matrix goes to LDS.
// The optimal mode fills togo[S][last] (80 KiB of LDS, requested in that mode alone: a greedy launch takes 3.5 KiB) level by level in the size of the served set, from n down to 1, a barrier
// per level: the states of a level read the level above only.  Thread 0 then runs the reconstruction, or the greedy mode, and
// writes order, total and legs; it also adds up the diagnostics.
//
// task_assign_order_kernel (mode ASSIGNED) and task_joint_kernel (mode JOINT) take task_order_kernel's place in a launch of their
// mode: the same workgroup per mission, the same matrix in LDS, the same publishing by thread 0.  The first fills rest[T] (8 KiB)
// level by level in the number of targets given away, from n down to 0; thread 0 reconstructs the assignment into LDS, and the
// workgroup goes on with the optimal mode's togo (80 KiB) for it: 91.6 KiB in all.  The second fills togo[Si][St][last] (40 KiB,
// directly indexed, no ranking) level by level in the number of tasks done; 43.6 KiB.  A launch in the greedy or optimal mode
// enqueues what it always did.
#include "backend_kernels.h"
#include "task_plan_wide.h"
#include "wide_visit.h"

namespace backend {

namespace ps = psearch;
namespace tp = tplan;

constexpr int COST_THREADS = 1024, ORDER_THREADS = 256;
constexpr int TABLE_BYTES = 512;                                   // safe[32] doubles, cell[32] ints, padding
constexpr int TOGO_BYTES = tp::STATES * (int)sizeof(tp::Cost);     // 81920
constexpr int MATRIX_INTS = tp::P_MAX * tp::P_MAX * 2;
// LDS of task_order_kernel: the matrix, the order of thread 0 (no private array), and in the optimal mode alone the states behind them
constexpr int ORDER_AT = (MATRIX_INTS * (int)sizeof(int) + 15) & ~15;
constexpr int TOGO_AT = ORDER_AT + ((tp::MAX_LEGS * (int)sizeof(int) + 15) & ~15);
constexpr int GREEDY_LDS_BYTES = TOGO_AT, OPTIMAL_LDS_BYTES = TOGO_AT + TOGO_BYTES;
// LDS of the kernels that choose the assignment: matrix and order as above, 64 bytes for the chosen assignment, its total and the
// matching's status, then the tables: togo and rest (88 KiB) in the assigned mode, the joint togo (40 KiB) in the joint mode
constexpr int CHOSEN_AT = TOGO_AT, TABLE_AT = CHOSEN_AT + 64;
constexpr int ASSIGNED_LDS_BYTES = TABLE_AT + tp::ASSIGNED_STATES * (int)sizeof(tp::Cost);
constexpr int JOINT_LDS_BYTES = TABLE_AT + tp::JOINT_STATES * (int)sizeof(tp::Cost);
static_assert((tp::MAX_TASKS + 3) * (int)sizeof(int) <= 64 && ASSIGNED_LDS_BYTES <= 160 * 1024, "task_plan.hip: LDS of the assigned mode");

extern __shared__ __align__(16) unsigned char task_lds[];

struct MissionIn {
    const double* pts;
    const int* assign;
    int n;
    bool masked;
};
__device__ inline MissionIn mission_in(const TaskArgs& a, int m)
{
    MissionIn in;
    in.masked = a.mask && *(const int*)((const char*)a.mask + (size_t)m * a.mask_stride) == 0;
    in.pts = (const double*)((const char*)a.points + (size_t)m * a.point_row_stride);
    in.assign = a.assign ? a.assign + (size_t)m * a.max_tasks : nullptr;
    in.n = a.n_tasks[m];
    return in;
}

__global__ __launch_bounds__(COST_THREADS) void task_costs_kernel(const TaskArgs* __restrict__ gp)
{
    const TaskArgs& a = *gp;
    const int sources = 2 * a.max_tasks; // workgroups per mission: the sources 0 .. P_max - 2
    const int m = blockIdx.x / sources, k = blockIdx.x - m * sources, tid = threadIdx.x;
    const MissionIn in = mission_in(a, m);
    if (in.masked) {
        if (k == 0 && tid == 0) a.status[m] = tp::MASKED;
        return;
    }
    const ps::Grid g = ps::make_grid(a.map.dist, a.map.nx, a.map.ny, a.map.x_lo, a.map.y_lo, a.map.x_hi, a.map.y_hi, a.map.res);
    tp::Mission ms = tp::check_mission(g, in.n, a.max_tasks, in.pts, in.assign, a.mode, a.window_margin); // the same in every thread
    const int cells = ms.wx * ms.wy;
    if (ms.status == tp::OK && cells > a.lds_cells) ms.status = tp::E_WINDOW; // cannot happen: a window is clipped to the map
    if (ms.status != tp::OK) {
        if (k == 0 && tid == 0) {
            a.status[m] = ms.status;
            a.n_order[m] = 0;
        }
        return;
    }
    const int P = ms.P;
    if (k >= P - 1) return; // surplus: the mission has fewer points than the launch allows
    double* safe = (double*)task_lds;
    int* cell = (int*)(task_lds + 256);
    unsigned* words = (unsigned*)(task_lds + TABLE_BYTES);
    int* mat = a.matrix + (size_t)m * MATRIX_INTS;
    if (tid < P) {
        double dj, dk;
        cell[tid] = tp::point_cell(g, ms, in.pts, tid, &dj);
        (void)tp::point_cell(g, ms, in.pts, k, &dk);
        safe[tid] = tp::pair_safe(a.safe_dis, dk, dj); // used for tid > k only
    }
    if (tid == 0) {
        tp::put_entry(mat, k, k, tp::Cost{0, 0});
        if (k == P - 2) tp::put_entry(mat, P - 1, P - 1, tp::Cost{0, 0});
    }
    __syncthreads();
    const int cell_k = cell[k];
    const int chunk = ((cells + COST_THREADS - 1) / COST_THREADS) | 1;
    const int lo = min(tid * chunk, cells), hi = min(lo + chunk, cells);
    int fields = 0, most = 0;
    for (int j = k + 1; j < P; ++j) {
        const double s = safe[j];
        bool first = true;
        for (int e = k + 1; e < j; ++e) first = first && !(safe[e] == s);
        if (!first) continue; // uniform
        const ps::Window w = tp::field_window(ms, cell_k, s);
        for (int c = tid; c < cells; c += COST_THREADS) {
            const int x = c / w.wy;
            words[c] = ps::first_word(g, w, x, c - x * w.wy);
        }
        __syncthreads();
        int sweeps = 0;
        for (;;) {
            int changed = 0;
            if (lo < hi) {
                if (sweeps & 1) {
                    int x = (hi - 1) / w.wy, y = (hi - 1) - x * w.wy;
                    for (int c = hi - 1; c >= lo; --c) {
                        changed |= (int)ps::relax_cell(words, w.wx, w.wy, x, y);
                        if (--y < 0) { y = w.wy - 1; --x; }
                    }
                } else {
                    int x = lo / w.wy, y = lo - x * w.wy;
                    for (int c = lo; c < hi; ++c) {
                        changed |= (int)ps::relax_cell(words, w.wx, w.wy, x, y);
                        if (++y == w.wy) { y = 0; ++x; }
                    }
                }
            }
            ++sweeps;
            if (!__syncthreads_or(changed)) break;
        }
        ++fields;
        most = max(most, sweeps);
        if (tid >= j && tid < P && safe[tid] == s) {
            const tp::Cost c = tp::read_cost(words, cell_k, cell[tid]);
            tp::put_entry(mat, k, tid, c);
            tp::put_entry(mat, tid, k, c);
        }
        __syncthreads(); // the words are read out before the next field overwrites them
    }
    if (tid == 0) {
        a.src_fields[(size_t)m * tp::MAX_LEGS + k] = fields;
        a.src_sweeps[(size_t)m * tp::MAX_LEGS + k] = most;
    }
}

// ---- missions on windows beyond LDS (alore_backend_task_reserve) ----------------------------------------------------------------
// task_costs_wide_kernel: `wide_slots` workgroups of 1024 threads between task_costs_kernel and the order kernel on the same stream,
// on a handle with a task reservation only.  Workgroup j owns slab j and takes the work items i = m (2 max_tasks) + k, mission m
// and source point k, for i = j, j + slots, ...: the sources of one mission spread over the workgroups.  A mission whose status
// task_costs_kernel did not leave at E_WINDOW is passed over at the cost of one load.  For the others every thread repeats the
// mission's checks with the reservation's cap (uniform); an item is worked on if the mission is OK under that cap, its window has
// more than lds_cells cells (task_costs_kernel left it at E_WINDOW) and k < P - 1, and skipped otherwise.  Per distinct safe_kj in
// order of first appearance: every word of the window is initialised in the slab (a slab that served another field leaks nothing),
// the field is relaxed tile by tile exactly as search_paths_wide_kernel does it -- wide_visit.h is the visit both run; thread 0
// keeps the dirty bits in LDS and picks the next tile -- the window is scanned for words out of range, and the threads j <= tid < P
// with that safe_kj read their word from the slab and write the entries (k, tid) and (tid, k).  The diagonal as task_costs_kernel
// writes it.  src_fields, src_sweeps (the most visits of tiles) and src_range go to the [count][20] arrays that the order kernel
// reads, the time of the source's fields to src_ticks (diagnostic).  No atomics; a slab has one owner, no workgroup waits for another or reads what another wrote.
// LDS: (126 + 2)^2 words of tile, the dirty bits of the largest window (4164 bytes), the next tile, 512 bytes of tables: 69 KiB.
constexpr int WIDE_TABLE_AT = ((WIDE_TILE_WORDS + WIDE_DIRTY_WORDS + 1) * (int)sizeof(unsigned) + 15) & ~15;
constexpr int COST_WIDE_LDS_BYTES = WIDE_TABLE_AT + TABLE_BYTES;

__global__ __launch_bounds__(WIDE_THREADS) void task_costs_wide_kernel(const TaskArgs* __restrict__ gp)
{
    const TaskArgs& a = *gp;
    const int tid = threadIdx.x;
    unsigned* tile = (unsigned*)task_lds;
    unsigned* dirty = tile + WIDE_TILE_WORDS;
    int* next = (int*)(dirty + WIDE_DIRTY_WORDS);
    double* safe = (double*)(task_lds + WIDE_TABLE_AT);
    int* cell = (int*)(task_lds + WIDE_TABLE_AT + 256);
    unsigned* slab = a.wide_slabs + (size_t)blockIdx.x * a.wide_cells;
    const long long cap = task_window_cap(a);
    const ps::Grid g = ps::make_grid(a.map.dist, a.map.nx, a.map.ny, a.map.x_lo, a.map.y_lo, a.map.x_hi, a.map.y_hi, a.map.res);
    const int sources = 2 * a.max_tasks, items = a.count * sources;
    for (int i = blockIdx.x; i < items; i += a.wide_slots) {
        const int m = i / sources, k = i - m * sources;
        if (a.status[m] != tp::E_WINDOW) continue; // what task_costs_kernel left: the same in every thread, as every branch up to the first barrier
        const MissionIn in = mission_in(a, m);
        if (in.masked) continue;
        const tp::Mission ms = tp::check_mission(g, in.n, a.max_tasks, in.pts, in.assign, a.mode, a.window_margin, cap);
        const int cells = ms.wx * ms.wy, P = ms.P;
        if (ms.status != tp::OK || cells <= a.lds_cells || k >= P - 1) continue;
        int* mat = a.matrix + (size_t)m * MATRIX_INTS;
        if (tid < P) {
            double dj, dk;
            cell[tid] = tp::point_cell(g, ms, in.pts, tid, &dj);
            (void)tp::point_cell(g, ms, in.pts, k, &dk);
            safe[tid] = tp::pair_safe(a.safe_dis, dk, dj); // used for tid > k only
        }
        if (tid == 0) {
            tp::put_entry(mat, k, k, tp::Cost{0, 0});
            if (k == P - 2) tp::put_entry(mat, P - 1, P - 1, tp::Cost{0, 0});
        }
        __syncthreads();
        const long long t_begin = wall_clock64();
        const int cell_k = cell[k];
        int fields = 0, most = 0, range = 0;
        for (int j = k + 1; j < P; ++j) {
            const double s = safe[j];
            bool first = true;
            for (int e = k + 1; e < j; ++e) first = first && !(safe[e] == s);
            if (!first) continue; // uniform
            const ps::Window w = tp::field_window(ms, cell_k, s);
            for (int c = tid; c < cells; c += WIDE_THREADS) {
                const int x = c / w.wy;
                slab[c] = ps::first_word(g, w, x, c - x * w.wy);
            }
            const ps::Tiling tl = ps::make_tiling<WTX, WTY>(w);
            const int n_tiles = tl.ntx * tl.nty;
            for (int e = tid; e < (n_tiles + 31) / 32; e += WIDE_THREADS) dirty[e] = 0u;
            __syncthreads();
            ps::Cursor cu = ps::cursor_begin();
            int visits = 0;
            if (tid == 0) tp::dirty_begin<WTX, WTY>(dirty, tl, w); // the root's tile and those of its neighbours
            for (;;) {
                if (tid == 0) *next = ps::next_visit(dirty, n_tiles, cu);
                __syncthreads();
                const int t = *next;
                if (t < 0) break;
                ++visits;
                if (wide_visit(slab, w, ps::tile_at<WTX, WTY>(w, tl, t), tile, tid) && tid == 0) ps::mark_neighbours(dirty, tl, t);
                __syncthreads(); // the stores before the next loads, and *next and the tile array are free again
            }
            int out = 0;
            for (int c = tid; c < cells; c += WIDE_THREADS) out |= (int)ps::out_of_range(slab[c]);
            range |= __syncthreads_or(out);
            ++fields;
            most = max(most, visits);
            if (tid >= j && tid < P && safe[tid] == s) {
                const tp::Cost c = tp::read_cost(slab, cell_k, cell[tid]);
                tp::put_entry(mat, k, tid, c);
                tp::put_entry(mat, tid, k, c);
            }
            __syncthreads(); // the words are read out before the next field overwrites them
        }
        if (tid == 0) {
            a.src_fields[(size_t)m * tp::MAX_LEGS + k] = fields;
            a.src_sweeps[(size_t)m * tp::MAX_LEGS + k] = most;
            a.src_range[(size_t)m * tp::MAX_LEGS + k] = range;
            a.src_ticks[(size_t)m * tp::MAX_LEGS + k] = wall_clock64() - t_begin;
        }
        __syncthreads(); // the tables are read out before the next item overwrites them
    }
}

// ---- what the three order kernels share --------------------------------------------------------------------------------------
// the mission of an order kernel's workgroup; false where the cost kernels wrote the status and there is nothing to order.  A
// mission on a window beyond LDS (it took task_costs_wide_kernel; task_costs_kernel left its status at E_WINDOW) has its per-source
// range flags read here, by every thread alike: one set, and thread 0 publishes E_RANGE -- status, n_order = 0, the diagnostics --
// and nothing is ordered.  The flags of no other mission are read
__device__ inline void publish(const TaskArgs& a, int m, const double* pts, int n, int P, int status, const int* order, int n_order, const int* total);
__device__ inline bool order_mission(const TaskArgs& a, int m, MissionIn* in, tp::Mission* ms)
{
    *in = mission_in(a, m);
    if (in->masked) return false;
    const ps::Grid g = ps::make_grid(a.map.dist, a.map.nx, a.map.ny, a.map.x_lo, a.map.y_lo, a.map.x_hi, a.map.y_hi, a.map.res);
    *ms = tp::check_mission(g, in->n, a.max_tasks, in->pts, in->assign, a.mode, a.window_margin, task_window_cap(a));
    if (ms->status != tp::OK) return false;
    if (ms->wx * ms->wy <= a.lds_cells) return true;
    int range = 0;
    for (int k = 0; k < ms->P - 1; ++k) range |= a.src_range[(size_t)m * tp::MAX_LEGS + k];
    if (!range) return true;
    if (threadIdx.x == 0) publish(a, m, in->pts, in->n, ms->P, tp::E_RANGE, nullptr, 0, nullptr);
    return false;
}
// the matrix of the mission to LDS; the barrier behind it is the caller's
__device__ inline void load_matrix(const TaskArgs& a, int m, int P, int* mat, int tid)
{
    const int* gm = a.matrix + (size_t)m * MATRIX_INTS;
    for (int e = tid; e < P * P; e += ORDER_THREADS) {
        const int i = e / P, j = e - i * P, at = (i * tp::P_MAX + j) * 2;
        mat[at] = gm[at];
        mat[at + 1] = gm[at + 1];
    }
}
// togo[S][last] of the routing for `assign`, level by level; ends behind a barrier
__device__ inline void fill_togo(const int* mat, int n, const int* assign, tp::Cost* togo, int tid)
{
    for (int level = n; level >= 1; --level) {
        for (unsigned S = tid; S < (1u << n); S += ORDER_THREADS) {
            if (__popc(S) != level) continue;
            for (int last = 0; last < n; ++last)
                if ((S >> last) & 1u) togo[S * tp::MAX_TASKS + last] = tp::togo_state(mat, n, assign, togo, S, last);
        }
        __syncthreads();
    }
}
// thread 0 publishes its mission: the diagnostics added up, status and n_order, and with status OK the total, the order and the legs
__device__ inline void publish(const TaskArgs& a, int m, const double* pts, int n, int P, int status, const int* order, int n_order, const int* total)
{
    int fields = 0, most = 0;
    for (int k = 0; k < P - 1; ++k) {
        fields += a.src_fields[(size_t)m * tp::MAX_LEGS + k];
        most = max(most, a.src_sweeps[(size_t)m * tp::MAX_LEGS + k]);
    }
    a.status[m] = status;
    a.n_order[m] = n_order;
    a.fields[m] = fields;
    a.sweeps[m] = most;
    if (status != tp::OK) return;
    a.total[2 * (size_t)m] = total[0];
    a.total[2 * (size_t)m + 1] = total[1];
    for (int e = 0; e < n_order; ++e) a.order[(size_t)m * tp::MAX_LEGS + e] = order[e];
    tp::write_legs(pts, n, order, n_order, a.leg_start_xy + (size_t)m * tp::MAX_LEGS * 2, a.leg_goal_xy + (size_t)m * tp::MAX_LEGS * 2);
}
// the two rows of the modes that choose the assignment
__device__ inline void publish_assignment(const TaskArgs& a, int m, int n, const int* assign, const int* assign_total)
{
    for (int i = 0; i < n; ++i) a.assignment[(size_t)m * tp::MAX_TASKS + i] = assign[i];
    a.assign_total[2 * (size_t)m] = assign_total[0];
    a.assign_total[2 * (size_t)m + 1] = assign_total[1];
}

__global__ __launch_bounds__(ORDER_THREADS) void task_order_kernel(const TaskArgs* __restrict__ gp)
{
    const TaskArgs& a = *gp;
    const int m = blockIdx.x, tid = threadIdx.x;
    MissionIn in;
    tp::Mission ms;
    if (!order_mission(a, m, &in, &ms)) return;
    const int n = in.n, P = ms.P;
    int* mat = (int*)task_lds;
    tp::Cost* togo = a.mode == tp::OPTIMAL ? (tp::Cost*)(task_lds + TOGO_AT) : nullptr; // a greedy launch has no LDS for the states
    load_matrix(a, m, P, mat, tid);
    __syncthreads();
    if (a.mode == tp::OPTIMAL) fill_togo(mat, n, in.assign, togo, tid);
    if (tid != 0) return;
    int* order = (int*)(task_lds + ORDER_AT);
    int n_order = 0, total[2] = {0, 0}, status = tp::OK;
    if (a.mode == tp::OPTIMAL) status = tp::optimal_order(mat, n, in.assign, togo, order, &n_order, total);
    else tp::greedy_order(mat, n, order, &n_order, total);
    publish(a, m, in.pts, n, P, status, order, n_order, total);
}

// the assigned mode: rest[T] level by level, the matching by thread 0, then the optimal mode's states and order for it
__global__ __launch_bounds__(ORDER_THREADS) void task_assign_order_kernel(const TaskArgs* __restrict__ gp)
{
    const TaskArgs& a = *gp;
    const int m = blockIdx.x, tid = threadIdx.x;
    MissionIn in;
    tp::Mission ms;
    if (!order_mission(a, m, &in, &ms)) return; // the same in every thread
    const int n = in.n, P = ms.P;
    int* mat = (int*)task_lds;
    int* chosen = (int*)(task_lds + CHOSEN_AT); // the assignment, its total at [MAX_TASKS], the matching's status behind it
    tp::Cost* togo = (tp::Cost*)(task_lds + TABLE_AT);
    tp::Cost* rest = togo + tp::STATES;
    load_matrix(a, m, P, mat, tid);
    __syncthreads();
    for (int level = n; level >= 0; --level) {
        for (unsigned T = tid; T < (1u << n); T += ORDER_THREADS)
            if (__popc(T) == level) rest[T] = tp::rest_state(mat, n, rest, T);
        __syncthreads();
    }
    if (tid == 0) chosen[tp::MAX_TASKS + 2] = tp::matching(mat, n, rest, chosen, chosen + tp::MAX_TASKS);
    __syncthreads();
    const int matched = chosen[tp::MAX_TASKS + 2];
    int* order = (int*)(task_lds + ORDER_AT);
    int n_order = 0, total[2] = {0, 0};
    if (matched != tp::OK) { // uniform
        if (tid == 0) publish(a, m, in.pts, n, P, matched, order, n_order, total);
        return;
    }
    fill_togo(mat, n, chosen, togo, tid);
    if (tid != 0) return;
    const int status = tp::optimal_order(mat, n, chosen, togo, order, &n_order, total);
    publish_assignment(a, m, n, chosen, chosen + tp::MAX_TASKS);
    publish(a, m, in.pts, n, P, status, order, n_order, total);
}

// the joint mode: togo[Si][St][last] level by level in the number of tasks done, the reconstruction by thread 0
__global__ __launch_bounds__(ORDER_THREADS) void task_joint_kernel(const TaskArgs* __restrict__ gp)
{
    const TaskArgs& a = *gp;
    const int m = blockIdx.x, tid = threadIdx.x;
    MissionIn in;
    tp::Mission ms;
    if (!order_mission(a, m, &in, &ms)) return; // n <= JOINT_MAX_TASKS behind this: max_tasks of the block is tp::task_limit, more is E_TASKS
    const int n = in.n, P = ms.P;
    int* mat = (int*)task_lds;
    int* chosen = (int*)(task_lds + CHOSEN_AT);
    tp::Cost* togo = (tp::Cost*)(task_lds + TABLE_AT);
    load_matrix(a, m, P, mat, tid);
    __syncthreads();
    const unsigned span = tp::joint_span(n);
    for (int level = n; level >= 1; --level) {
        for (unsigned e = tid; e < span; e += ORDER_THREADS)
            if (tp::joint_on_level(n, e, level)) togo[e] = tp::joint_state(mat, n, togo, e);
        __syncthreads();
    }
    if (tid != 0) return;
    int* order = (int*)(task_lds + ORDER_AT);
    int n_order = 0, total[2] = {0, 0};
    const int status = tp::joint_order(mat, n, togo, order, &n_order, total, chosen, chosen + tp::MAX_TASKS);
    if (status == tp::OK) publish_assignment(a, m, n, chosen, chosen + tp::MAX_TASKS);
    publish(a, m, in.pts, n, P, status, order, n_order, total);
}

static size_t cost_lds_bytes(int lds_cells) { return TABLE_BYTES + sizeof(unsigned) * (size_t)lds_cells; }

hipError_t task_configure()
{
    hipError_t e = hipFuncSetAttribute((const void*)task_costs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cost_lds_bytes(ps::MAX_CELLS));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute((const void*)task_costs_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, COST_WIDE_LDS_BYTES);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute((const void*)task_order_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, OPTIMAL_LDS_BYTES);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute((const void*)task_assign_order_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ASSIGNED_LDS_BYTES);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void*)task_joint_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, JOINT_LDS_BYTES);
}

hipError_t task_plan(const TaskArgs* d_args, int count, int max_tasks, int mode, int lds_cells, int wide_slots, hipStream_t s)
{
    void* args[] = {&d_args};
    hipError_t e = hipLaunchKernel((const void*)task_costs_kernel, dim3(count * 2 * max_tasks), dim3(COST_THREADS), args, cost_lds_bytes(lds_cells), s);
    if (e != hipSuccess) return e;
    if (wide_slots > 0) { // a reservation: the missions that the first kernel left at E_WINDOW, on its slabs
        e = hipLaunchKernel((const void*)task_costs_wide_kernel, dim3(wide_slots), dim3(WIDE_THREADS), args, COST_WIDE_LDS_BYTES, s);
        if (e != hipSuccess) return e;
    }
    return task_order(d_args, count, mode, s);
}

hipError_t task_order(const TaskArgs* d_args, int count, int mode, hipStream_t s)
{
    void* args[] = {&d_args};
    hipError_t e;
    if (mode == tp::ASSIGNED) e = hipLaunchKernel((const void*)task_assign_order_kernel, dim3(count), dim3(ORDER_THREADS), args, ASSIGNED_LDS_BYTES, s);
    else if (mode == tp::JOINT) e = hipLaunchKernel((const void*)task_joint_kernel, dim3(count), dim3(ORDER_THREADS), args, JOINT_LDS_BYTES, s);
    else e = hipLaunchKernel((const void*)task_order_kernel, dim3(count), dim3(ORDER_THREADS), args,
                             mode == tp::OPTIMAL ? OPTIMAL_LDS_BYTES : GREEDY_LDS_BYTES, s);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

} // namespace backend
