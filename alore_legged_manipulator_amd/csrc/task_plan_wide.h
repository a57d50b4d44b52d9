// task_plan_wide.h -- task_plan.h for missions whose window does not fit in LDS, serially (internal).  Plain C++17.  The contract is
// task_plan.h's (paragraph WIDE); the tiling, the visit of a tile, the order of the visits, the dirty bits and the range flag are
// path_search_wide.h's functions as they are, the fields' roots, safe distances and the reading of the costs task_plan.h's: no
// arithmetic is restated.  plan_one_wide() is what tests/harness/task_plan_wide_check.cpp and tools/micro/task_plan_wide_host.cpp
// run on the CPU; the device's form is task_costs_wide_kernel (task_plan.hip).  The oracle is tests/task_plan_wide_cases.py.
#ifndef ALORE_TASK_PLAN_WIDE_H
#define ALORE_TASK_PLAN_WIDE_H

#include "path_search_wide.h"
#include "task_plan.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace tplan {

// the tiles that are dirty when a field starts: the root's, and every tile that holds one of the root's eight neighbours.  The
// root's word is reached before any visit, so the argument of path_search_wide.h (a clean tile was verified against words that
// have not changed since) needs every tile next to it verified once: were the root's tile alone dirty, a root on a tile's border
// whose neighbours inside its tile are all blocked would see a visit that changes nothing and marks nothing, and its free
// neighbours across the border would never be relaxed.  A root inside a tile marks its own tile alone, as the search does
template <int TX, int TY>
PS_HD void dirty_begin(unsigned* dirty, const psearch::Tiling& tl, const psearch::Window& w)
{
    psearch::dirty_set(dirty, psearch::tile_of_cell<TX, TY>(tl, w.gx, w.gy));
    for (int k = 0; k < 8; ++k) {
        const int x = w.gx + psearch::dir_dx(k), y = w.gy + psearch::dir_dy(k);
        if (x >= 0 && y >= 0 && x < w.wx && y < w.wy) psearch::dirty_set(dirty, psearch::tile_of_cell<TX, TY>(tl, x, y));
    }
}

// one field on the slab by the tiled iteration, every word of the window initialised first; returns the visits of tiles.
// tile[] holds (TX + 2)(TY + 2) words, dirty[] psearch::dirty_words<TX, TY>(cells of the slab)
template <int TX, int TY>
inline int field_wide(const psearch::Grid& g, const psearch::Window& w, unsigned* slab, unsigned* tile, unsigned* dirty)
{
    namespace ps = psearch;
    for (int x = 0; x < w.wx; ++x)
        for (int y = 0; y < w.wy; ++y) slab[x * w.wy + y] = ps::first_word(g, w, x, y);
    const ps::Tiling tl = ps::make_tiling<TX, TY>(w);
    const int n_tiles = tl.ntx * tl.nty;
    for (int i = 0; i < (n_tiles + 31) / 32; ++i) dirty[i] = 0u;
    dirty_begin<TX, TY>(dirty, tl, w);
    ps::Cursor cu = ps::cursor_begin();
    int visits = 0;
    for (int t; (t = ps::next_visit(dirty, n_tiles, cu)) >= 0;) {
        ++visits;
        if (ps::visit_tile<TX, TY>(slab, w, ps::tile_at<TX, TY>(w, tl, t), tile)) ps::mark_neighbours(dirty, tl, t);
    }
    return visits;
}

// fill_matrix with every field on the slab; true: a field has a reached word out of range (the matrix is then unspecified)
template <int TX, int TY>
inline bool fill_matrix_wide(const psearch::Grid& g, const Mission& m, const double* pts, const Params& p, unsigned* slab, unsigned* tile,
                             unsigned* dirty, const Out& o)
{
    int cell[P_MAX];
    double dist[P_MAX], safe[P_MAX];
    for (int j = 0; j < m.P; ++j) cell[j] = point_cell(g, m, pts, j, &dist[j]);
    int fields = 0, most = 0;
    bool range = false;
    for (int k = 0; k < m.P; ++k) put_entry(o.matrix, k, k, Cost{0, 0});
    for (int k = 0; k < m.P - 1; ++k) {
        for (int j = k + 1; j < m.P; ++j) safe[j] = pair_safe(p.safe_dis, dist[k], dist[j]);
        for (int j = k + 1; j < m.P; ++j) {
            bool first = true;
            for (int e = k + 1; e < j; ++e) first = first && !(safe[e] == safe[j]);
            if (!first) continue;
            const psearch::Window w = field_window(m, cell[k], safe[j]);
            const int visits = field_wide<TX, TY>(g, w, slab, tile, dirty);
            for (int c = 0; c < w.wx * w.wy; ++c) range |= psearch::out_of_range(slab[c]);
            ++fields;
            most = visits > most ? visits : most;
            for (int e = j; e < m.P; ++e) {
                if (!(safe[e] == safe[j])) continue;
                const Cost c = read_cost(slab, cell[k], cell[e]);
                put_entry(o.matrix, k, e, c);
                put_entry(o.matrix, e, k, c);
            }
        }
    }
    *o.fields = fields;
    *o.sweeps = most;
    return range;
}

// one mission in any of the four modes, always by the tiled iteration (whatever the size of its window).  slab[] holds max_cells
// words (or the map's cells if fewer), tile[] and dirty[] as field_wide takes them; table[] STATES pairs (OPTIMAL), ASSIGNED_STATES
// (ASSIGNED) or JOINT_STATES (JOINT), unused in the greedy mode; assign is read in the optimal mode only; assignment[MAX_TASKS]
// and assign_total[2] are written in the modes ASSIGNED and JOINT as the contract says
template <int TX, int TY>
inline int plan_one_wide(const psearch::Grid& g, int n, int max_tasks, const double* pts, const int* assign, const Params& p,
                         long long max_cells, unsigned* slab, unsigned* tile, unsigned* dirty, Cost* table, const Out& o, int* assignment,
                         int* assign_total)
{
    const bool chosen = p.mode == ASSIGNED || p.mode == JOINT;
    if (p.mode != OPTIMAL) assign = nullptr;
    const Mission m = check_mission(g, n, task_limit(p.mode, max_tasks), pts, assign, p.mode, p.window_margin, max_cells);
    if (m.status != OK) { *o.n_order = 0; return m.status; }
    if (fill_matrix_wide<TX, TY>(g, m, pts, p, slab, tile, dirty, o)) { *o.n_order = 0; return E_RANGE; }
    return chosen ? order_chosen(n, pts, p, table, o, assignment, assign_total) : order_given(n, pts, assign, p, table, o);
}

} // namespace tplan

#endif
