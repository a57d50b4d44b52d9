// mission_map.h -- the edits a rearrangement mission makes to the occupancy map, the arithmetic once (internal).
// Plain C++17, float64: __host__ __device__ under hipcc, no HIP dependency otherwise.  Restates what plan_manager does to the map
// while a mission runs (reference planning_ddr_opt/plan_manager/include/plan_manager/plan_manager.hpp): paintSquare / paintBox /
// paintTable / paintChair (:470-496), the three rules of MapUpdateThread (:498-554), the goal classification of MainThread with its
// nearest_point (:618-658) and the post-plan rule (:695-704), on top of SDFmap::setObs and setFree
// (utils/plan_env/src/sdf_map.cpp:485-509).  The small functions are what one lane of the kernels of mission_map.hip computes;
// paint_list() and the *_all() drivers string them together serially and are what tests/harness/mission_map_check.cpp runs on the
// CPU.  The grid is indexed x * ny + y (occupancy_update.h, whose Geom and cell states are used here).
//
// WHAT DECIDES A CELL (each is pinned by a test):
//   lattice    a rectangle is the reference's double loop "for (x = cx - hx; x <= cx + hx; x += res)": the coordinates come from
//              repeated addition of res in double, never from cx - hx + i * res (axis_cells);
//   narrowing  setObs / setFree narrow the coordinate to float first, compare that float with the double bounds (skip when < lo or
//              >= hi) and index with (int)((coord - lo) * inv) in double.  The cells of an edit are therefore neither a contiguous
//              range nor one cell per lattice point; per axis they are a first cell and a 64-bit mask of offsets from it (Axis);
//   state only the state grid is written (Occupied or Unoccupied); log-odds and counts stay as they are.
// The cell of the lattice point (x, y) is (cell(x), cell(y)) and a point is skipped when either coordinate is: the cells of an edit
// are the product of the cells of its two axes.
//
// CONTRACTION is off as in occupancy_update.h: every distance is sqrt(dx * dx + dy * dy) of correctly rounded double operations.
//
// DEVIATIONS from the reference:
//   validity   an edit with a field that is not finite, a negative half size or more than MAX_LATTICE lattice points on an axis
//              ((int)(2 h / res) + 2 > 64, the bound of occ::lattice_cap) is skipped and counted (edit_valid); the reference would
//              loop on.  A lattice that reaches MAX_LATTICE points stops there;
//   map edge   an index that rounding takes to n (a float just below hi) is clamped to n - 1; the reference writes out of bounds;
//   fleet      every mission of a handle edits the handle's ONE map: the fleet form of the reference's one robot with its own map.
//   A point more than 63 cells from the first cell of its axis is dropped (it cannot happen while a float's spacing at the
//   coordinate is far below res, i.e. for any map in metres).
#ifndef ALORE_MISSION_MAP_H
#define ALORE_MISSION_MAP_H

#include <cfloat>

#include "occupancy_update.h"

namespace mission {

constexpr int MAX_LATTICE = 64;
constexpr int MAX_TASKS = 10; // ALORE_BE_TASK_MAX_TASKS
constexpr int OK = 0, MASKED = 1, E_POINT = -1, E_TASKS = -6;
constexpr int PHASE_NONE = 0, PHASE_ITEM = 1, PHASE_TARGET = 2;
constexpr int GOAL_OK = 0, GOAL_E_POINT = -1;
constexpr int KIND_SQUARE = 0, KIND_BOX = 1, KIND_TABLE = 2, KIND_CHAIR = 3;

// alore_backend_map_edit, field for field
struct Edit {
    double cx, cy, hx, hy;
    int make_obs, reserved;
};
// alore_backend_mission_params, field for field
struct Params {
    double item_half, free_half, item_free_dist, target_lock_half, target_lock_dist, left_target_half, left_target_dist;
};
inline void default_params(Params* p)
{
    p->item_half = 0.5;        // plan_manager.hpp:518
    p->free_half = 0.5;        // :533
    p->item_free_dist = 2.0;   // :531
    p->target_lock_half = 0.3; // :547
    p->target_lock_dist = 0.5; // :545
    p->left_target_half = 0.2; // :700
    p->left_target_dist = 0.3; // :699
}

OCC_HD bool finite(double v) { return v - v == 0.0; }
// (int)(2 h / res) + 2 <= MAX_LATTICE, decided before the conversion so that it is defined for every h
OCC_HD bool half_fits(double h, double res) { return h >= 0.0 && 2 * h / res < (double)(MAX_LATTICE - 1); }
OCC_HD bool edit_valid(const Edit& e, double res)
{
    return finite(e.cx) && finite(e.cy) && finite(e.hx) && finite(e.hy) && half_fits(e.hx, res) && half_fits(e.hy, res);
}
// the index of the first edit of a host list that edit_valid refuses, or -1
inline long first_invalid(const Edit* edits, long n, double res)
{
    for (long k = 0; k < n; ++k)
        if (!edit_valid(edits[k], res)) return k;
    return -1;
}

// the cells one axis of an edit covers: cell first + k for every set bit k of mask; mask == 0: none (first = 0, last = -1)
struct Axis {
    int first, last;
    unsigned long long mask;
};
OCC_HD Axis axis_cells(double c, double h, double res, double lo, double hi, double inv, int n)
{
    Axis a{0, -1, 0ull};
    int k = 0;
    for (double v = c - h; v <= c + h; v += res) {
        if (k++ == MAX_LATTICE) break;
        const double f = (double)(float)v; // "float coord_x = coord.x()", then promoted again by every operation with a double
        if (f < lo || f >= hi) continue;
        int i = (int)((f - lo) * inv);
        if (i > n - 1) i = n - 1;
        if (a.mask == 0ull) a.first = i;
        if (i - a.first >= 64) continue;
        a.mask |= 1ull << (i - a.first);
        a.last = i;
    }
    return a;
}
OCC_HD Axis axis_x(const occ::Geom& g, const Edit& e) { return axis_cells(e.cx, e.hx, g.res, g.x_lo, g.x_hi, g.inv, g.nx); }
OCC_HD Axis axis_y(const occ::Geom& g, const Edit& e) { return axis_cells(e.cy, e.hy, g.res, g.y_lo, g.y_hi, g.inv, g.ny); }
OCC_HD unsigned char edit_state(const Edit& e) { return e.make_obs ? occ::OCCUPIED : occ::UNOCCUPIED; }

// what a call leaves behind: cells whose state after the call differs from before it, their box, skipped edits
struct Counters {
    int n_changed, min_x, min_y, max_x, max_y, n_skipped;
    int pad[2];
};
OCC_HD Counters no_change(int nx, int ny) { return Counters{0, nx, ny, -1, -1, 0, {0, 0}}; }

OCC_HD Edit make_edit(double cx, double cy, double hx, double hy, int make_obs) { return Edit{cx, cy, hx, hy, make_obs, 0}; }

// ---- missions ------------------------------------------------------------------------------------------------------------------
// the slab of the missions, one row per slot; kinds [.][MAX_TASKS], items and targets [.][MAX_TASKS][2]
struct Slab {
    int *status, *phase, *goal_item, *goal_target, *goal_status, *n, *kinds;
    double *items, *targets;
};
OCC_HD bool kind_half(int kind, double item_half, double* hx, double* hy)
{
    switch (kind) {
    case KIND_SQUARE: *hx = item_half; *hy = item_half; return true;
    case KIND_BOX: *hx = 0.25; *hy = 0.15; return true;   // paintBox
    case KIND_TABLE: *hx = 0.5; *hy = 0.25; return true;  // paintTable
    case KIND_CHAIR: *hx = 0.2; *hy = 0.2; return true;   // paintChair
    }
    return false;
}
// mission m from a row of 1 + 2 max_tasks (x, y) pairs (point 0, the robot, is ignored) and max_tasks kinds (NULL: squares).
// A mission that fails keeps nothing but its status
OCC_HD int set_one(const Slab& s, int m, int max_tasks, int n, const double* row, const int* kinds)
{
    int status = OK;
    if (n < 1 || n > max_tasks) status = E_TASKS;
    else {
        for (int i = 0; i < n; ++i) {
            double hx, hy;
            if (kinds && !kind_half(kinds[i], 0.0, &hx, &hy)) status = E_TASKS;
        }
        if (status == OK)
            for (int i = 2; i < 2 + 4 * n; ++i)
                if (!finite(row[i])) status = E_POINT;
    }
    s.status[m] = status;
    s.phase[m] = PHASE_NONE;
    s.goal_item[m] = s.goal_target[m] = -1;
    s.goal_status[m] = GOAL_OK;
    s.n[m] = status == OK ? n : 0;
    if (status != OK) return status;
    for (int i = 0; i < n; ++i) {
        s.kinds[m * MAX_TASKS + i] = kinds ? kinds[i] : KIND_SQUARE;
        s.items[(m * MAX_TASKS + i) * 2] = row[2 * (1 + i)];
        s.items[(m * MAX_TASKS + i) * 2 + 1] = row[2 * (1 + i) + 1];
        s.targets[(m * MAX_TASKS + i) * 2] = row[2 * (1 + n + i)];
        s.targets[(m * MAX_TASKS + i) * 2 + 1] = row[2 * (1 + n + i) + 1];
    }
    return status;
}
// "items -> OBS" for item i of mission m
OCC_HD Edit item_edit(const Slab& s, const Params& P, int m, int i)
{
    double hx = 0, hy = 0;
    kind_half(s.kinds[m * MAX_TASKS + i], P.item_half, &hx, &hy);
    return make_edit(s.items[(m * MAX_TASKS + i) * 2], s.items[(m * MAX_TASKS + i) * 2 + 1], hx, hy, 1);
}
// nearest_point: the first point at the least distance, from DBL_MAX with a strict <; -1 when every comparison fails
OCC_HD int nearest(const double* pts, int n, double px, double py, double* best)
{
    int at = -1;
    *best = DBL_MAX;
    for (int i = 0; i < n; ++i) {
        const double d = occ::distance(px, py, pts[2 * i], pts[2 * i + 1]);
        if (d < *best) { *best = d; at = i; }
    }
    return at;
}
// the classification at a plan start for a mission with status OK
OCC_HD void goals_one(const Slab& s, int m, double gx, double gy)
{
    if (s.status[m] != OK) return;
    if (!finite(gx) || !finite(gy)) {
        s.phase[m] = PHASE_NONE;
        s.goal_status[m] = GOAL_E_POINT;
        return;
    }
    double di, dt;
    s.goal_item[m] = nearest(s.items + m * MAX_TASKS * 2, s.n[m], gx, gy, &di);
    s.goal_target[m] = nearest(s.targets + m * MAX_TASKS * 2, s.n[m], gx, gy, &dt);
    s.phase[m] = di < dt ? PHASE_ITEM : PHASE_TARGET;
    s.goal_status[m] = GOAL_OK;
}
// one tick for mission m at the pose (px, py): which rules fire.  Rules 1 and 2 exclude each other (the phase is ITEM or TARGET)
struct Fired {
    int first; // 0 none, 1 rule 1 (free goal_item), 2 rule 2 (lock goal_target)
    int left;  // rule 3: the index of the target just left, or -1
};
OCC_HD int fired_count(const Fired& f) { return (f.first != 0 ? 1 : 0) + (f.left >= 0 ? 1 : 0); }
OCC_HD Fired step_rules(const Slab& s, const Params& P, int m, double px, double py, bool after_plan)
{
    Fired f{0, -1};
    if (s.status[m] != OK || s.phase[m] == PHASE_NONE) return f;
    const double* items = s.items + m * MAX_TASKS * 2;
    const double* targets = s.targets + m * MAX_TASKS * 2;
    if (s.phase[m] == PHASE_ITEM) {
        const double* p = items + 2 * s.goal_item[m];
        if (occ::distance(px, py, p[0], p[1]) < P.item_free_dist) f.first = 1;
    }
    if (s.phase[m] == PHASE_TARGET) {
        const double* p = targets + 2 * s.goal_target[m];
        if (occ::distance(px, py, p[0], p[1]) < P.target_lock_dist) f.first = 2;
    }
    if (after_plan && s.phase[m] == PHASE_ITEM) {
        double d;
        const int t = nearest(targets, s.n[m], px, py, &d);
        if (t >= 0 && d < P.left_target_dist) f.left = t;
    }
    return f;
}
// the edits of the rules that fired, in rule order
OCC_HD Edit first_edit(const Slab& s, const Params& P, int m, int first)
{
    const double* p = first == 1 ? s.items + (m * MAX_TASKS + s.goal_item[m]) * 2 : s.targets + (m * MAX_TASKS + s.goal_target[m]) * 2;
    const double half = first == 1 ? P.free_half : P.target_lock_half;
    return make_edit(p[0], p[1], half, half, first == 1 ? 0 : 1);
}
OCC_HD Edit left_edit(const Slab& s, const Params& P, int m, int left)
{
    const double* p = s.targets + (m * MAX_TASKS + left) * 2;
    return make_edit(p[0], p[1], P.left_target_half, P.left_target_half, 1);
}
OCC_HD int step_one(const Slab& s, const Params& P, int m, double px, double py, bool after_plan, Edit* out)
{
    const Fired f = step_rules(s, P, m, px, py, after_plan);
    if (f.first != 0) out[0] = first_edit(s, P, m, f.first);
    if (f.left >= 0) out[f.first != 0 ? 1 : 0] = left_edit(s, P, m, f.left);
    return fired_count(f);
}

// ---- serially (the CPU harness; the kernels of mission_map.hip give the same result) ----------------------------------------------
// the edits one after the other in list order; the counters from the grid before and after (`before`: scratch of nx * ny cells)
inline Counters paint_list(const occ::Geom& g, unsigned char* grid, const Edit* edits, long n, unsigned char* before)
{
    Counters c = no_change(g.nx, g.ny);
    const long cells = (long)g.nx * g.ny;
    for (long k = 0; k < cells; ++k) before[k] = grid[k];
    for (long k = 0; k < n; ++k) {
        if (!edit_valid(edits[k], g.res)) { c.n_skipped += 1; continue; }
        const Axis ax = axis_x(g, edits[k]), ay = axis_y(g, edits[k]);
        for (int i = 0; i < 64; ++i)
            for (int j = 0; j < 64; ++j)
                if ((ax.mask >> i & 1ull) && (ay.mask >> j & 1ull)) grid[(long)(ax.first + i) * g.ny + ay.first + j] = edit_state(edits[k]);
    }
    for (int x = 0; x < g.nx; ++x)
        for (int y = 0; y < g.ny; ++y)
            if (grid[(long)x * g.ny + y] != before[(long)x * g.ny + y]) {
                c.n_changed += 1;
                if (x < c.min_x) c.min_x = x;
                if (y < c.min_y) c.min_y = y;
                if (x > c.max_x) c.max_x = x;
                if (y > c.max_y) c.max_y = y;
            }
    return c;
}
// the item edits of the missions set in one call (set[m] != 0 and status OK), slot order, item order; returns their number
inline long item_edits_all(const Slab& s, const Params& P, int count, const int* set, Edit* out)
{
    long n = 0;
    for (int m = 0; m < count; ++m)
        if (set[m] && s.status[m] == OK)
            for (int i = 0; i < s.n[m]; ++i) out[n++] = item_edit(s, P, m, i);
    return n;
}
inline long step_all(const Slab& s, const Params& P, int count, const double* poses_xy, const int* after_plan, Edit* out)
{
    long n = 0;
    for (int m = 0; m < count; ++m) n += step_one(s, P, m, poses_xy[2 * m], poses_xy[2 * m + 1], after_plan[m] != 0, out + n);
    return n;
}

} // namespace mission

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

// ---- the kernels of mission_map.hip ------------------------------------------------------------------------------------------------
namespace mission {

// what the first pass leaves per edit for the second: the cells of both axes and the state to write (0: the edit is skipped)
struct Desc {
    int x0, x1, y0, y1;
    unsigned long long mx, my;
    int value, pad;
};
constexpr int PAINT_CHUNK = 8192; // descriptors a handle starts with
// Paints the list into `grid` in stream order, as if one edit after the other.  d_count NULL: `limit` edits; otherwise
// min(max(*d_count, 0), limit), read on the device.  counters: 8 device ints (Counters), reset here.  d_desc holds desc_capacity
// descriptors: a list of no more than that is ONE launch of the two passes and the counters are exact.  A longer list is cut into
// launches in order; later-wins holds across them, and the counters then add up per launch (a cell that one launch changes and a later
// one changes back counts twice).
hipError_t paint_enqueue(const occ::Geom& g, unsigned char* grid, const Edit* d_edits, const int* d_count, int limit, Desc* d_desc,
                         int desc_capacity, int* d_counters, hipStream_t s);
// was_set[m] = the mask selects mission m (read like every mask of alore_backend.h; NULL: every mission)
hipError_t set_enqueue(const Slab& s, int count, int max_tasks, const int* n_tasks, const double* points, int row_stride, const int* kinds,
                       const int* mask, int mask_stride, int* was_set, hipStream_t st);
hipError_t goals_enqueue(const Slab& s, int count, const double* goals, int goal_stride, const int* mask, int mask_stride, hipStream_t st);
// the compacted edit list, slot order: the item edits of the missions of was_set (poses NULL), or one tick of every mission
hipError_t edits_enqueue(const Slab& s, const Params& P, int count, const int* was_set, const double* poses, int pose_stride,
                         const int* after_plan, int after_stride, Edit* out, int* out_count, hipStream_t st);

} // namespace mission
#endif

#endif
