// occupancy_update.h -- point clouds into the occupancy map, the arithmetic once (internal).
// Plain C++17, float64: __host__ __device__ under hipcc, no HIP dependency otherwise.  Restates the half of plan_env::SDFmap that
// runs before updateESDF2d (reference planning_ddr_opt/utils/plan_env/src/sdf_map.cpp): coord2gridIndex (:467-472), isInGloMap and
// closetPointInMap (:591-614), the end-point rule of raycastProcess (:146-163), getGridsBetweenPoints2D (:387-414) as a step
// function, the per-cell log-odds update of updateOccupancyMap (:291-312), the cell-state rule (:81-91), the if_perspective
// branch (:95-124) and RemoveOutliers (:316-350).  The small functions are what one lane of the kernels of occupancy_map.hip
// computes for its point or its cell; integrate_scan() strings them together serially and is what
// tests/harness/occupancy_check.cpp runs on the CPU.  The grid is indexed x * ny + y, x_hi = x_lo + nx * res.
//
// CONTRACTION.  Everything that decides a cell index is a correctly rounded double operation (subtract, multiply, divide,
// sqrt(dx * dx + dy * dy)); a fused multiply-add in their place moves points that lie within an ulp of a cell border.  hipcc
// contracts a * b + c by default: the pragma below turns that off for everything after it in the translation unit.  g++ does not
// contract in ISO mode (-std=c++17), and the CPU harness is built with -ffp-contract=off on top.  Device, harness and the NumPy
// oracle (tests/occupancy_cases.py) then agree bit for bit.
//
// Kept from the reference: the "- 1e-3" and the start value 1000000 of closetPointInMap; the last cell of a ray's line is not
// counted as a miss; "hit >= total - 3 * hit"; both early-outs of the log-odds update (the second writes clamp_min); the in_local
// reset; an Occupied cell is never turned free by the state rule; the lattice of RemoveOutliers comes from repeated addition of
// res starting at odom - detection_range (lattice_row), never from start + i * res.
//
// DEVIATIONS from the reference (each has a test):
//   counts     int, not short: the contract is fewer than 32768 rays through one cell per scan (where the two agree).  A cloud
//              of 32768 valid points or more breaks that contract in the sensor's cell, which every ray passes: the reference's
//              short total wraps negative there, "hit >= total - 3 * hit" turns true and the cell takes a hit update.  Here the
//              total is exact up to 2^31 - 1 and such a cell is a miss (the scenario "crowded" of tests/occupancy_cases.py);
//   non-finite a point with a non-finite coordinate is skipped (the reference would compute with it);
//   sensor     a scan whose sensor position is not strictly inside the map is refused (sensor_inside): closetPointInMap is
//              meaningless there;
//   map edge   the 3 x 3 fill round the sensor skips cells outside [0, nx) x [0, ny), and a lattice point whose cell lies in
//              the outermost ring of the map is skipped, since one of its four neighbours is outside (the reference reads and
//              writes out of bounds there).
// PARALLEL RemoveOutliers.  The lattice pass writes a cell only when it is Unknown and its four neighbours are Unoccupied.  A
// cell that is written therefore has no Unknown neighbour, and a cell that is read as a neighbour and could change (an Unknown
// one) makes the reader's test fail before and after the change: an Unknown cell next to an Unknown cell is never filled.  So
// the reference's in-place scan, a read-old / write-new pass and an in-place pass in any order give the same grid.  The cell of a
// lattice point (x, y) is (cell(x), cell(y)): the visited cells are the product of the visited columns and the visited rows
// (lattice_marks).  The 3 x 3 fill must come after the whole lattice pass (fused into it, it races with a neighbour's read); it
// touches only its own cell and is applied together with the state rule in a second pass (fill_and_state).
#ifndef ALORE_OCCUPANCY_UPDATE_H
#define ALORE_OCCUPANCY_UPDATE_H

#include <cmath>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define OCC_HD __host__ __device__ inline
#else
#define OCC_HD inline
#endif

namespace occ {

constexpr unsigned char UNKNOWN = 0, UNOCCUPIED = 1, OCCUPIED = 2; // sdf_map.h:98
constexpr double UNKNOWN_FLAG = 0.01;                              // log-odds start at clamp_min - 0.01 (sdf_map.h:179-180)

struct Geom {
    int nx, ny;
    double x_lo, y_lo, x_hi, y_hi, res, inv;
};
OCC_HD Geom make_geom(int nx, int ny, double x_lo, double y_lo, double res)
{
    return Geom{nx, ny, x_lo, y_lo, x_lo + nx * res, y_lo + ny * res, res, 1 / res};
}

struct LogOdds {
    double hit, miss, min, max, occ; // logit of p_hit, p_miss, p_min, p_max, p_occ
};
// the reference's logit macro (sdf_map.h:34); host only: computed once per map and handed to every consumer as five values
inline double logit(double p) { return std::log(p / (1 - p)); }

// one axis of coord2gridIndex: int((p - lo) * inv) clamped to [0, n - 1]; the comparisons come first so that the conversion
// is defined for every finite p (the result is the reference's wherever that is defined)
OCC_HD int cell_1d(double p, double lo, double inv, int n)
{
    const double v = (p - lo) * inv;
    if (!(v > 0.0)) return 0;
    if (v >= (double)n) return n - 1;
    return (int)v;
}
OCC_HD int cell_x(const Geom& g, double x) { return cell_1d(x, g.x_lo, g.inv, g.nx); }
OCC_HD int cell_y(const Geom& g, double y) { return cell_1d(y, g.y_lo, g.inv, g.ny); }

OCC_HD bool in_map(const Geom& g, double x, double y) { return x < g.x_hi && x > g.x_lo && y < g.y_hi && y > g.y_lo; }
// finite and strictly inside: what a scan's sensor position must be
OCC_HD bool sensor_inside(const Geom& g, double x, double y) { return in_map(g, x, y); } // a NaN fails every comparison
OCC_HD bool finite_point(double x, double y) { return x - x == 0.0 && y - y == 0.0; }

OCC_HD void closest_point_in_map(const Geom& g, double px, double py, double ox, double oy, double* cx, double* cy)
{
    const double diff[2] = {px - ox, py - oy};
    const double max_tc[2] = {g.x_hi - ox, g.y_hi - oy}, min_tc[2] = {g.x_lo - ox, g.y_lo - oy};
    double min_t = 1000000;
    for (int i = 0; i < 2; ++i) {
        if (std::fabs(diff[i]) > 0) {
            const double t1 = max_tc[i] / diff[i];
            if (t1 > 0 && t1 < min_t) min_t = t1;
            const double t2 = min_tc[i] / diff[i];
            if (t2 > 0 && t2 < min_t) min_t = t2;
        }
    }
    const double t = min_t - 1e-3;
    *cx = ox + t * diff[0];
    *cy = oy + t * diff[1];
}

OCC_HD void clip_to_range(double ox, double oy, double range, double length, double* x, double* y)
{
    *x = (*x - ox) / length * range + ox;
    *y = (*y - oy) / length * range + oy;
}
OCC_HD double distance(double ax, double ay, double bx, double by)
{
    const double dx = ax - bx, dy = ay - by;
    return std::sqrt(dx * dx + dy * dy);
}

// the end point of the ray to the finite point (px, py) and whether it is a hit: out of the map -> the closest point in the map,
// clipped to the range, a miss; in the map and beyond the range -> clipped, a miss; otherwise a hit
OCC_HD bool ray_end(const Geom& g, double ox, double oy, double range, double px, double py, double* ex, double* ey)
{
    bool hit = false;
    if (!in_map(g, px, py)) {
        closest_point_in_map(g, px, py, ox, oy, &px, &py);
        const double length = distance(px, py, ox, oy);
        if (length > range) clip_to_range(ox, oy, range, length, &px, &py);
    } else {
        const double length = distance(px, py, ox, oy);
        if (length > range) clip_to_range(ox, oy, range, length, &px, &py);
        else hit = true;
    }
    *ex = px;
    *ey = py;
    return hit;
}

// getGridsBetweenPoints2D as a step function: the line is the cells (x, y) from line_begin until line_done, the end cell included
struct Line {
    int x, y, ex, ey, dx, dy, sx, sy, err;
};
OCC_HD Line line_begin(int x0, int y0, int x1, int y1)
{
    Line l;
    l.x = x0; l.y = y0; l.ex = x1; l.ey = y1;
    l.dx = x1 > x0 ? x1 - x0 : x0 - x1;
    l.dy = y1 > y0 ? y1 - y0 : y0 - y1;
    l.sx = x0 < x1 ? 1 : -1;
    l.sy = y0 < y1 ? 1 : -1;
    l.err = l.dx - l.dy;
    return l;
}
OCC_HD bool line_at_end(const Line& l) { return l.x == l.ex && l.y == l.ey; }
OCC_HD void line_step(Line& l)
{
    const int e2 = 2 * l.err;
    if (e2 > -l.dy) { l.err -= l.dy; l.x += l.sx; }
    if (e2 < l.dx) { l.err += l.dx; l.y += l.sy; }
}

// the window of a scan and its box of cells, as updateOccupancyCallback computes them
struct Window {
    double x_lower, x_upper, y_lower, y_upper;
    int min_x, min_y, max_x, max_y;
};
OCC_HD Window window(const Geom& g, double ox, double oy, double range)
{
    const double half = std::ceil(range / g.res) * g.res;
    Window w;
    w.x_lower = std::fmax(ox - half, g.x_lo);
    w.x_upper = std::fmin(ox + half, g.x_hi);
    w.y_lower = std::fmax(oy - half, g.y_lo);
    w.y_upper = std::fmin(oy + half, g.y_hi);
    w.min_x = cell_x(g, w.x_lower); w.min_y = cell_y(g, w.y_lower);
    w.max_x = cell_x(g, w.x_upper); w.max_y = cell_y(g, w.y_upper);
    return w;
}
OCC_HD bool in_box(const Window& w, int x, int y) { return x >= w.min_x && x <= w.max_x && y >= w.min_y && y <= w.max_y; }

// updateOccupancyMap for one cell with a non-zero count: the new log-odds
OCC_HD double logodds_update(const LogOdds& L, double value, int hit, int total, bool in_local)
{
    const double update = hit >= total - 3 * hit ? L.hit : L.miss;
    if (update >= 0 && value >= L.max) return value;
    if (update <= 0 && value <= L.min) return L.min;
    if (!in_local) value = L.min;
    return std::fmin(std::fmax(value + update, L.min), L.max);
}

// "will not treat obstacles as free space"
OCC_HD unsigned char state_update(const LogOdds& L, unsigned char state, double value)
{
    if (state == UNKNOWN && value >= L.min && value <= L.occ) return UNOCCUPIED;
    if (value > L.occ) return OCCUPIED;
    return state;
}

// ---- RemoveOutliers -------------------------------------------------------------------------------------------------------
// one coordinate row of the lattice: odom - range, then repeated addition of res while below odom + range + 1e-10.
// `cap` = lattice_cap() is never reached, the break only guards the caller's array: the exact row has floor(2 range / res) + 1
// entries, and k additions are off by at most k ulps of the largest value, k * 2.2e-16 * |odom + range| with k < 2e6 for the
// range / res < 1e6 that map_create admits.  While that error plus the 1e-10 of the loop's bound stays below res (by orders of
// magnitude for any map in metres) rounding adds at most one entry, and (int)(2 range / res) + 2 holds the row
OCC_HD int lattice_row(double odom, double range, double res, double* out, int cap)
{
    int n = 0;
    for (double v = odom - range; v < odom + range + 1e-10; v += res) {
        if (n == cap) break;
        out[n++] = v;
    }
    return n;
}
OCC_HD int lattice_cap(double range, double res) { return (int)(2 * range / res) + 2; }
// marks[i] = 1 where a lattice coordinate that passes the reference's margin test (lo + res < v < hi - res) falls into cell i
OCC_HD void lattice_marks(const double* row, int n, double lo, double hi, double res, double inv, int cells, unsigned char* marks)
{
    for (int i = 0; i < cells; ++i) marks[i] = 0;
    const double low = lo + res, up = hi - res;
    for (int k = 0; k < n; ++k)
        if (row[k] > low && row[k] < up) marks[cell_1d(row[k], lo, inv, cells)] = 1;
}
// the lattice pass for the visited cell (x, y): does it turn Unoccupied?
OCC_HD bool outlier_fills(const unsigned char* grid, int nx, int ny, int x, int y)
{
    if (x < 1 || y < 1 || x > nx - 2 || y > ny - 2) return false; // the outermost ring: a neighbour is outside the map
    const unsigned char* c = grid + (long)x * ny + y;
    return c[0] == UNKNOWN && c[1] == UNOCCUPIED && c[-1] == UNOCCUPIED && c[ny] == UNOCCUPIED && c[-ny] == UNOCCUPIED;
}
// the second pass for cell (x, y): the 3 x 3 fill round the sensor's cell (sx, sy), then the state rule inside the box
OCC_HD unsigned char fill_and_state(const LogOdds& L, const Window& w, int sx, int sy, int x, int y, unsigned char state, double value)
{
    if (state == UNKNOWN && x >= sx - 1 && x <= sx + 1 && y >= sy - 1 && y <= sy + 1) state = UNOCCUPIED;
    if (in_box(w, x, y)) state = state_update(L, state, value);
    return state;
}

// the cells that the passes of a scan run over: the box and one cell round it, inside the map.  A ray's end point is within the
// range of the sensor up to rounding, so a count lies at most one cell outside the box (what the reference's in_local is for),
// and so does a cell of the 3 x 3 fill.
struct Box {
    int x0, y0, x1, y1;
};
OCC_HD Box pass_box(const Geom& g, const Window& w)
{
    Box b;
    b.x0 = w.min_x > 0 ? w.min_x - 1 : 0;
    b.y0 = w.min_y > 0 ? w.min_y - 1 : 0;
    b.x1 = w.max_x < g.nx - 1 ? w.max_x + 1 : g.nx - 1;
    b.y1 = w.max_y < g.ny - 1 ? w.max_y + 1 : g.ny - 1;
    return b;
}

// ---- one scan, serially (the CPU harness; the kernels of occupancy_map.hip do the same per lane) ----------------------------
struct Map {
    Geom g;
    LogOdds L;
    unsigned char* grid; // [nx][ny]
    double* log_odds;    // [nx][ny]
    int *count_hit, *count_all;
    unsigned char *mark_x, *mark_y; // [nx], [ny] scratch
    double* row;                    // [lattice_cap] scratch
};
constexpr int SCAN_OK = 0, SCAN_E_SENSOR = -1;

inline void read_point(const float* points, int stride_bytes, int i, double* x, double* y)
{
    const float* p = (const float*)((const char*)points + (long)i * stride_bytes);
    *x = (double)p[0];
    *y = (double)p[1];
}

inline int integrate_scan(Map& m, const float* points, int n_points, int stride_bytes, double ox, double oy, double range, bool perspective)
{
    const Geom& g = m.g;
    if (!sensor_inside(g, ox, oy)) return SCAN_E_SENSOR;
    const Window w = window(g, ox, oy, range);
    const Box b = pass_box(g, w);
    if (perspective) {
        for (int x = w.min_x; x <= w.max_x; ++x)
            for (int y = w.min_y; y <= w.max_y; ++y)
                if (m.grid[(long)x * g.ny + y] == UNKNOWN) m.grid[(long)x * g.ny + y] = UNOCCUPIED;
        for (int i = 0; i < n_points; ++i) {
            double px, py;
            read_point(points, stride_bytes, i, &px, &py);
            if (in_map(g, px, py)) m.grid[(long)cell_x(g, px) * g.ny + cell_y(g, py)] = OCCUPIED;
        }
        return SCAN_OK;
    }
    const int sx = cell_x(g, ox), sy = cell_y(g, oy);
    for (int i = 0; i < n_points; ++i) {
        double px, py, ex, ey;
        read_point(points, stride_bytes, i, &px, &py);
        if (!finite_point(px, py)) continue;
        const bool hit = ray_end(g, ox, oy, range, px, py, &ex, &ey);
        const int cx = cell_x(g, ex), cy = cell_y(g, ey);
        m.count_all[(long)cx * g.ny + cy] += 1;
        if (hit) m.count_hit[(long)cx * g.ny + cy] += 1;
        for (Line l = line_begin(sx, sy, cx, cy); !line_at_end(l); line_step(l)) m.count_all[(long)l.x * g.ny + l.y] += 1;
    }
    const int cap = lattice_cap(range, g.res);
    lattice_marks(m.row, lattice_row(ox, range, g.res, m.row, cap), g.x_lo, g.x_hi, g.res, g.inv, g.nx, m.mark_x);
    lattice_marks(m.row, lattice_row(oy, range, g.res, m.row, cap), g.y_lo, g.y_hi, g.res, g.inv, g.ny, m.mark_y);
    for (int x = b.x0; x <= b.x1; ++x)
        for (int y = b.y0; y <= b.y1; ++y) {
            const long c = (long)x * g.ny + y;
            if (m.count_all[c] != 0) {
                m.log_odds[c] = logodds_update(m.L, m.log_odds[c], m.count_hit[c], m.count_all[c], in_box(w, x, y));
                m.count_hit[c] = m.count_all[c] = 0;
            }
            if (m.mark_x[x] && m.mark_y[y] && outlier_fills(m.grid, g.nx, g.ny, x, y)) m.grid[c] = UNOCCUPIED;
        }
    for (int x = b.x0; x <= b.x1; ++x)
        for (int y = b.y0; y <= b.y1; ++y) {
            const long c = (long)x * g.ny + y;
            m.grid[c] = fill_and_state(m.L, w, sx, sy, x, y, m.grid[c], m.log_odds[c]);
        }
    return SCAN_OK;
}

} // namespace occ

#endif
