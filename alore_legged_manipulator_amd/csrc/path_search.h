// path_search.h -- way-point paths by grid search on the distance field, the arithmetic once (internal).
// Plain C++17: __host__ __device__ under hipcc, no HIP dependency otherwise.  What the reference gets from JPSPlanner::plan and
// removeCornerPts (planning_ddr_opt/front_end/src/jps_planner/jps_planner.cpp:31-68, 97-177; graph_search.cpp:92-243), stated so
// that it has exactly one answer: the reference's JPS returns A shortest path, and which one depends on how its heap orders equal
// keys.  The small functions are what the kernel of path_search.hip runs per thread; search_one() strings them together serially
// and is what tests/harness/path_search_check.cpp and tools/micro/path_search_host.cpp run on the CPU.  The oracle is
// tests/path_search_cases.py (Dijkstra on exact keys); harness and device equal it bit for bit.
//
// THE CONTRACT
//   map      dist [nx][ny], cell (ix, iy) at ix * ny + iy; the cell of a coordinate by coord2gridIndex (occ::cell_1d), the centre
//            of a cell ((double)i + 0.5) * res + lo (sdf_map.cpp:453-458).
//   problem  a start and a goal (x, y).  A non-finite coordinate or one outside [lo, hi] is E_ENDPOINT (the reference clamps);
//            start cell == goal cell is E_SAME_CELL (the reference hands on a one-point path).  Then, in this order: E_WINDOW,
//            the safe distance, E_NO_PATH for an end cell that is not free.
//   safe     max(min(max(min(safe_dis, 0.8 dist[start]), 0), 0.8 dist[goal]), 0), std::min / std::max as comparisons
//            (jps_planner.cpp:39-42).
//   window   the bounding box of the two cells grown by ceil(window_margin / res) cells a side, clipped to the map; more than
//            MAX_CELLS cells is E_WINDOW.  A cell is free when it is in the window and !(dist < safe).  The search never leaves
//            the window.
//   graph    eight moves, a move needs only its destination free (diagonals cut corners), cost 1 or sqrt 2
//            (graph_search.cpp:225-243).
//   cost     the exact pair (a, b) for a + b sqrt 2, packed a << 16 | b in one word; ordered by double(a) + double(b) * SQRT2
//            computed from the pair each time (a path has fewer than 32768 steps; distinct pairs in that range differ by more
//            than 5e-6, so the comparison is exact).  Never an accumulated floating-point sum.
//   field    g[c] = the least cost from c to the goal over free cells: the fixed point of relax_cell over all cells, unique
//            whatever the order of the relaxations, since a word only ever decreases to the cost of a real path.
//   path     walk from the start: at c a neighbour n qualifies when it is free and g[n] + w(c, n) == g[c] as pairs; keep the
//            previous direction if it qualifies, otherwise the first in the order (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1)
//            (1,-1).  Raw nodes: the start cell, every cell where the direction changes, the goal cell; more than MAX_NODES is
//            E_POINTS.
//   pruning  removeCornerPts (jps_planner.cpp:97-138) on the raw nodes: interior nodes are cell centres, the first and the last
//            are the given start and goal (:63-64) with the start and goal cells as their cells; checkLineCollision walks
//            getGridsBetweenPoints2D (:150-177) and tests dist < safe; norms sqrt(dx dx + dy dy); cost3 < cost1 + cost2 with
//            infinity for a blocked line.  More than MAX_POINTS way-points is E_POINTS.
// The line walk of JPSPlanner::getGridsBetweenPoints2D was compared with SDFmap's (occ::line_step): the same integer steps; it
// is restated here (line_step) because the two are separate functions in the reference and need not stay equal.
// A line between two cells of the window stays in their bounding box, hence in the window: the pruning reads the field words.
#ifndef ALORE_PATH_SEARCH_H
#define ALORE_PATH_SEARCH_H

#include <cmath>

#include "occupancy_update.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define PS_HD __host__ __device__ inline
#else
#define PS_HD inline
#endif

namespace psearch {

constexpr int MAX_CELLS = 32768; // window cells: one word each, 128 KiB of LDS
constexpr int MAX_NODES = 1024;  // raw nodes of a walk
constexpr int MAX_POINTS = 31;   // way-points of a pruned path (flat_traj::MAX_POINTS)
constexpr int OK = 0, MASKED = 1, E_ENDPOINT = -1, E_SAME_CELL = -2, E_WINDOW = -3, E_NO_PATH = -4, E_POINTS = -5;
constexpr unsigned BLOCKED = 0xFFFFFFFFu, UNREACHED = 0xFFFFFFFEu; // every cost word is below both
constexpr unsigned STRAIGHT = 0x10000u, DIAGONAL = 1u;
constexpr double SQRT2 = 1.4142135623730951;
constexpr int KEPT = 1 << 30; // mark of a node that the pruning keeps

struct Grid {
    const double* dist;
    int nx, ny;
    double x_lo, y_lo, x_hi, y_hi, res, inv;
};
PS_HD Grid make_grid(const double* dist, int nx, int ny, double x_lo, double y_lo, double x_hi, double y_hi, double res)
{
    return Grid{dist, nx, ny, x_lo, y_lo, x_hi, y_hi, res, 1 / res};
}
struct Params {
    double safe_dis, window_margin;
};
inline void default_params(Params* p) { p->safe_dis = 0.3; p->window_margin = 3.0; } // jps_safe_dis (jps3ms.yaml:2)

// the eight moves in the order of the tie rule
PS_HD int dir_dx(int k) { return (k == 0 || k == 1 || k == 7) ? 1 : (k >= 3 && k <= 5) ? -1 : 0; }
PS_HD int dir_dy(int k) { return (k >= 1 && k <= 3) ? 1 : (k >= 5) ? -1 : 0; }
PS_HD unsigned dir_cost(int k) { return (k & 1) ? DIAGONAL : STRAIGHT; }

PS_HD double key(unsigned w) { return (double)(w >> 16) + (double)(w & 0xFFFFu) * SQRT2; }
PS_HD double min_of(double a, double b) { return b < a ? b : a; } // std::min
PS_HD double max_of(double a, double b) { return a < b ? b : a; } // std::max
PS_HD double centre(int i, double lo, double res) { return ((double)i + 0.5) * res + lo; }

struct Window {
    int status;
    int x0, y0, wx, wy; // origin in the map and size in cells
    int sx, sy, gx, gy; // start and goal cell, window coordinates
    double safe;
};

PS_HD Window setup(const Grid& g, double sx, double sy, double gx, double gy, const Params& p)
{
    Window w{};
    w.status = E_ENDPOINT;
    if (!occ::finite_point(sx, sy) || !occ::finite_point(gx, gy)) return w;
    if (sx < g.x_lo || sx > g.x_hi || sy < g.y_lo || sy > g.y_hi || gx < g.x_lo || gx > g.x_hi || gy < g.y_lo || gy > g.y_hi) return w;
    const int csx = occ::cell_1d(sx, g.x_lo, g.inv, g.nx), csy = occ::cell_1d(sy, g.y_lo, g.inv, g.ny);
    const int cgx = occ::cell_1d(gx, g.x_lo, g.inv, g.nx), cgy = occ::cell_1d(gy, g.y_lo, g.inv, g.ny);
    w.status = E_SAME_CELL;
    if (csx == cgx && csy == cgy) return w;
    double md = std::ceil(p.window_margin / g.res);
    if (!(md > 0.0)) md = 0.0;
    if (md > 1.0e9) md = 1.0e9;
    const long long m = (long long)md;
    const long long xa = (csx < cgx ? csx : cgx) - m, xb = (csx < cgx ? cgx : csx) + m;
    const long long ya = (csy < cgy ? csy : cgy) - m, yb = (csy < cgy ? cgy : csy) + m;
    const int x0 = xa < 0 ? 0 : (int)xa, x1 = xb > g.nx - 1 ? g.nx - 1 : (int)xb;
    const int y0 = ya < 0 ? 0 : (int)ya, y1 = yb > g.ny - 1 ? g.ny - 1 : (int)yb;
    w.x0 = x0; w.y0 = y0; w.wx = x1 - x0 + 1; w.wy = y1 - y0 + 1;
    w.sx = csx - x0; w.sy = csy - y0; w.gx = cgx - x0; w.gy = cgy - y0;
    w.status = E_WINDOW;
    if ((long long)w.wx * w.wy > MAX_CELLS) return w;
    const double ds = g.dist[(long)csx * g.ny + csy], dg = g.dist[(long)cgx * g.ny + cgy];
    double safe = max_of(min_of(p.safe_dis, 0.8 * ds), 0.0);
    safe = max_of(min_of(safe, 0.8 * dg), 0.0);
    w.safe = safe;
    w.status = (ds < safe || dg < safe) ? E_NO_PATH : OK;
    return w;
}

// the first word of window cell (x, y): not free, the goal, or not reached yet.  dist is read here and nowhere else
PS_HD unsigned first_word(const Grid& g, const Window& w, int x, int y)
{
    if (g.dist[(long)(w.x0 + x) * g.ny + (w.y0 + y)] < w.safe) return BLOCKED;
    return (x == w.gx && y == w.gy) ? 0u : UNREACHED;
}

// one relaxation of cell (x, y) in gather form: reads the eight neighbours, writes only this cell.  true: the word went down
PS_HD bool relax_cell(unsigned* words, int wx, int wy, int x, int y)
{
    const int c = x * wy + y;
    const unsigned cur = words[c];
    if (cur == BLOCKED) return false;
    unsigned best = cur;
    double kb = key(cur); // UNREACHED has a larger key than any cost
    for (int k = 0; k < 8; ++k) {
        const int nx = x + dir_dx(k), ny = y + dir_dy(k);
        if (nx < 0 || ny < 0 || nx >= wx || ny >= wy) continue;
        const unsigned v = words[nx * wy + ny];
        if (v >= UNREACHED) continue;
        const unsigned cand = v + dir_cost(k);
        const double kc = key(cand);
        if (kc < kb) { best = cand; kb = kc; }
    }
    if (best == cur) return false;
    words[c] = best;
    return true;
}

// the walk from the start cell; nodes[] (capacity MAX_NODES) gets the raw nodes as window cell indices
PS_HD int walk(const unsigned* words, int wx, int wy, int sc, int gc, int* nodes, int* n_nodes)
{
    *n_nodes = 0;
    if (words[sc] >= UNREACHED) return E_NO_PATH;
    int n = 0, c = sc, prev = -1;
    nodes[n++] = sc;
    while (c != gc) {
        const int x = c / wy, y = c - x * wy;
        const unsigned cur = words[c];
        int pick = -1;
        for (int t = (prev >= 0 ? -1 : 0); t < 8 && pick < 0; ++t) {
            const int k = t < 0 ? prev : t;
            const int nx = x + dir_dx(k), ny = y + dir_dy(k);
            if (nx < 0 || ny < 0 || nx >= wx || ny >= wy) continue;
            const unsigned v = words[nx * wy + ny];
            if (v < UNREACHED && v + dir_cost(k) == cur) pick = k;
        }
        if (pick < 0) return E_NO_PATH; // never at the fixed point: a reached cell other than the goal has such a neighbour
        if (c != sc && pick != prev) {
            if (n == MAX_NODES) return E_POINTS;
            nodes[n++] = c;
        }
        c = (x + dir_dx(pick)) * wy + (y + dir_dy(pick));
        prev = pick;
    }
    if (n == MAX_NODES) return E_POINTS;
    nodes[n++] = gc;
    *n_nodes = n;
    return OK;
}

// JPSPlanner::getGridsBetweenPoints2D (jps_planner.cpp:150-177) as a step function: the cells from line_begin until line_at_end,
// the end cell included
struct Line {
    int x, y, ex, ey, dx, dy, sx, sy, err;
};
PS_HD Line line_begin(int x0, int y0, int x1, int y1)
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
PS_HD bool line_at_end(const Line& l) { return l.x == l.ex && l.y == l.ey; }
PS_HD void line_step(Line& l)
{
    const int e2 = 2 * l.err;
    if (e2 > -l.dy) { l.err -= l.dy; l.x += l.sx; }
    if (e2 < l.dx) { l.err += l.dx; l.y += l.sy; }
}
// checkLineCollision between two window cells
PS_HD bool line_blocked(const unsigned* words, int wy, int a, int b)
{
    const int ax = a / wy, bx = b / wy;
    Line l = line_begin(ax, a - ax * wy, bx, b - bx * wy);
    for (;;) {
        if (words[l.x * wy + l.y] == BLOCKED) return true;
        if (line_at_end(l)) return false;
        line_step(l);
    }
}

// way-point i of the raw path
PS_HD void node_xy(const Grid& g, const Window& w, const int* nodes, int n, int i, const double* sxy, const double* gxy, double* x, double* y)
{
    if (i == 0) { *x = sxy[0]; *y = sxy[1]; return; }
    if (i == n - 1) { *x = gxy[0]; *y = gxy[1]; return; }
    const int c = nodes[i] & (KEPT - 1), cx = c / w.wy;
    *x = centre(w.x0 + cx, g.x_lo, g.res);
    *y = centre(w.y0 + (c - cx * w.wy), g.y_lo, g.res);
}
PS_HD double segment_cost(const Grid& g, const Window& w, const unsigned* words, const int* nodes, int n, int i, int j, const double* sxy,
                          const double* gxy, bool check)
{
    if (check && line_blocked(words, w.wy, nodes[i] & (KEPT - 1), nodes[j] & (KEPT - 1))) return INFINITY;
    double ax, ay, bx, by;
    node_xy(g, w, nodes, n, i, sxy, gxy, &ax, &ay);
    node_xy(g, w, nodes, n, j, sxy, gxy, &bx, &by);
    const double dx = ax - bx, dy = ay - by;
    return std::sqrt(dx * dx + dy * dy);
}
// removeCornerPts on the raw nodes (n >= 2): marks the interior nodes it keeps with KEPT and returns the number of way-points
PS_HD int prune(const Grid& g, const Window& w, const unsigned* words, int* nodes, int n, const double* sxy, const double* gxy)
{
    int kept = 2, prev = 0;
    double cost1 = segment_cost(g, w, words, nodes, n, 0, 1, sxy, gxy, true);
    for (int i = 1; i < n - 1; ++i) {
        const double cost2 = segment_cost(g, w, words, nodes, n, i, i + 1, sxy, gxy, true);
        const double cost3 = segment_cost(g, w, words, nodes, n, prev, i + 1, sxy, gxy, true);
        if (cost3 < cost1 + cost2) {
            cost1 = cost3;
        } else {
            nodes[i] |= KEPT;
            ++kept;
            cost1 = segment_cost(g, w, words, nodes, n, i, i + 1, sxy, gxy, false);
            prev = i;
        }
    }
    return kept;
}

// after the field stands still: walk, prune, write.  A failure writes nothing but *n_points = 0
PS_HD int finish(const Grid& g, const Window& w, const unsigned* words, int* nodes, const double* sxy, const double* gxy, int* n_points,
                 double* xy, int* cost_ab)
{
    *n_points = 0;
    const int sc = w.sx * w.wy + w.sy, gc = w.gx * w.wy + w.gy;
    int n = 0;
    const int st = walk(words, w.wx, w.wy, sc, gc, nodes, &n);
    if (st != OK) return st;
    const int kept = prune(g, w, words, nodes, n, sxy, gxy);
    if (kept > MAX_POINTS) return E_POINTS;
    int at = 0;
    for (int i = 0; i < n; ++i) {
        if (i != 0 && i != n - 1 && !(nodes[i] & KEPT)) continue;
        node_xy(g, w, nodes, n, i, sxy, gxy, &xy[2 * at], &xy[2 * at + 1]);
        ++at;
    }
    *n_points = kept;
    cost_ab[0] = (int)(words[sc] >> 16);
    cost_ab[1] = (int)(words[sc] & 0xFFFFu);
    return OK;
}

// ---- one problem, serially: words[] holds the window (<= MAX_CELLS), nodes[] MAX_NODES ---------------------------------------
// the field by alternating forward and backward sweeps over all cells until one changes nothing; *sweeps counts them
inline int search_one(const Grid& g, const double* sxy, const double* gxy, const Params& p, unsigned* words, int* nodes, int* n_points,
                      double* xy, int* cost_ab, int* sweeps)
{
    *sweeps = 0;
    const Window w = setup(g, sxy[0], sxy[1], gxy[0], gxy[1], p);
    if (w.status != OK) { *n_points = 0; return w.status; }
    for (int x = 0; x < w.wx; ++x)
        for (int y = 0; y < w.wy; ++y) words[x * w.wy + y] = first_word(g, w, x, y);
    for (bool changed = true; changed;) {
        changed = false;
        if (*sweeps & 1) {
            for (int x = w.wx - 1; x >= 0; --x)
                for (int y = w.wy - 1; y >= 0; --y) changed |= relax_cell(words, w.wx, w.wy, x, y);
        } else {
            for (int x = 0; x < w.wx; ++x)
                for (int y = 0; y < w.wy; ++y) changed |= relax_cell(words, w.wx, w.wy, x, y);
        }
        ++*sweeps;
    }
    return finish(g, w, words, nodes, sxy, gxy, n_points, xy, cost_ab);
}

} // namespace psearch

#endif
