// path_search_wide.h -- the grid search of path_search.h on windows that do not fit in LDS, the arithmetic once (internal).
// Plain C++17 like path_search.h, whose contract holds unchanged: the same graph, exact pair costs, tie rule, walk, pruning and
// limits of MAX_NODES raw nodes and MAX_POINTS way-points.  Nothing of path_search.h is restated but setup (the cap becomes a
// parameter); walk, prune and finish read the field through a const unsigned* and run on the slab as they are.  The small
// functions are what the kernel of path_search_wide.hip runs per thread; search_one_wide() strings them together serially and is
// what tests/harness/path_search_wide_check.cpp and tools/micro/path_search_wide_host.cpp run on the CPU.  The oracle is
// tests/path_search_wide_cases.py; harness and device equal it bit for bit.
//
// THE SLAB holds the field of the window in memory that is not LDS, one word per cell, cell (x, y) at x * wy + y.
// THE TILING cuts the window into tiles of TX x TY interior cells (the last column and row of tiles may be smaller), tile
// (tx, ty) has the index tx * nty + ty.  A VISIT of a tile
//   loads   its interior and a one-cell halo from the slab into a (TX + 2) x (TY + 2) array; a halo cell outside the window is
//           BLOCKED;
//   relaxes the interior cells only, by alternating forward and backward gather sweeps, until a sweep changes nothing: the
//           tile's own fixed point against the halo it loaded.  Halo words are read and never written;
//   stores  the interior if any word changed.
// DIRTY FLAGS, one bit per tile.  At the start only the goal's tile is dirty.  A visit that changed a word marks the (up to) eight
// neighbouring tiles dirty and leaves its own tile clean; one that changed nothing only cleans its own.  Visits go over the dirty
// tiles in ascending tile order, then descending, and so on, until no tile is dirty.
//   Why that is the field: a word only ever goes down, and to the cost of a real path, so the iteration ends.  A clean tile was
//   last verified -- every interior cell relaxed without a change -- against words that have not changed since: a change of one
//   of its own words happens only in its own visit, which ends at its fixed point, and a change of a halo word is a change in a
//   neighbouring tile, which marks it dirty.  (A tile never visited holds no reached word next to a reached one: such a
//   neighbour would have changed in a visit, which marks.)  So when no tile is dirty, every cell has been verified against final
//   neighbours: the state is the fixed point of relax over the window, which is unique whatever the order of the relaxations.
//
// THE RANGE RULE.  The packed word holds a and b in 16 bits each, and key()'s exactness argument needs both below 32768.  A window
// of MAX_CELLS cells cannot break that, one of WIDE_MAX_CELLS can.  So here a word with a component of RANGE_LIMIT = 32767 or
// more is never extended (no component ever exceeds 32767, every comparison stays exact), and after the fixed point a slot
// fails with E_RANGE if any reached word of the window has a >= 32767 or b >= 32767: n_points = 0, the xy row untouched, before the
// walk (so before its E_NO_PATH and E_POINTS).
//   Why the flag is a property of the map and the window alone: along a least-cost path from the goal both components grow by at
//   most one a step, and least-cost pairs are unique.  If some cell the goal reaches has a least-cost pair with a component
//   >= 32767, the first such cell on its least-cost path has a component of exactly 32767 and every cell before it smaller ones:
//   nothing on that stretch was refused, the cell holds its exact pair, the flag is set.  Otherwise no refusal ever touched an
//   optimal path, every reached cell holds its least-cost pair (all components below 32767: no flag) and the field is exact.
//   An oracle therefore decides E_RANGE from its own field.
#ifndef ALORE_PATH_SEARCH_WIDE_H
#define ALORE_PATH_SEARCH_WIDE_H

#include "path_search.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace psearch {

constexpr int WIDE_MAX_CELLS = 1 << 22; // the largest window a reservation may ask for
constexpr int E_RANGE = -6;             // a reached cell's cost has a component that the packed word cannot order exactly
constexpr unsigned RANGE_LIMIT = 32767u;

// setup() with the cap as a parameter; the order of the statuses is unchanged
PS_HD Window setup_wide(const Grid& g, double sx, double sy, double gx, double gy, const Params& p, long long max_cells)
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
    if ((long long)w.wx * w.wy > max_cells) return w;
    const double ds = g.dist[(long)csx * g.ny + csy], dg = g.dist[(long)cgx * g.ny + cgy];
    double safe = max_of(min_of(p.safe_dis, 0.8 * ds), 0.0);
    safe = max_of(min_of(safe, 0.8 * dg), 0.0);
    w.safe = safe;
    w.status = (ds < safe || dg < safe) ? E_NO_PATH : OK;
    return w;
}

// ---- the tiling ---------------------------------------------------------------------------------------------------------------
struct Tiling {
    int ntx, nty; // tiles along x and y
};
struct Tile {
    int x0, y0, tw, th; // origin of the interior in the window and its size, 1 <= tw <= TX, 1 <= th <= TY
};
template <int TX, int TY>
PS_HD Tiling make_tiling(const Window& w)
{
    return Tiling{(w.wx + TX - 1) / TX, (w.wy + TY - 1) / TY};
}
template <int TX, int TY>
PS_HD Tile tile_at(const Window& w, const Tiling& tl, int t)
{
    const int tx = t / tl.nty, ty = t - tx * tl.nty;
    Tile r;
    r.x0 = tx * TX; r.y0 = ty * TY;
    r.tw = w.wx - r.x0 < TX ? w.wx - r.x0 : TX;
    r.th = w.wy - r.y0 < TY ? w.wy - r.y0 : TY;
    return r;
}
template <int TX, int TY>
PS_HD int tile_of_cell(const Tiling& tl, int x, int y)
{
    return (x / TX) * tl.nty + y / TY;
}
// words of the dirty bits for any window of at most max_cells cells.  ceil(wx / TX) ceil(wy / TY) <= wx wy / min(TX, TY) + 2: with
// one side below its tile size the other gives at most cells / T + 1 tiles; with both at or above, (wx / TX + 1)(wy / TY + 1) <=
// 3 cells / (TX TY) + 1, and 3 <= max(TX, TY)
template <int TX, int TY>
constexpr int dirty_words(long long max_cells)
{
    static_assert(TX >= 3 && TY >= 3, "dirty_words' bound");
    return (int)((max_cells / (TX < TY ? TX : TY) + 2 + 31) / 32);
}

// the word of window cell (x, y) as a tile sees it: BLOCKED outside the window
PS_HD unsigned slab_word(const unsigned* slab, const Window& w, int x, int y)
{
    return (x < 0 || y < 0 || x >= w.wx || y >= w.wy) ? BLOCKED : slab[x * w.wy + y];
}
// a word that may be extended: reached, and both components below RANGE_LIMIT (BLOCKED and UNREACHED have a = 65535)
PS_HD bool extendable(unsigned v) { return (v >> 16) < RANGE_LIMIT && (v & 0xFFFFu) < RANGE_LIMIT; }
// a reached word that sets the range flag
PS_HD bool out_of_range(unsigned v) { return v < UNREACHED && !extendable(v); }

// relax_cell on the cell at (lx, ly) of a tile array of row length `stride`, 1 <= lx, ly: every neighbour is in the array (the
// halo), and one that is not extendable is passed over.  true: the word went down
PS_HD bool relax_tile_cell(unsigned* tile, int stride, int lx, int ly)
{
    const int c = lx * stride + ly;
    const unsigned cur = tile[c];
    if (cur == BLOCKED) return false;
    unsigned best = cur;
    double kb = key(cur);
    for (int k = 0; k < 8; ++k) {
        const unsigned v = tile[c + dir_dx(k) * stride + dir_dy(k)];
        if (!extendable(v)) continue;
        const unsigned cand = v + dir_cost(k);
        const double kc = key(cand);
        if (kc < kb) { best = cand; kb = kc; }
    }
    if (best == cur) return false;
    tile[c] = best;
    return true;
}

// ---- the dirty bits and the order of the visits -------------------------------------------------------------------------------
PS_HD void dirty_set(unsigned* d, int t) { d[t >> 5] |= 1u << (t & 31); }
PS_HD void dirty_clear(unsigned* d, int t) { d[t >> 5] &= ~(1u << (t & 31)); }
PS_HD bool dirty_test(const unsigned* d, int t) { return (d[t >> 5] >> (t & 31)) & 1u; }
PS_HD void mark_neighbours(unsigned* d, const Tiling& tl, int t)
{
    const int tx = t / tl.nty, ty = t - tx * tl.nty;
    for (int k = 0; k < 8; ++k) {
        const int nx = tx + dir_dx(k), ny = ty + dir_dy(k);
        if (nx < 0 || ny < 0 || nx >= tl.ntx || ny >= tl.nty) continue;
        dirty_set(d, nx * tl.nty + ny);
    }
}
// the first dirty tile in [from, n), or n; the last dirty tile in [0, from], or -1.  Whole clean words are passed over
PS_HD int dirty_up(const unsigned* d, int from, int n)
{
    for (int t = from; t < n;) {
        if (!(d[t >> 5] >> (t & 31))) { t = (t | 31) + 1; continue; }
        if (dirty_test(d, t)) return t;
        ++t;
    }
    return n;
}
PS_HD int dirty_down(const unsigned* d, int from)
{
    for (int t = from; t >= 0;) {
        if (!(d[t >> 5] << (31 - (t & 31)))) { t = (t & ~31) - 1; continue; }
        if (dirty_test(d, t)) return t;
        --t;
    }
    return -1;
}
struct Cursor {
    int pos, dir; // the next tile to look at and the direction of the pass, +1 or -1
};
PS_HD Cursor cursor_begin() { return Cursor{0, 1}; }
// the next tile to visit, its bit cleared; -1 when the rest of this pass and a whole pass the other way found none
PS_HD int next_visit(unsigned* d, int n, Cursor& cu)
{
    for (int turned = 0; turned < 2; ++turned) {
        const int t = cu.dir > 0 ? dirty_up(d, cu.pos, n) : dirty_down(d, cu.pos);
        if (t >= 0 && t < n) {
            dirty_clear(d, t);
            cu.pos = t + cu.dir;
            return t;
        }
        cu.dir = -cu.dir;
        cu.pos = cu.dir > 0 ? 0 : n - 1;
    }
    return -1;
}

// ---- one visit, serially: tile[] holds (TX + 2) * (TY + 2) words.  true: a word changed (and the interior was stored) ----------
template <int TX, int TY>
inline bool visit_tile(unsigned* slab, const Window& w, const Tile& t, unsigned* tile)
{
    constexpr int S = TY + 2;
    for (int lx = 0; lx < t.tw + 2; ++lx)
        for (int ly = 0; ly < t.th + 2; ++ly) tile[lx * S + ly] = slab_word(slab, w, t.x0 + lx - 1, t.y0 + ly - 1);
    bool any = false;
    for (int sweep = 0;; ++sweep) {
        bool changed = false;
        if (sweep & 1) {
            for (int lx = t.tw; lx >= 1; --lx)
                for (int ly = t.th; ly >= 1; --ly) changed |= relax_tile_cell(tile, S, lx, ly);
        } else {
            for (int lx = 1; lx <= t.tw; ++lx)
                for (int ly = 1; ly <= t.th; ++ly) changed |= relax_tile_cell(tile, S, lx, ly);
        }
        if (!changed) break;
        any = true;
    }
    if (any)
        for (int lx = 1; lx <= t.tw; ++lx)
            for (int ly = 1; ly <= t.th; ++ly) slab[(t.x0 + lx - 1) * w.wy + (t.y0 + ly - 1)] = tile[lx * S + ly];
    return any;
}

// ---- one problem, serially, always by the tiled iteration (whatever the size of its window) -----------------------------------
// slab[] holds max_cells words (or the map's cells if fewer), tile[] (TX + 2)(TY + 2), dirty[] dirty_words<TX, TY>(max_cells),
// nodes[] MAX_NODES; *visits counts the visits of tiles
template <int TX, int TY>
inline int search_one_wide(const Grid& g, const double* sxy, const double* gxy, const Params& p, long long max_cells, unsigned* slab,
                           unsigned* tile, unsigned* dirty, int* nodes, int* n_points, double* xy, int* cost_ab, int* visits)
{
    *visits = 0;
    *n_points = 0;
    const Window w = setup_wide(g, sxy[0], sxy[1], gxy[0], gxy[1], p, max_cells);
    if (w.status != OK) return w.status;
    for (int x = 0; x < w.wx; ++x)
        for (int y = 0; y < w.wy; ++y) slab[x * w.wy + y] = first_word(g, w, x, y);
    const Tiling tl = make_tiling<TX, TY>(w);
    const int n_tiles = tl.ntx * tl.nty;
    for (int i = 0; i < (n_tiles + 31) / 32; ++i) dirty[i] = 0u;
    dirty_set(dirty, tile_of_cell<TX, TY>(tl, w.gx, w.gy));
    Cursor cu = cursor_begin();
    for (int t; (t = next_visit(dirty, n_tiles, cu)) >= 0;) {
        ++*visits;
        if (visit_tile<TX, TY>(slab, w, tile_at<TX, TY>(w, tl, t), tile)) mark_neighbours(dirty, tl, t);
    }
    bool range = false;
    for (int c = 0; c < w.wx * w.wy; ++c) range |= out_of_range(slab[c]);
    if (range) return E_RANGE;
    return finish(g, w, slab, nodes, sxy, gxy, n_points, xy, cost_ab);
}

} // namespace psearch

#endif
