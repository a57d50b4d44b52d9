// wide_visit.h -- one visit of a tile by a workgroup of 1024 threads, the device code that search_paths_wide_kernel
// (path_search_wide.hip) and task_costs_wide_kernel (task_plan.hip) both run (internal).  The arithmetic is path_search_wide.h's.
#pragma once

#include <hip/hip_runtime.h>

#include "path_search_wide.h"

namespace backend {

constexpr int WIDE_THREADS = 1024;
constexpr int WTX = 126, WTY = 126;                   // interior cells of a tile
constexpr int WS = WTY + 2;                           // row length of the tile array
constexpr int WIDE_TILE_WORDS = (WTX + 2) * WS;
constexpr int WIDE_DIRTY_WORDS = psearch::dirty_words<WTX, WTY>(psearch::WIDE_MAX_CELLS);
static_assert(WS == 128 && WIDE_TILE_WORDS % WIDE_THREADS == 0, "the load and store loops address the tile array by i >> 7, i & 127");

// All threads of the workgroup call it with the same arguments, behind a barrier that orders the slab's last stores.  Loads the
// tile and its halo into tile[] (rows of the slab along y are contiguous: coalesced), relaxes the interior by gather sweeps -- a
// thread owns a run of `chunk` consecutive interior cells, chunk odd, which spreads a wavefront over the LDS banks; halo words are
// read and never written -- until a sweep changes no word (a workgroup-wide OR at a barrier), and stores the interior if the first
// sweep changed one.  true (in every thread): it did.  The caller's barrier orders the stores before the next loads
__device__ inline bool wide_visit(unsigned* slab, const psearch::Window& w, const psearch::Tile& tt, unsigned* tile, int tid)
{
    namespace ps = psearch;
    for (int i = tid; i < WIDE_TILE_WORDS; i += WIDE_THREADS) {
        const int lx = i >> 7, ly = i & 127;
        if (lx < tt.tw + 2 && ly < tt.th + 2) tile[i] = ps::slab_word(slab, w, tt.x0 + lx - 1, tt.y0 + ly - 1);
    }
    __syncthreads();
    const int n = tt.tw * tt.th;
    const int chunk = ((n + WIDE_THREADS - 1) / WIDE_THREADS) | 1;
    const int lo = min(tid * chunk, n), hi = min(lo + chunk, n);
    int sweeps = 0;
    for (;;) {
        int changed = 0;
        if (lo < hi) {
            if (sweeps & 1) {
                int x = (hi - 1) / tt.th, y = (hi - 1) - x * tt.th;
                for (int c = hi - 1; c >= lo; --c) {
                    changed |= (int)ps::relax_tile_cell(tile, WS, x + 1, y + 1);
                    if (--y < 0) { y = tt.th - 1; --x; }
                }
            } else {
                int x = lo / tt.th, y = lo - x * tt.th;
                for (int c = lo; c < hi; ++c) {
                    changed |= (int)ps::relax_tile_cell(tile, WS, x + 1, y + 1);
                    if (++y == tt.th) { y = 0; ++x; }
                }
            }
        }
        ++sweeps;
        if (!__syncthreads_or(changed)) break;
    }
    if (sweeps <= 1) return false;
    for (int i = tid; i < WIDE_TILE_WORDS; i += WIDE_THREADS) {
        const int lx = i >> 7, ly = i & 127;
        if (lx >= 1 && lx <= tt.tw && ly >= 1 && ly <= tt.th) slab[(tt.x0 + lx - 1) * w.wy + (tt.y0 + ly - 1)] = tile[i];
    }
    return true;
}

} // namespace backend
