// path_search_wide.hip -- the grid search on windows that do not fit in LDS (alore_backend_search_reserve, then
// alore_backend_search_paths); arithmetic, the tiling's argument and the range rule in path_search_wide.h.
// `slots` workgroups of 1024 threads run behind search_paths_kernel on the same stream.  Workgroup j owns slab j of the
// reservation and takes the slots b = j, j + slots, ... of the call in turn; it searches the ones that the first kernel left at
// E_WINDOW and whose window fits the slab, and skips every other (masked out, solved, failed).  A slot's field lies in the slab,
// one word per cell, every word of the window initialised first, so a slab that served another slot leaks nothing.
//
// A VISIT of a tile: all threads load the tile and its halo into LDS (rows of the slab along y are contiguous: coalesced), then
// relax the interior by the gather sweeps of path_search.hip -- a thread owns a run of `chunk` consecutive interior cells, chunk
// odd, which spreads a wavefront over the LDS banks; halo words are read and never written -- until a sweep changes no word
// (a workgroup-wide OR at a barrier), then store the interior if the first sweep changed one.  Thread 0 keeps the dirty bits (LDS)
// and picks the next tile: one writer, no atomics.  No workgroup waits for another or reads what another wrote: a slab has one
// owner, and __syncthreads() orders its stores and loads within the workgroup.
// THE WALK AND THE PRUNING: thread 0 runs psearch::finish on the slab, the raw nodes in a 4 KiB LDS list; a chain of dependent
// loads from device memory (profiles/path_search_wide.txt has its share of a search).
// LDS: (126 + 2)^2 words of tile, 4 KiB of nodes, the dirty bits of the largest window (4164 bytes): 72 KiB.  Two workgroups would
// fit in a CU's LDS; the 91 registers allow one (bounded to 64 the compiler spills, which was not taken).
#include "backend_kernels.h"
#include "path_search_wide.h"
#include "wide_visit.h"

namespace backend {

namespace ps = psearch;

extern __shared__ __align__(16) unsigned wide_lds[];

__global__ __launch_bounds__(WIDE_THREADS) void search_paths_wide_kernel(const SearchArgs* __restrict__ gp)
{
    const SearchArgs& a = *gp;
    const int tid = threadIdx.x;
    unsigned* tile = wide_lds;
    int* nodes = (int*)(wide_lds + WIDE_TILE_WORDS);
    unsigned* dirty = wide_lds + WIDE_TILE_WORDS + ps::MAX_NODES;
    int* next = (int*)(dirty + WIDE_DIRTY_WORDS);
    unsigned* slab = a.wide_slabs + (size_t)blockIdx.x * a.wide_cells;
    const long long cap = a.wide_cells < ps::WIDE_MAX_CELLS ? a.wide_cells : ps::WIDE_MAX_CELLS;
    const ps::Grid g = ps::make_grid(a.map.dist, a.map.nx, a.map.ny, a.map.x_lo, a.map.y_lo, a.map.x_hi, a.map.y_hi, a.map.res);
    const ps::Params prm{a.safe_dis, a.window_margin};
    for (int b = blockIdx.x; b < a.count; b += a.wide_slots) {
        if (a.status[b] != ps::E_WINDOW) continue; // the same in every thread, as every branch up to the first barrier
        const double* sp = (const double*)((const char*)a.start + (size_t)b * a.start_stride);
        const double* gl = (const double*)((const char*)a.goal + (size_t)b * a.goal_stride);
        const double sxy[2] = {sp[0], sp[1]}, gxy[2] = {gl[0], gl[1]};
        const ps::Window w = ps::setup_wide(g, sxy[0], sxy[1], gxy[0], gxy[1], prm, cap);
        if (w.status == ps::E_WINDOW) continue;    // more than the reservation: as the first kernel left it
        if (w.status != ps::OK) {                  // an end cell that is not free; n_points and sweeps are 0 already
            if (tid == 0) a.status[b] = w.status;
            continue;
        }
        const long long t_begin = wall_clock64();
        const int cells = w.wx * w.wy;
        for (int c = tid; c < cells; c += WIDE_THREADS) {
            const int x = c / w.wy;
            slab[c] = ps::first_word(g, w, x, c - x * w.wy);
        }
        const ps::Tiling tl = ps::make_tiling<WTX, WTY>(w);
        const int n_tiles = tl.ntx * tl.nty;
        for (int i = tid; i < (n_tiles + 31) / 32; i += WIDE_THREADS) dirty[i] = 0u;
        __syncthreads();
        ps::Cursor cu = ps::cursor_begin();
        int visits = 0;
        if (tid == 0) ps::dirty_set(dirty, ps::tile_of_cell<WTX, WTY>(tl, w.gx, w.gy));
        for (;;) {
            if (tid == 0) *next = ps::next_visit(dirty, n_tiles, cu);
            __syncthreads();
            const int t = *next;
            if (t < 0) break;
            ++visits;
            const ps::Tile tt = ps::tile_at<WTX, WTY>(w, tl, t);
            if (wide_visit(slab, w, tt, tile, tid) && tid == 0) ps::mark_neighbours(dirty, tl, t); // a sweep changed a word
            __syncthreads(); // the stores before the next loads, and *next and the tile array are free again
        }
        int range = 0;
        for (int c = tid; c < cells; c += WIDE_THREADS) range |= (int)ps::out_of_range(slab[c]);
        range = __syncthreads_or(range);
        if (tid == 0) {
            int n_points = 0, cost[2], st = ps::E_RANGE;
            const long long t_field = wall_clock64();
            if (!range) st = ps::finish(g, w, slab, nodes, sxy, gxy, &n_points, a.xy + (size_t)b * ps::MAX_POINTS * 2, cost);
            const long long t_end = wall_clock64();
            a.wide_ticks[2 * (size_t)b] = t_end - t_begin;
            a.wide_ticks[2 * (size_t)b + 1] = t_end - t_field;
            a.status[b] = st;
            a.n_points[b] = n_points;
            a.sweeps[b] = visits;
            if (st == ps::OK) {
                a.cost_ab[2 * (size_t)b] = cost[0];
                a.cost_ab[2 * (size_t)b + 1] = cost[1];
            }
        }
        __syncthreads(); // thread 0 has read the slab and the nodes before the next slot overwrites them
    }
}

constexpr size_t WIDE_LDS_BYTES = (sizeof(unsigned) * (WIDE_TILE_WORDS + ps::MAX_NODES + WIDE_DIRTY_WORDS + 1) + 15) & ~size_t(15);

hipError_t search_wide_configure()
{
    return hipFuncSetAttribute((const void*)search_paths_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)WIDE_LDS_BYTES);
}

hipError_t search_paths_wide(const SearchArgs* d_args, int slots, hipStream_t s)
{
    void* args[] = {&d_args};
    hipError_t e = hipLaunchKernel((const void*)search_paths_wide_kernel, dim3(slots), dim3(WIDE_THREADS), args, WIDE_LDS_BYTES, s);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

} // namespace backend
