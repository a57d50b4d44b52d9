// path_search.hip -- way-point paths by grid search on the device map (alore_backend_search_paths); arithmetic in path_search.h.
// One workgroup of 1024 threads per problem, the cost-to-goal field of the search window in LDS, one word per cell.
//
// THE FIELD is found by label-correcting sweeps in gather form.  A thread owns a run of `chunk` consecutive window cells and
// relaxes them in turn, forwards in even sweeps and backwards in odd ones: it reads the eight neighbours of a cell and writes
// only that cell, so every word has one writer and there are no atomics.  A neighbour's word may be stale; that is harmless,
// because a word only ever goes down, and to the cost of a real path: the fixed point is the exact field whatever the
// interleaving.  A sweep that changes no word anywhere (a workgroup-wide OR at a barrier) ran on words that stood still, so
// every cell has been verified against final neighbours: the field is the fixed point.  Within a sweep a thread's own run is
// Gauss-Seidel (news travels the length of the run, i.e. along y), across runs news moves about one cell per sweep.
// chunk is odd: lane t reads word t * chunk + offset, an odd stride in dwords, which spreads a wavefront's 64 lanes over the
// 64 banks.
// THE WALK AND THE PRUNING are short sequential chains; thread 0 runs them (psearch::finish) on the field in LDS, the raw
// nodes in a 4 KiB LDS list.
// LDS: 4 bytes per cell of the largest window the map allows, min(nx ny, 32768) (the host knows the map, not the problems), plus
// 4 KiB: up to 132 KiB, one workgroup per CU then.  1024 threads keep all four SIMDs of that CU at four wavefronts each.
#include "backend_kernels.h"
#include "path_search.h"

namespace backend {

namespace ps = psearch;

constexpr int SEARCH_THREADS = 1024;

extern __shared__ __align__(16) unsigned search_lds[];

__global__ __launch_bounds__(SEARCH_THREADS) void search_paths_kernel(const SearchArgs* __restrict__ gp)
{
    const SearchArgs& a = *gp;
    const int b = blockIdx.x, tid = threadIdx.x;
    // a masked-out workgroup leaves before any LDS access or barrier; only its status word is written
    if (a.mask && *(const int*)((const char*)a.mask + (size_t)b * a.mask_stride) == 0) {
        if (tid == 0) a.status[b] = ps::MASKED;
        return;
    }
    const double* sp = (const double*)((const char*)a.start + (size_t)b * a.start_stride);
    const double* gl = (const double*)((const char*)a.goal + (size_t)b * a.goal_stride);
    const double sxy[2] = {sp[0], sp[1]}, gxy[2] = {gl[0], gl[1]};
    const ps::Grid g = ps::make_grid(a.map.dist, a.map.nx, a.map.ny, a.map.x_lo, a.map.y_lo, a.map.x_hi, a.map.y_hi, a.map.res);
    const ps::Params prm{a.safe_dis, a.window_margin};
    ps::Window w = ps::setup(g, sxy[0], sxy[1], gxy[0], gxy[1], prm); // the same in every thread
    const int cells = w.wx * w.wy;
    if (w.status == ps::OK && cells > a.lds_cells) w.status = ps::E_WINDOW; // cannot happen: a window is clipped to the map
    if (w.status != ps::OK) {
        if (tid == 0) {
            a.status[b] = w.status;
            a.n_points[b] = 0;
            a.sweeps[b] = 0;
        }
        return;
    }
    unsigned* words = search_lds;
    int* nodes = (int*)(search_lds + a.lds_cells);
    for (int c = tid; c < cells; c += SEARCH_THREADS) {
        const int x = c / w.wy;
        words[c] = ps::first_word(g, w, x, c - x * w.wy);
    }
    __syncthreads();
    const int chunk = ((cells + SEARCH_THREADS - 1) / SEARCH_THREADS) | 1;
    const int lo = min(tid * chunk, cells), hi = min(lo + chunk, cells);
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
    if (tid == 0) {
        int n_points = 0, cost[2];
        double* xy = a.xy + (size_t)b * ps::MAX_POINTS * 2;
        const int st = ps::finish(g, w, words, nodes, sxy, gxy, &n_points, xy, cost);
        a.status[b] = st;
        a.n_points[b] = n_points;
        a.sweeps[b] = sweeps;
        if (st == ps::OK) {
            a.cost_ab[2 * (size_t)b] = cost[0];
            a.cost_ab[2 * (size_t)b + 1] = cost[1];
        }
    }
}

static size_t search_lds_bytes(int lds_cells) { return sizeof(unsigned) * (size_t)lds_cells + sizeof(int) * ps::MAX_NODES; }

hipError_t search_configure()
{
    return hipFuncSetAttribute((const void*)search_paths_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)search_lds_bytes(ps::MAX_CELLS));
}

hipError_t search_paths(const SearchArgs* d_args, int count, int lds_cells, hipStream_t s)
{
    void* args[] = {&d_args};
    hipError_t e = hipLaunchKernel((const void*)search_paths_kernel, dim3(count), dim3(SEARCH_THREADS), args, search_lds_bytes(lds_cells), s);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

} // namespace backend
