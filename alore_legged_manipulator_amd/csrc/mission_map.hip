// mission_map.hip -- the kernels behind alore_backend_map_paint and alore_backend_mission_* (arithmetic and contract: mission_map.h).
//
// PAINTING.  Two passes per launch of as many edits as the handle has descriptors, no atomics on cells, no LDS:
//   mission_paint_axes_kernel   one lane per (edit, axis) walks the accumulated lattice (at most 64 dependent adds) and leaves the
//                               axis' half of the edit's descriptor: first and last cell, the 64-bit mask of covered offsets;
//   mission_paint_cells_kernel  one wavefront per edit, lane l on offset l of the y mask.  "As if one after the other" means the LAST
//                               edit that covers a cell decides it: the wavefront runs over the later descriptors of the launch -- a
//                               wavefront-uniform loop, the descriptors come in through scalar loads, a bounding-box reject first --
//                               and every lane clears, in its copy of the x mask, the columns a later edit covers in its row.  What
//                               is left is written, so every cell has at most one writer in a launch.  The writer compares with the
//                               old state; the wavefront adds its changes with one atomicAdd and widens the box with atomicMin /
//                               atomicMax, all from lane 0.
// MISSIONS.  mission_set_kernel and mission_goals_kernel, one lane per mission, write the slab; mission_edits_kernel, ONE workgroup,
// walks the slots in order 256 at a time, scans the edit counts of its lanes in LDS and appends every lane's edits behind a running
// offset: the list is compacted in slot order, its length is left on the device, and the paint kernels read both in stream order.
#include "mission_map.h"

namespace mission {
namespace {

__device__ inline int list_length(const int* d_count, int limit)
{
    if (!d_count) return limit;
    const int n = *d_count;
    return n < 0 ? 0 : (n > limit ? limit : n);
}
__device__ inline bool selected(const int* mask, int stride, int m) { return !mask || *(const int*)((const char*)mask + (size_t)m * stride) != 0; }

__global__ void mission_paint_begin_kernel(int* counters, int nx, int ny)
{
    if (threadIdx.x < 8) {
        const Counters c = no_change(nx, ny);
        const int v[8] = {c.n_changed, c.min_x, c.min_y, c.max_x, c.max_y, c.n_skipped, 0, 0};
        counters[threadIdx.x] = v[threadIdx.x];
    }
}

__global__ void __launch_bounds__(256) mission_paint_axes_kernel(occ::Geom g, const Edit* edits, const int* d_count, int limit, int base,
                                                                  int chunk, Desc* desc, int* counters)
{
    const int n = list_length(d_count, limit);
    const int end = n < base + chunk ? n : base + chunk;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = base + (t >> 1);
    if (e >= end) return;
    const Edit ed = edits[e];
    const bool valid = edit_valid(ed, g.res);
    Desc& d = desc[e - base];
    if ((t & 1) == 0) {
        const Axis a = valid ? axis_x(g, ed) : Axis{0, -1, 0ull};
        d.x0 = a.first; d.x1 = a.last; d.mx = a.mask;
        d.value = valid ? (int)edit_state(ed) : 0;
        d.pad = 0;
        if (!valid) atomicAdd(&counters[5], 1);
    } else {
        const Axis a = valid ? axis_y(g, ed) : Axis{0, -1, 0ull};
        d.y0 = a.first; d.y1 = a.last; d.my = a.mask;
    }
}

__global__ void __launch_bounds__(256) mission_paint_cells_kernel(occ::Geom g, unsigned char* grid, const int* d_count, int limit, int base,
                                                                   int chunk, const Desc* desc, int* counters)
{
    const int n = list_length(d_count, limit);
    const int end = (n < base + chunk ? n : base + chunk) - base; // descriptors of this launch
    const int e = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (e >= end) return;
    const int lane = threadIdx.x & 63;
    const Desc d = desc[e];
    if (d.value == 0 || d.mx == 0ull || d.my == 0ull) return;
    const int y = d.y0 + lane;
    const bool mine = (d.my >> lane) & 1ull;
    unsigned long long live = d.mx;
    for (int j = e + 1; j < end; ++j) {
        const Desc& o = desc[j];
        const int ox0 = o.x0, ox1 = o.x1, oy0 = o.y0, oy1 = o.y1;
        if (o.value == 0 || ox1 < d.x0 || ox0 > d.x1 || oy1 < d.y0 || oy0 > d.y1) continue; // an axis without cells has last = -1
        const int shift = ox0 - d.x0; // |shift| <= 63: the boxes overlap and each spans at most 64 cells
        const unsigned long long cols = shift >= 0 ? o.mx << shift : o.mx >> -shift;
        const int dy = y - oy0;
        if (dy >= 0 && dy < 64 && ((o.my >> dy) & 1ull)) live &= ~cols;
    }
    const unsigned char value = (unsigned char)d.value;
    int changed = 0, min_x = g.nx, max_x = -1, min_y = g.ny, max_y = -1;
    for (unsigned long long rem = d.mx; rem != 0ull; rem &= rem - 1ull) {
        const int k = __builtin_ctzll(rem);
        const int x = d.x0 + k;
        bool wrote = false;
        if (mine && ((live >> k) & 1ull)) {
            unsigned char* c = grid + (size_t)x * g.ny + y; // x <= x1 <= nx - 1 and y <= y1 <= ny - 1 (axis_cells clamps)
            if (*c != value) { *c = value; wrote = true; }
        }
        const unsigned long long b = __ballot(wrote);
        if (b != 0ull) {
            changed += __popcll(b);
            if (x < min_x) min_x = x;
            if (x > max_x) max_x = x;
            const int lo = d.y0 + __builtin_ctzll(b), hi = d.y0 + 63 - __builtin_clzll(b);
            if (lo < min_y) min_y = lo;
            if (hi > max_y) max_y = hi;
        }
    }
    if (lane == 0 && changed) {
        atomicAdd(&counters[0], changed);
        atomicMin(&counters[1], min_x);
        atomicMin(&counters[2], min_y);
        atomicMax(&counters[3], max_x);
        atomicMax(&counters[4], max_y);
    }
}

__global__ void __launch_bounds__(256) mission_set_kernel(Slab s, int count, int max_tasks, const int* n_tasks, const double* points,
                                                           int row_stride, const int* kinds, const int* mask, int mask_stride, int* was_set)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= count) return;
    const bool sel = selected(mask, mask_stride, m);
    was_set[m] = sel;
    if (!sel) return;
    set_one(s, m, max_tasks, n_tasks[m], (const double*)((const char*)points + (size_t)m * row_stride), kinds ? kinds + (size_t)m * max_tasks : nullptr);
}

__global__ void __launch_bounds__(256) mission_goals_kernel(Slab s, int count, const double* goals, int goal_stride, const int* mask, int mask_stride)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= count || !selected(mask, mask_stride, m)) return;
    const double* g = (const double*)((const char*)goals + (size_t)m * goal_stride);
    goals_one(s, m, g[0], g[1]);
}

__global__ void __launch_bounds__(256) mission_edits_kernel(Slab s, Params P, int count, const int* was_set, const double* poses, int pose_stride,
                                                             const int* after_plan, int after_stride, Edit* out, int* out_count)
{
    __shared__ int scan[256];
    const int t = threadIdx.x;
    int running = 0;
    for (int first = 0; first < count; first += 256) {
        const int m = first + t;
        int c = 0;
        Fired f{0, -1};
        if (m < count) {
            if (!poses) c = was_set[m] && s.status[m] == OK ? s.n[m] : 0;
            else {
                const double* p = (const double*)((const char*)poses + (size_t)m * pose_stride);
                f = step_rules(s, P, m, p[0], p[1], after_plan && selected(after_plan, after_stride, m));
                c = fired_count(f);
            }
        }
        scan[t] = c;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) { // inclusive scan of the 256 counts
            const int v = t >= d ? scan[t - d] : 0;
            __syncthreads();
            scan[t] += v;
            __syncthreads();
        }
        const int at = running + scan[t] - c;
        running += scan[255];
        __syncthreads();
        if (!poses) {
            for (int i = 0; i < c; ++i) out[at + i] = item_edit(s, P, m, i);
        } else {
            if (f.first != 0) out[at] = first_edit(s, P, m, f.first);
            if (f.left >= 0) out[at + (f.first != 0 ? 1 : 0)] = left_edit(s, P, m, f.left);
        }
    }
    if (t == 0) *out_count = running;
}

} // namespace

hipError_t paint_enqueue(const occ::Geom& g, unsigned char* grid, const Edit* d_edits, const int* d_count, int limit, Desc* d_desc,
                         int desc_capacity, int* d_counters, hipStream_t s)
{
    hipLaunchKernelGGL(mission_paint_begin_kernel, dim3(1), dim3(64), 0, s, d_counters, g.nx, g.ny);
    for (int base = 0; base < limit; base += desc_capacity) {
        const int here = limit - base < desc_capacity ? limit - base : desc_capacity;
        hipLaunchKernelGGL(mission_paint_axes_kernel, dim3((2 * here + 255) / 256), dim3(256), 0, s, g, d_edits, d_count, limit, base, desc_capacity, d_desc,
                           d_counters);
        hipLaunchKernelGGL(mission_paint_cells_kernel, dim3((here + 3) / 4), dim3(256), 0, s, g, grid, d_count, limit, base, desc_capacity,
                           (const Desc*)d_desc, d_counters);
    }
    return hipGetLastError();
}

hipError_t set_enqueue(const Slab& s, int count, int max_tasks, const int* n_tasks, const double* points, int row_stride, const int* kinds,
                       const int* mask, int mask_stride, int* was_set, hipStream_t st)
{
    hipLaunchKernelGGL(mission_set_kernel, dim3((count + 255) / 256), dim3(256), 0, st, s, count, max_tasks, n_tasks, points, row_stride, kinds, mask,
                       mask_stride, was_set);
    return hipGetLastError();
}

hipError_t goals_enqueue(const Slab& s, int count, const double* goals, int goal_stride, const int* mask, int mask_stride, hipStream_t st)
{
    hipLaunchKernelGGL(mission_goals_kernel, dim3((count + 255) / 256), dim3(256), 0, st, s, count, goals, goal_stride, mask, mask_stride);
    return hipGetLastError();
}

hipError_t edits_enqueue(const Slab& s, const Params& P, int count, const int* was_set, const double* poses, int pose_stride,
                         const int* after_plan, int after_stride, Edit* out, int* out_count, hipStream_t st)
{
    hipLaunchKernelGGL(mission_edits_kernel, dim3(1), dim3(256), 0, st, s, P, count, was_set, poses, pose_stride, after_plan, after_stride, out, out_count);
    return hipGetLastError();
}

} // namespace mission
