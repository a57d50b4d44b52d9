// occupancy_map.hip -- point clouds into the resident occupancy map on the device (gfx950): what alore_backend_map_integrate
// launches per scan, the arithmetic of occupancy_update.h (one updateOccupancyCallback of plan_env::SDFmap per scan).
//
// Raycast mode, three launches:
//   occ_ray_kernel     one lane per point: the end-point rule, then the Bresenham walk from the sensor's cell.  Every visited cell
//                      gets an integer atomic add on count_all, the end cell of a hit one on count_hit as well; integer adds
//                      commute, so the counts do not depend on arrival order.  All rays start in the sensor's cell and the first
//                      steps of a wavefront land on a handful of addresses: the lanes whose cell equals that of the first active
//                      lane are added as ONE atomic of their population count, the others singly (wave_add).
//   occ_cells_kernel   one lane per cell of the box (and one cell round it, see occ::pass_box): the log-odds update of a cell with
//                      a count, which zeroes both counts, and the lattice pass of RemoveOutliers on the state grid of the previous
//                      cycle, in place (occupancy_update.h says why in place is the reference's sequential scan).
//   occ_state_kernel   the same cells: the 3 x 3 fill round the sensor, which must not run before the whole lattice pass has ended,
//                      then the state rule from the new log-odds.
// Perspective mode, two launches: occ_window_kernel (Unknown -> Unoccupied in the box) and occ_points_kernel (the cell of every
// point inside the map becomes Occupied: no range clip, idempotent writes).
// The kernels read their arguments from a device block that the caller fills in stream order: ScanArgs, then the marks of the
// lattice's columns and rows, which the host computes from the pose by the reference's sequential additions (occ::lattice_row).
// No LDS, no scratch, no barrier.  Every index is a clamped cell index (occ::cell_1d) or lies inside the box, which lies inside the map.
#include <cstring>

#include "backend_kernels.h"
#include "occupancy_update.h"

namespace backend {

struct ScanArgs {
    occ::Geom g;
    occ::LogOdds L;
    double ox, oy, range; // the sensor position and the detection range
    occ::Window w;        // the window and its box of cells
    occ::Box box;         // the cells the passes run over
    int sx, sy;           // the sensor's cell
    const char* points;   // float pairs, `stride` bytes apart
    int n_points, stride;
    unsigned char* grid;
    double* log_odds;
    int *count_hit, *count_all;
    const unsigned char *mark_x, *mark_y; // [nx], [ny]: columns and rows the lattice of RemoveOutliers visits
    int perspective;
};

namespace {

constexpr int THREADS = 256;

__device__ __forceinline__ void load_point(const ScanArgs& a, int i, double* x, double* y)
{
    const float* p = (const float*)(a.points + (size_t)i * a.stride);
    *x = (double)p[0];
    *y = (double)p[1];
}

// counts[cell] += 1 for every lane with `on`.  Every lane of the wavefront reaches the call (the call sites are wave-uniform), but
// readfirstlane and the ballot sit inside the divergent `if (on)`: both act on the ACTIVE lanes only, which is what makes `first`
// the cell of the first lane that is on and `group` a set of lanes that are on
__device__ __forceinline__ void wave_add(int* counts, int cell, bool on)
{
    if (on) {
        const int first = __builtin_amdgcn_readfirstlane(cell); // the cell of the first lane that is on
        const bool same = cell == first;
        const unsigned long long group = __ballot(same);
        if (same) {
            if ((int)(threadIdx.x & 63) == __ffsll((long long)group) - 1) atomicAdd(counts + first, __popcll(group));
        } else {
            atomicAdd(counts + cell, 1);
        }
    }
}

} // namespace

__global__ __launch_bounds__(THREADS) void occ_ray_kernel(const ScanArgs* __restrict__ gp)
{
    const ScanArgs& a = *gp;
    const occ::Geom g = a.g;
    const int i = blockIdx.x * THREADS + threadIdx.x;
    bool valid = i < a.n_points;
    double px = 0.0, py = 0.0, ex = 0.0, ey = 0.0;
    if (valid) load_point(a, i, &px, &py);
    valid = valid && occ::finite_point(px, py);
    bool hit = false;
    if (valid) hit = occ::ray_end(g, a.ox, a.oy, a.range, px, py, &ex, &ey);
    const int cx = valid ? occ::cell_x(g, ex) : a.sx, cy = valid ? occ::cell_y(g, ey) : a.sy;
    wave_add(a.count_all, cx * g.ny + cy, valid);
    wave_add(a.count_hit, cx * g.ny + cy, valid && hit);
    occ::Line l = occ::line_begin(a.sx, a.sy, cx, cy);
    bool walking = valid && !occ::line_at_end(l);
    // a line has at most nx + ny cells: the bound only keeps a corrupted block of arguments from spinning
    for (int step = 0; step < g.nx + g.ny && __ballot(walking) != 0ull; ++step) {
        wave_add(a.count_all, l.x * g.ny + l.y, walking);
        if (walking) {
            occ::line_step(l);
            walking = !occ::line_at_end(l);
        }
    }
}

__global__ __launch_bounds__(THREADS) void occ_cells_kernel(const ScanArgs* __restrict__ gp)
{
    const ScanArgs& a = *gp;
    const int h = a.box.y1 - a.box.y0 + 1, w = a.box.x1 - a.box.x0 + 1;
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= w * h) return;
    const int x = a.box.x0 + t / h, y = a.box.y0 + t % h;
    const size_t c = (size_t)x * a.g.ny + y;
    const int total = a.count_all[c];
    if (total != 0) {
        a.log_odds[c] = occ::logodds_update(a.L, a.log_odds[c], a.count_hit[c], total, occ::in_box(a.w, x, y));
        a.count_all[c] = 0;
        a.count_hit[c] = 0;
    }
    if (a.mark_x[x] && a.mark_y[y] && occ::outlier_fills(a.grid, a.g.nx, a.g.ny, x, y)) a.grid[c] = occ::UNOCCUPIED;
}

__global__ __launch_bounds__(THREADS) void occ_state_kernel(const ScanArgs* __restrict__ gp)
{
    const ScanArgs& a = *gp;
    const int h = a.box.y1 - a.box.y0 + 1, w = a.box.x1 - a.box.x0 + 1;
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= w * h) return;
    const int x = a.box.x0 + t / h, y = a.box.y0 + t % h;
    const size_t c = (size_t)x * a.g.ny + y;
    const unsigned char before = a.grid[c], after = occ::fill_and_state(a.L, a.w, a.sx, a.sy, x, y, before, a.log_odds[c]);
    if (after != before) a.grid[c] = after;
}

__global__ __launch_bounds__(THREADS) void occ_window_kernel(const ScanArgs* __restrict__ gp)
{
    const ScanArgs& a = *gp;
    const int h = a.w.max_y - a.w.min_y + 1, w = a.w.max_x - a.w.min_x + 1;
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= w * h) return;
    const size_t c = (size_t)(a.w.min_x + t / h) * a.g.ny + a.w.min_y + t % h;
    if (a.grid[c] == occ::UNKNOWN) a.grid[c] = occ::UNOCCUPIED;
}

__global__ __launch_bounds__(THREADS) void occ_points_kernel(const ScanArgs* __restrict__ gp)
{
    const ScanArgs& a = *gp;
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.n_points) return;
    double px, py;
    load_point(a, i, &px, &py);
    if (!occ::in_map(a.g, px, py)) return; // a NaN fails every comparison
    a.grid[(size_t)occ::cell_x(a.g, px) * a.g.ny + occ::cell_y(a.g, py)] = occ::OCCUPIED;
}

__global__ void occ_fill_kernel(double* p, size_t n, double v)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) p[t] = v;
}

// ---- host ---------------------------------------------------------------------------------------------------------------
void occ_log_odds(const alore_backend_map_params& p, double out[5])
{
    out[0] = occ::logit(p.p_hit); out[1] = occ::logit(p.p_miss); out[2] = occ::logit(p.p_min); out[3] = occ::logit(p.p_max);
    out[4] = occ::logit(p.p_occ);
}

size_t occ_block_bytes(int nx, int ny) { return ((sizeof(ScanArgs) + 15) & ~size_t(15)) + (((size_t)nx + ny + 15) & ~size_t(15)); }

bool occ_prepare_scan(const OccMap& m, double ox, double oy, const char* d_points, int n_points, int stride, char* h_block, const char* d_block)
{
    const occ::Geom g = occ::make_geom(m.nx, m.ny, m.x_lo, m.y_lo, m.res);
    if (!occ::sensor_inside(g, ox, oy)) return false;
    ScanArgs a{};
    a.g = g;
    a.L = occ::LogOdds{m.log_odds5[0], m.log_odds5[1], m.log_odds5[2], m.log_odds5[3], m.log_odds5[4]};
    a.ox = ox; a.oy = oy; a.range = m.range;
    a.w = occ::window(g, ox, oy, m.range);
    a.box = occ::pass_box(g, a.w);
    a.sx = occ::cell_x(g, ox); a.sy = occ::cell_y(g, oy);
    a.points = d_points; a.n_points = n_points; a.stride = stride;
    a.grid = m.grid; a.log_odds = m.log_odds; a.count_hit = m.count_hit; a.count_all = m.count_all;
    const size_t marks = (sizeof(ScanArgs) + 15) & ~size_t(15);
    a.mark_x = (const unsigned char*)d_block + marks;
    a.mark_y = a.mark_x + m.nx;
    a.perspective = m.perspective;
    std::memcpy(h_block, &a, sizeof(a));
    if (!m.perspective) {
        unsigned char* mk = (unsigned char*)h_block + marks;
        const int cap = occ::lattice_cap(m.range, m.res);
        occ::lattice_marks(m.h_row, occ::lattice_row(ox, m.range, m.res, m.h_row, cap), g.x_lo, g.x_hi, g.res, g.inv, g.nx, mk);
        occ::lattice_marks(m.h_row, occ::lattice_row(oy, m.range, m.res, m.h_row, cap), g.y_lo, g.y_hi, g.res, g.inv, g.ny, mk + m.nx);
    }
    return true;
}

hipError_t occ_enqueue_scan(const char* h_block, const char* d_block, hipStream_t s)
{
    ScanArgs a;
    std::memcpy(&a, h_block, sizeof(a));
    const ScanArgs* d = (const ScanArgs*)d_block;
    void* args[] = {&d};
    const unsigned point_blocks = (unsigned)((a.n_points + THREADS - 1) / THREADS);
    hipError_t e = hipSuccess;
    if (a.perspective) {
        const long cells = (long)(a.w.max_x - a.w.min_x + 1) * (a.w.max_y - a.w.min_y + 1);
        e = hipLaunchKernel((const void*)occ_window_kernel, dim3((unsigned)((cells + THREADS - 1) / THREADS)), dim3(THREADS), args, 0, s);
        if (e == hipSuccess && point_blocks) e = hipLaunchKernel((const void*)occ_points_kernel, dim3(point_blocks), dim3(THREADS), args, 0, s);
    } else {
        const long cells = (long)(a.box.x1 - a.box.x0 + 1) * (a.box.y1 - a.box.y0 + 1);
        const dim3 cell_blocks((unsigned)((cells + THREADS - 1) / THREADS));
        if (point_blocks) e = hipLaunchKernel((const void*)occ_ray_kernel, dim3(point_blocks), dim3(THREADS), args, 0, s);
        if (e == hipSuccess) e = hipLaunchKernel((const void*)occ_cells_kernel, cell_blocks, dim3(THREADS), args, 0, s);
        if (e == hipSuccess) e = hipLaunchKernel((const void*)occ_state_kernel, cell_blocks, dim3(THREADS), args, 0, s);
    }
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t occ_fill(double* p, size_t n, double v, hipStream_t s)
{
    occ_fill_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(p, n, v);
    return hipGetLastError();
}

int occ_lattice_cap(double range, double res) { return occ::lattice_cap(range, res); }

} // namespace backend
