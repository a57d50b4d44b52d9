// esdf_window.h -- the window of SDFmap::updateESDF2d (P/utils/plan_env/src/sdf_map.cpp:618-640) and the workspace that holds every
// window of a map, stated once for esdf_enqueue, esdf_update and the resident map (esdf_build.hip, backend_capi.hip).  Plain C++, no
// HIP: tests/harness/esdf_window_check.cpp compiles it with g++ alone (tests/test_esdf_window_cpu.py).
//
// The window is the cells min .. max around odom +- range, clipped to the map.  Its upper end is ceil(min(n res, ...) (1 / res)) - 1:
// where ceil((n res) (1 / res)) rounds up (n = 3, 6, 7, 12, ... at res 0.1) it is n, one row or column past the map, as in the
// reference.  The kernels read the (X + 1) x (Y + 1) cells min .. max and write the X x Y cells min .. max - 1, so every write lies
// in the map and the reads reach at most cell [GLX][GLY]: flat index GLX GLY + GLY.  Cells past the end of the grid are unknown (0):
// whoever owns the grid carries GLY + 1 zero cells after its last row.
#pragma once
#include <cmath>
#include <cstddef>

namespace backend {

struct EsdfWindow {
    int min_x, min_y, max_x, max_y;
    int X, Y;     // max - min: the kernels run lines 0 .. X and 0 .. Y
    int D;        // max(X, Y) + 1: the stride of the envelope stacks and the number of lines
    int empty;    // X < 1 or Y < 1: nothing to update
    size_t total; // (X + 1) (Y + 1) cells of tmp, pos and neg
};

inline EsdfWindow esdf_window(int GLX, int GLY, double res, double x_lo, double y_lo, double odom_x, double odom_y, double range)
{
    const double inv = 1.0 / res, gx = GLX * res, gy = GLY * res;
    const int min_x = (int)floor(fmax(0.0, odom_x - range - x_lo) * inv), min_y = (int)floor(fmax(0.0, odom_y - range - y_lo) * inv);
    const int max_x = (int)ceil(fmin(gx, odom_x + range - x_lo) * inv) - 1, max_y = (int)ceil(fmin(gy, odom_y + range - y_lo) * inv) - 1;
    const int X = max_x - min_x, Y = max_y - min_y;
    EsdfWindow w{min_x, min_y, max_x, max_y, X, Y, 0, (X < 1 || Y < 1) ? 1 : 0, 0};
    if (w.empty) return w;
    w.total = (size_t)(X + 1) * (Y + 1);
    w.D = (X > Y ? X : Y) + 1;
    return w;
}

// the largest window of a map of GLX x GLY cells at this detection range: (X + 1) <= xc, (Y + 1) <= yc
inline void esdf_workspace_size(int GLX, int GLY, double res, double range, size_t* cells, int* lines)
{
    const double span = ceil(2.0 * range / res) + 3.0;
    const int xc = span < GLX + 1 ? (int)span : GLX + 1, yc = span < GLY + 1 ? (int)span : GLY + 1;
    *cells = (size_t)xc * yc;
    *lines = xc > yc ? xc : yc;
}

} // namespace backend
