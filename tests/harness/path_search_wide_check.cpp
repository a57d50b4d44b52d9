// path_search_wide_check.cpp -- csrc/path_search_wide.h on the CPU (tests/test_path_search_wide_cpu.py): runs the problems of a
// text file through psearch::search_one_wide, i.e. EVERY window by the tiled iteration whatever its size, and prints every
// result, every double with 17 digits.
//   usage: path_search_wide_check <problems file> <tiles: 8x8 | 5x7 | 126x126> <max_cells>
//   file:  nx ny x_lo y_lo res  n_problems;  nx * ny distances;  then per problem:  sx sy gx gy safe_dis window_margin
//   out:   per problem "status n_points a b visits", then the 31 x 2 doubles of its xy row (pre-filled with -777)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "path_search_wide.h"

template <int TX, int TY>
static int run(std::FILE* f, const psearch::Grid& g, size_t cells, int n, long long max_cells)
{
    const size_t cap = cells < (size_t)max_cells ? cells : (size_t)max_cells; // a window is clipped to the map
    for (int k = 0; k < n; ++k) {
        double s[2], e[2];
        psearch::Params p;
        if (std::fscanf(f, "%lf %lf %lf %lf %lf %lf", &s[0], &s[1], &e[0], &e[1], &p.safe_dis, &p.window_margin) != 6) return 3;
        // every array on the heap with its exact size: the address sanitizer sees an overrun
        unsigned* slab = new unsigned[cap];
        unsigned* tile = new unsigned[(TX + 2) * (TY + 2)];
        unsigned* dirty = new unsigned[psearch::dirty_words<TX, TY>((long long)cap)];
        int* nodes = new int[psearch::MAX_NODES];
        double* xy = new double[psearch::MAX_POINTS * 2];
        for (int i = 0; i < psearch::MAX_POINTS * 2; ++i) xy[i] = -777.0;
        int n_points = -1, cost[2] = {-1, -1}, visits = 0;
        const int status = psearch::search_one_wide<TX, TY>(g, s, e, p, max_cells, slab, tile, dirty, nodes, &n_points, xy, cost, &visits);
        std::printf("%d %d %d %d %d\n", status, n_points, cost[0], cost[1], visits);
        for (int i = 0; i < psearch::MAX_POINTS * 2; ++i) std::printf("%.17g ", xy[i]);
        std::printf("\n");
        delete[] slab; delete[] tile; delete[] dirty; delete[] nodes; delete[] xy;
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    const long long max_cells = std::atoll(argv[3]);
    int nx, ny, n;
    double x_lo, y_lo, res;
    if (std::fscanf(f, "%d %d %lf %lf %lf %d", &nx, &ny, &x_lo, &y_lo, &res, &n) != 6 || nx < 2 || ny < 2 || n < 0 || max_cells < 1) return 3;
    const size_t cells = (size_t)nx * ny;
    double* dist = new double[cells];
    for (size_t c = 0; c < cells; ++c)
        if (std::fscanf(f, "%lf", &dist[c]) != 1) return 3;
    const psearch::Grid g = psearch::make_grid(dist, nx, ny, x_lo, y_lo, x_lo + nx * res, y_lo + ny * res, res);
    int rc = 2;
    if (!std::strcmp(argv[2], "8x8")) rc = run<8, 8>(f, g, cells, n, max_cells);
    else if (!std::strcmp(argv[2], "5x7")) rc = run<5, 7>(f, g, cells, n, max_cells);
    else if (!std::strcmp(argv[2], "126x126")) rc = run<126, 126>(f, g, cells, n, max_cells);
    std::fclose(f);
    delete[] dist;
    return rc;
}
