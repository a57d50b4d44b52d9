// path_search_check.cpp -- csrc/path_search.h on the CPU (tests/test_path_search_cpu.py): runs the problems of a text file through
// psearch::search_one (the header's own sweeps, walk and pruning) and prints every result, every double with 17 digits.
//   usage: path_search_check <problems file>
//   file:  nx ny x_lo y_lo res  n_problems;  nx * ny distances;  then per problem:  sx sy gx gy safe_dis window_margin
//   out:   per problem "status n_points a b sweeps", then the 31 x 2 doubles of its xy row (pre-filled with -777)
#include <cstdio>
#include <cstdlib>

#include "path_search.h"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int nx, ny, n;
    double x_lo, y_lo, res;
    if (std::fscanf(f, "%d %d %lf %lf %lf %d", &nx, &ny, &x_lo, &y_lo, &res, &n) != 6 || nx < 2 || ny < 2 || n < 0) return 3;
    const size_t cells = (size_t)nx * ny;
    // every array on the heap with its exact size: the address sanitizer sees an overrun
    double* dist = new double[cells];
    for (size_t c = 0; c < cells; ++c)
        if (std::fscanf(f, "%lf", &dist[c]) != 1) return 3;
    const psearch::Grid g = psearch::make_grid(dist, nx, ny, x_lo, y_lo, x_lo + nx * res, y_lo + ny * res, res);
    const size_t cap = cells < (size_t)psearch::MAX_CELLS ? cells : (size_t)psearch::MAX_CELLS; // a window is clipped to the map
    for (int k = 0; k < n; ++k) {
        double s[2], e[2];
        psearch::Params p;
        if (std::fscanf(f, "%lf %lf %lf %lf %lf %lf", &s[0], &s[1], &e[0], &e[1], &p.safe_dis, &p.window_margin) != 6) return 3;
        unsigned* words = new unsigned[cap];
        int* nodes = new int[psearch::MAX_NODES];
        double* xy = new double[psearch::MAX_POINTS * 2];
        for (int i = 0; i < psearch::MAX_POINTS * 2; ++i) xy[i] = -777.0;
        int n_points = -1, cost[2] = {-1, -1}, sweeps = 0;
        const int status = psearch::search_one(g, s, e, p, words, nodes, &n_points, xy, cost, &sweeps);
        std::printf("%d %d %d %d %d\n", status, n_points, cost[0], cost[1], sweeps);
        for (int i = 0; i < psearch::MAX_POINTS * 2; ++i) std::printf("%.17g ", xy[i]);
        std::printf("\n");
        delete[] words; delete[] nodes; delete[] xy;
    }
    std::fclose(f);
    delete[] dist;
    return 0;
}
