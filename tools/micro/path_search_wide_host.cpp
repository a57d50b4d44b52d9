// path_search_wide_host.cpp -- csrc/path_search_wide.h on one host core: the time of psearch::search_one_wide (tiles of
// 126 x 126, the kernel's size) per problem, for the comparison that tools/path_search.py wide prints.
//   usage: path_search_wide_host <map file: nx * ny float64> nx ny x_lo y_lo res <problems file: n x 4 float64> safe_dis window_margin
//          max_cells
//   out:   "n total_us max_visits", then the count of every status 0 .. -6
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "path_search_wide.h"

int main(int argc, char** argv)
{
    if (argc != 11) return 2;
    const int nx = std::atoi(argv[2]), ny = std::atoi(argv[3]);
    const double x_lo = std::atof(argv[4]), y_lo = std::atof(argv[5]), res = std::atof(argv[6]);
    const long long max_cells = std::atoll(argv[10]);
    if (nx < 2 || ny < 2 || !(res > 0.0) || max_cells < 1 || max_cells > psearch::WIDE_MAX_CELLS) return 2;
    std::vector<double> dist((size_t)nx * ny), prob;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(dist.data(), sizeof(double), dist.size(), f) != dist.size()) return 2;
    std::fclose(f);
    f = std::fopen(argv[7], "rb");
    if (!f) return 2;
    double buf[4];
    while (std::fread(buf, sizeof(double), 4, f) == 4) prob.insert(prob.end(), buf, buf + 4);
    std::fclose(f);
    const psearch::Params p{std::atof(argv[8]), std::atof(argv[9])};
    const psearch::Grid g = psearch::make_grid(dist.data(), nx, ny, x_lo, y_lo, x_lo + nx * res, y_lo + ny * res, res);
    constexpr int T = 126;
    std::vector<unsigned> slab((size_t)max_cells), tile((T + 2) * (T + 2)), dirty(psearch::dirty_words<T, T>(max_cells));
    std::vector<int> nodes(psearch::MAX_NODES);
    double xy[psearch::MAX_POINTS * 2];
    long counts[7] = {0, 0, 0, 0, 0, 0, 0};
    int max_visits = 0;
    const size_t n = prob.size() / 4;
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t b = 0; b < n; ++b) {
        int n_points, cost[2], visits;
        const int st = psearch::search_one_wide<T, T>(g, &prob[4 * b], &prob[4 * b + 2], p, max_cells, slab.data(), tile.data(), dirty.data(),
                                                      nodes.data(), &n_points, xy, cost, &visits);
        counts[-st] += 1;
        if (visits > max_visits) max_visits = visits;
    }
    const auto t1 = std::chrono::steady_clock::now();
    std::printf("%zu %.1f %d\n", n, std::chrono::duration<double, std::micro>(t1 - t0).count(), max_visits);
    for (long c : counts) std::printf("%ld ", c);
    std::printf("\n");
    return 0;
}
