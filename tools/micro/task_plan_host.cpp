// task_plan_host.cpp -- csrc/task_plan.h on one host core: the time of tplan::plan_one per mission, for the comparison that
// tools/task_plan.py prints.
//   usage: task_plan_host <map file: nx * ny float64> nx ny x_lo y_lo res <missions file: count x (1 + 2 n) x 2 float64> n mode
//          safe_dis window_margin
//   out:   "count total_us fields_sum max_sweeps ok no_order", and a checksum of the orders
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "task_plan.h"

int main(int argc, char** argv)
{
    if (argc != 12) return 2;
    const int nx = std::atoi(argv[2]), ny = std::atoi(argv[3]), n = std::atoi(argv[8]);
    const double x_lo = std::atof(argv[4]), y_lo = std::atof(argv[5]), res = std::atof(argv[6]);
    if (nx < 2 || ny < 2 || !(res > 0.0) || n < 1 || n > tplan::MAX_TASKS) return 2;
    std::vector<double> dist((size_t)nx * ny), pts;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(dist.data(), sizeof(double), dist.size(), f) != dist.size()) return 2;
    std::fclose(f);
    f = std::fopen(argv[7], "rb");
    if (!f) return 2;
    const size_t row = 2 * (1 + 2 * (size_t)n);
    std::vector<double> buf(row);
    while (std::fread(buf.data(), sizeof(double), row, f) == row) pts.insert(pts.end(), buf.begin(), buf.end());
    std::fclose(f);
    const tplan::Params p{std::atof(argv[10]), std::atof(argv[11]), std::atoi(argv[9])};
    const psearch::Grid g = psearch::make_grid(dist.data(), nx, ny, x_lo, y_lo, x_lo + nx * res, y_lo + ny * res, res);
    std::vector<unsigned> words(psearch::MAX_CELLS);
    std::vector<tplan::Cost> togo(tplan::STATES);
    std::vector<int> matrix(tplan::P_MAX * tplan::P_MAX * 2), order(tplan::MAX_LEGS);
    std::vector<double> legs(4 * tplan::MAX_LEGS);
    const size_t count = pts.size() / row;
    long fields_sum = 0, ok = 0, no_order = 0;
    unsigned long checksum = 0;
    int max_sweeps = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t m = 0; m < count; ++m) {
        int n_order = 0, total[2] = {0, 0}, fields = 0, sweeps = 0;
        const tplan::Out o{matrix.data(), order.data(), &n_order, total, legs.data(), legs.data() + 2 * tplan::MAX_LEGS, &fields, &sweeps};
        const int st = tplan::plan_one(g, n, n, &pts[row * m], nullptr, p, words.data(), togo.data(), o);
        ok += st == tplan::OK;
        no_order += st == tplan::E_NO_ORDER;
        fields_sum += fields;
        if (sweeps > max_sweeps) max_sweeps = sweeps;
        for (int e = 0; e < n_order; ++e) checksum = checksum * 31u + (unsigned long)order[e];
    }
    const auto t1 = std::chrono::steady_clock::now();
    std::printf("%zu %.1f %ld %d %ld %ld\n%lu\n", count, std::chrono::duration<double, std::micro>(t1 - t0).count(), fields_sum, max_sweeps, ok,
                no_order, checksum);
    return 0;
}
