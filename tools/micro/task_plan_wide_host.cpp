// task_plan_wide_host.cpp -- csrc/task_plan_wide.h on one host core: the time of tplan::plan_one_wide (tiles of 126 x 126, the
// kernel's size) per mission, for the comparison that tools/task_plan.py wide prints.
//   usage: task_plan_wide_host <map file: nx * ny float64> nx ny x_lo y_lo res <missions file: count x (1 + 2 n) x 2 float64> n mode
//          safe_dis window_margin max_cells
//   out:   "count total_us fields max_visits ok range"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "task_plan_wide.h"

int main(int argc, char** argv)
{
    if (argc != 13) return 2;
    const int nx = std::atoi(argv[2]), ny = std::atoi(argv[3]), n = std::atoi(argv[8]);
    const double x_lo = std::atof(argv[4]), y_lo = std::atof(argv[5]), res = std::atof(argv[6]);
    tplan::Params p;
    p.mode = std::atoi(argv[9]); p.safe_dis = std::atof(argv[10]); p.window_margin = std::atof(argv[11]);
    const long long max_cells = std::atoll(argv[12]);
    if (nx < 2 || ny < 2 || !(res > 0.0) || n < 1 || n > tplan::MAX_TASKS || p.mode < tplan::GREEDY || p.mode > tplan::JOINT || max_cells < 1 ||
        max_cells > psearch::WIDE_MAX_CELLS)
        return 2;
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
    const psearch::Grid g = psearch::make_grid(dist.data(), nx, ny, x_lo, y_lo, x_lo + nx * res, y_lo + ny * res, res);
    constexpr int T = 126;
    std::vector<unsigned> slab((size_t)max_cells), tile((T + 2) * (T + 2)), dirty(psearch::dirty_words<T, T>(max_cells));
    std::vector<tplan::Cost> table(tplan::ASSIGNED_STATES);
    std::vector<int> matrix(tplan::P_MAX * tplan::P_MAX * 2), order(tplan::MAX_LEGS);
    std::vector<double> leg_start(2 * tplan::MAX_LEGS), leg_goal(2 * tplan::MAX_LEGS);
    int n_order, total[2], fields, visits, assignment[tplan::MAX_TASKS], assign_total[2];
    long all_fields = 0, ok = 0, range = 0;
    int max_visits = 0;
    const size_t count = pts.size() / row;
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t b = 0; b < count; ++b) {
        fields = visits = 0;
        const tplan::Out o{matrix.data(), order.data(), &n_order, total, leg_start.data(), leg_goal.data(), &fields, &visits};
        const int st = tplan::plan_one_wide<T, T>(g, n, n, &pts[row * b], nullptr, p, max_cells, slab.data(), tile.data(), dirty.data(), table.data(),
                                                  o, assignment, assign_total);
        all_fields += fields;
        ok += st == tplan::OK;
        range += st == tplan::E_RANGE;
        if (visits > max_visits) max_visits = visits;
    }
    const auto t1 = std::chrono::steady_clock::now();
    std::printf("%zu %.1f %ld %d %ld %ld\n", count, std::chrono::duration<double, std::micro>(t1 - t0).count(), all_fields, max_visits, ok, range);
    return 0;
}
