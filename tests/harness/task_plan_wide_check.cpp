// task_plan_wide_check.cpp -- csrc/task_plan_wide.h on the CPU (tests/test_task_plan_wide_cpu.py): runs the missions of a text file
// through tplan::plan_one_wide, which computes EVERY field by the tiled iteration whatever the size of the window, at the tile
// size and under the cap on the window given on the command line, in any of the four modes, and prints every result row, every
// double with 17 digits.  Every row is pre-filled (ints -9, doubles -777), so what a mission must leave untouched shows.
//   usage: task_plan_wide_check <missions file> <8x8 | 5x7 | 126x126> <max cells>
//   file:  as task_plan_check.cpp reads it, mode 0 .. 3
//   out:   as task_assign_check.cpp prints it, seven lines per mission; `sweeps` is the most visits of tiles a field needed
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "task_plan_wide.h"

namespace {

void print_ints(const int* v, int n)
{
    for (int i = 0; i < n; ++i) std::printf("%d ", v[i]);
    std::printf("\n");
}

template <int TX, int TY>
int run(std::FILE* f, long long max_cells)
{
    int nx, ny, count, T, has_assign;
    double x_lo, y_lo, res;
    tplan::Params p;
    if (std::fscanf(f, "%d %d %lf %lf %lf %d %d %d %lf %lf %d", &nx, &ny, &x_lo, &y_lo, &res, &count, &T, &p.mode, &p.safe_dis, &p.window_margin,
                    &has_assign) != 11 || nx < 2 || ny < 2 || count < 0 || T < 1 || T > tplan::MAX_TASKS || p.mode < tplan::GREEDY || p.mode > tplan::JOINT)
        return 3;
    const size_t cells = (size_t)nx * ny;
    // every array on the heap with its exact size: the address sanitizer sees an overrun
    double* dist = new double[cells];
    for (size_t c = 0; c < cells; ++c)
        if (std::fscanf(f, "%lf", &dist[c]) != 1) return 3;
    const psearch::Grid g = psearch::make_grid(dist, nx, ny, x_lo, y_lo, x_lo + nx * res, y_lo + ny * res, res);
    const size_t cap = cells < (size_t)max_cells ? cells : (size_t)max_cells; // a window is clipped to the map
    const int M = tplan::P_MAX * tplan::P_MAX * 2, L = tplan::MAX_LEGS;
    const int states = p.mode == tplan::JOINT ? tplan::JOINT_STATES : p.mode == tplan::ASSIGNED ? tplan::ASSIGNED_STATES : tplan::STATES;
    for (int k = 0; k < count; ++k) {
        int n;
        if (std::fscanf(f, "%d", &n) != 1) return 3;
        double* pts = new double[2 * (1 + 2 * T)];
        for (int i = 0; i < 2 * (1 + 2 * T); ++i)
            if (std::fscanf(f, "%lf", &pts[i]) != 1) return 3;
        int* assign = has_assign ? new int[T] : nullptr;
        for (int i = 0; has_assign && i < T; ++i)
            if (std::fscanf(f, "%d", &assign[i]) != 1) return 3;
        unsigned* slab = new unsigned[cap];
        unsigned* tile = new unsigned[(TX + 2) * (TY + 2)];
        unsigned* dirty = new unsigned[psearch::dirty_words<TX, TY>((long long)cap)];
        tplan::Cost* table = new tplan::Cost[states];
        int *matrix = new int[M], *order = new int[L], *scalars = new int[5], *assignment = new int[tplan::MAX_TASKS], *assign_total = new int[2];
        double *leg_start = new double[2 * L], *leg_goal = new double[2 * L];
        for (int i = 0; i < M; ++i) matrix[i] = -9;
        for (int i = 0; i < L; ++i) order[i] = -9;
        for (int i = 0; i < 5; ++i) scalars[i] = -9;
        for (int i = 0; i < tplan::MAX_TASKS; ++i) assignment[i] = -9;
        assign_total[0] = assign_total[1] = -9;
        for (int i = 0; i < 2 * L; ++i) leg_start[i] = leg_goal[i] = -777.0;
        const tplan::Out o{matrix, order, &scalars[0], &scalars[1], leg_start, leg_goal, &scalars[3], &scalars[4]};
        const int status = tplan::plan_one_wide<TX, TY>(g, n, T, pts, assign, p, (long long)cap, slab, tile, dirty, table, o, assignment, assign_total);
        std::printf("%d %d %d %d %d %d\n", status, scalars[0], scalars[1], scalars[2], scalars[3], scalars[4]);
        print_ints(matrix, M);
        print_ints(order, L);
        for (int i = 0; i < 2 * L; ++i) std::printf("%.17g ", leg_start[i]);
        std::printf("\n");
        for (int i = 0; i < 2 * L; ++i) std::printf("%.17g ", leg_goal[i]);
        std::printf("\n");
        print_ints(assignment, tplan::MAX_TASKS);
        print_ints(assign_total, 2);
        delete[] pts; delete[] assign; delete[] slab; delete[] tile; delete[] dirty; delete[] table; delete[] matrix; delete[] order;
        delete[] scalars; delete[] assignment; delete[] assign_total; delete[] leg_start; delete[] leg_goal;
    }
    delete[] dist;
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const long long max_cells = std::atoll(argv[3]);
    if (max_cells < 1 || max_cells > psearch::WIDE_MAX_CELLS) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int rc = 2;
    if (!std::strcmp(argv[2], "8x8")) rc = run<8, 8>(f, max_cells);
    else if (!std::strcmp(argv[2], "5x7")) rc = run<5, 7>(f, max_cells);
    else if (!std::strcmp(argv[2], "126x126")) rc = run<126, 126>(f, max_cells);
    std::fclose(f);
    return rc;
}
