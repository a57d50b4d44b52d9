// task_plan_check.cpp -- csrc/task_plan.h on the CPU (tests/test_task_plan_cpu.py): runs the missions of a text file through
// tplan::plan_one (the header's own fields, greedy order and dynamic programme) and prints every result row, every double with 17
// digits.  Every row is pre-filled (ints -9, doubles -777), so what a mission must leave untouched shows.
//   usage: task_plan_check <missions file>
//   file:  nx ny x_lo y_lo res  count max_tasks mode safe_dis window_margin has_assignment;  nx * ny distances;  then per mission:
//          n, the 2 (1 + 2 max_tasks) coordinates of its row, and with has_assignment max_tasks ints
//   out:   per mission "status n_order total_a total_b fields sweeps", the 21 x 21 x 2 ints of the matrix, the 20 ints of the order,
//          the 20 x 2 doubles of leg_start_xy, the 20 x 2 doubles of leg_goal_xy, one line each
#include <cstdio>
#include <cstdlib>

#include "task_plan.h"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int nx, ny, count, T, has_assign;
    double x_lo, y_lo, res;
    tplan::Params p;
    if (std::fscanf(f, "%d %d %lf %lf %lf %d %d %d %lf %lf %d", &nx, &ny, &x_lo, &y_lo, &res, &count, &T, &p.mode, &p.safe_dis, &p.window_margin,
                    &has_assign) != 11 || nx < 2 || ny < 2 || count < 0 || T < 1 || T > tplan::MAX_TASKS)
        return 3;
    const size_t cells = (size_t)nx * ny;
    // every array on the heap with its exact size: the address sanitizer sees an overrun
    double* dist = new double[cells];
    for (size_t c = 0; c < cells; ++c)
        if (std::fscanf(f, "%lf", &dist[c]) != 1) return 3;
    const psearch::Grid g = psearch::make_grid(dist, nx, ny, x_lo, y_lo, x_lo + nx * res, y_lo + ny * res, res);
    const size_t cap = cells < (size_t)psearch::MAX_CELLS ? cells : (size_t)psearch::MAX_CELLS; // a window is clipped to the map
    const int M = tplan::P_MAX * tplan::P_MAX * 2, L = tplan::MAX_LEGS;
    for (int k = 0; k < count; ++k) {
        int n;
        if (std::fscanf(f, "%d", &n) != 1) return 3;
        double* pts = new double[2 * (1 + 2 * T)];
        for (int i = 0; i < 2 * (1 + 2 * T); ++i)
            if (std::fscanf(f, "%lf", &pts[i]) != 1) return 3;
        int* assign = has_assign ? new int[T] : nullptr;
        for (int i = 0; has_assign && i < T; ++i)
            if (std::fscanf(f, "%d", &assign[i]) != 1) return 3;
        unsigned* words = new unsigned[cap];
        tplan::Cost* togo = new tplan::Cost[tplan::STATES];
        int *matrix = new int[M], *order = new int[L], *scalars = new int[5];
        double *leg_start = new double[2 * L], *leg_goal = new double[2 * L];
        for (int i = 0; i < M; ++i) matrix[i] = -9;
        for (int i = 0; i < L; ++i) order[i] = -9;
        for (int i = 0; i < 5; ++i) scalars[i] = -9;
        for (int i = 0; i < 2 * L; ++i) leg_start[i] = leg_goal[i] = -777.0;
        const tplan::Out o{matrix, order, &scalars[0], &scalars[1], leg_start, leg_goal, &scalars[3], &scalars[4]};
        const int status = tplan::plan_one(g, n, T, pts, assign, p, words, togo, o);
        std::printf("%d %d %d %d %d %d\n", status, scalars[0], scalars[1], scalars[2], scalars[3], scalars[4]);
        for (int i = 0; i < M; ++i) std::printf("%d ", matrix[i]);
        std::printf("\n");
        for (int i = 0; i < L; ++i) std::printf("%d ", order[i]);
        std::printf("\n");
        for (int i = 0; i < 2 * L; ++i) std::printf("%.17g ", leg_start[i]);
        std::printf("\n");
        for (int i = 0; i < 2 * L; ++i) std::printf("%.17g ", leg_goal[i]);
        std::printf("\n");
        delete[] pts; delete[] assign; delete[] words; delete[] togo; delete[] matrix; delete[] order; delete[] scalars;
        delete[] leg_start; delete[] leg_goal;
    }
    std::fclose(f);
    delete[] dist;
    return 0;
}
