// task_assign_check.cpp -- the modes of csrc/task_plan.h that choose the assignment, on the CPU (tests/test_task_assign_cpu.py): runs
// the missions of a text file through tplan::plan_one_assigned (the header's own fields, matching, routing and joint programme) and
// prints every result row, every double with 17 digits.  Every row is pre-filled (ints -9, doubles -777), so what a mission must
// leave untouched shows.  With "matrix" as the first argument the file holds cost matrices instead of a map: the programmes alone.
//   usage: task_assign_check <missions file>  |  task_assign_check matrix <matrices file>
//   file:  as task_plan_check.cpp reads it, mode 2 or 3; a given assignment is read and dropped: these modes take none
//   out:   as task_plan_check.cpp prints it, and a sixth line per mission: the 10 ints of the assignment and the 2 of assign_total
//   matrices file: mode count; per matrix n and the P * P pairs (a, b), P = 1 + 2 n, row by row
//   out:   per matrix "status n_order total_a total_b", the 20 ints of the order, the 10 + 2 ints of the assignment rows
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "task_plan.h"

namespace {

// the tables with their exact sizes: the address sanitizer sees an overrun
tplan::Cost* new_table(int mode) { return new tplan::Cost[mode == tplan::JOINT ? tplan::JOINT_STATES : tplan::ASSIGNED_STATES]; }

void print_ints(const int* v, int n)
{
    for (int i = 0; i < n; ++i) std::printf("%d ", v[i]);
    std::printf("\n");
}

// the programmes on a given matrix: what plan_one_assigned does behind the matrix
int run_matrices(std::FILE* f)
{
    int mode, count;
    if (std::fscanf(f, "%d %d", &mode, &count) != 2 || (mode != tplan::ASSIGNED && mode != tplan::JOINT)) return 3;
    const int M = tplan::P_MAX * tplan::P_MAX * 2, L = tplan::MAX_LEGS, T = tplan::MAX_TASKS;
    for (int k = 0; k < count; ++k) {
        int n;
        if (std::fscanf(f, "%d", &n) != 1 || n < 1 || n > (mode == tplan::JOINT ? tplan::JOINT_MAX_TASKS : T)) return 3;
        int *matrix = new int[M], *order = new int[L], *rows = new int[T + 2], *scalars = new int[3];
        for (int i = 0; i < M; ++i) matrix[i] = -9;
        for (int i = 0; i < L; ++i) order[i] = -9;
        for (int i = 0; i < T + 2; ++i) rows[i] = -9;
        for (int i = 0; i < 3; ++i) scalars[i] = -9;
        const int P = 1 + 2 * n;
        for (int i = 0; i < P; ++i)
            for (int j = 0; j < P; ++j) {
                tplan::Cost c;
                if (std::fscanf(f, "%d %d", &c.a, &c.b) != 2) return 3;
                tplan::put_entry(matrix, i, j, c);
            }
        tplan::Cost* table = new_table(mode);
        int status;
        if (mode == tplan::JOINT) {
            for (int level = n; level >= 1; --level)
                for (unsigned e = 0; e < tplan::joint_span(n); ++e)
                    if (tplan::joint_on_level(n, e, level)) table[e] = tplan::joint_state(matrix, n, table, e);
            int asg[tplan::JOINT_MAX_TASKS], sum[2];
            status = tplan::joint_order(matrix, n, table, order, &scalars[0], &scalars[1], asg, sum);
            if (status == tplan::OK) {
                std::memcpy(rows, asg, sizeof(int) * n);
                rows[T] = sum[0]; rows[T + 1] = sum[1];
            }
        } else {
            tplan::Cost* rest = table + tplan::STATES;
            for (int level = n; level >= 0; --level)
                for (unsigned S = 0; S < (1u << n); ++S)
                    if (tplan::popcount(S) == level) rest[S] = tplan::rest_state(matrix, n, rest, S);
            scalars[0] = 0;
            status = tplan::matching(matrix, n, rest, rows, rows + T);
            if (status == tplan::OK) {
                const tplan::Out o{matrix, order, &scalars[0], &scalars[1], nullptr, nullptr, nullptr, nullptr};
                status = tplan::route_one(matrix, n, rows, table, o);
            }
        }
        std::printf("%d %d %d %d\n", status, scalars[0], scalars[1], scalars[2]);
        print_ints(order, L);
        print_ints(rows, T + 2);
        delete[] matrix; delete[] order; delete[] rows; delete[] scalars; delete[] table;
    }
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "matrix")) {
        std::FILE* f = std::fopen(argv[2], "r");
        if (!f) return 2;
        const int rc = run_matrices(f);
        std::fclose(f);
        return rc;
    }
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int nx, ny, count, T, has_assign;
    double x_lo, y_lo, res;
    tplan::Params p;
    if (std::fscanf(f, "%d %d %lf %lf %lf %d %d %d %lf %lf %d", &nx, &ny, &x_lo, &y_lo, &res, &count, &T, &p.mode, &p.safe_dis, &p.window_margin,
                    &has_assign) != 11 || nx < 2 || ny < 2 || count < 0 || T < 1 || T > tplan::MAX_TASKS ||
        (p.mode != tplan::ASSIGNED && p.mode != tplan::JOINT))
        return 3;
    const size_t cells = (size_t)nx * ny;
    double* dist = new double[cells];
    for (size_t c = 0; c < cells; ++c)
        if (std::fscanf(f, "%lf", &dist[c]) != 1) return 3;
    const psearch::Grid g = psearch::make_grid(dist, nx, ny, x_lo, y_lo, x_lo + nx * res, y_lo + ny * res, res);
    const size_t cap = cells < (size_t)psearch::MAX_CELLS ? cells : (size_t)psearch::MAX_CELLS; // a window is clipped to the map
    const int M = tplan::P_MAX * tplan::P_MAX * 2, L = tplan::MAX_LEGS;
    for (int k = 0; k < count; ++k) {
        int n, dropped;
        if (std::fscanf(f, "%d", &n) != 1) return 3;
        double* pts = new double[2 * (1 + 2 * T)];
        for (int i = 0; i < 2 * (1 + 2 * T); ++i)
            if (std::fscanf(f, "%lf", &pts[i]) != 1) return 3;
        for (int i = 0; has_assign && i < T; ++i)
            if (std::fscanf(f, "%d", &dropped) != 1) return 3;
        unsigned* words = new unsigned[cap];
        tplan::Cost* table = new_table(p.mode);
        int *matrix = new int[M], *order = new int[L], *scalars = new int[5], *assignment = new int[tplan::MAX_TASKS], *assign_total = new int[2];
        double *leg_start = new double[2 * L], *leg_goal = new double[2 * L];
        for (int i = 0; i < M; ++i) matrix[i] = -9;
        for (int i = 0; i < L; ++i) order[i] = -9;
        for (int i = 0; i < 5; ++i) scalars[i] = -9;
        for (int i = 0; i < tplan::MAX_TASKS; ++i) assignment[i] = -9;
        assign_total[0] = assign_total[1] = -9;
        for (int i = 0; i < 2 * L; ++i) leg_start[i] = leg_goal[i] = -777.0;
        const tplan::Out o{matrix, order, &scalars[0], &scalars[1], leg_start, leg_goal, &scalars[3], &scalars[4]};
        const int status = tplan::plan_one_assigned(g, n, T, pts, p, words, table, o, assignment, assign_total);
        std::printf("%d %d %d %d %d %d\n", status, scalars[0], scalars[1], scalars[2], scalars[3], scalars[4]);
        print_ints(matrix, M);
        print_ints(order, L);
        for (int i = 0; i < 2 * L; ++i) std::printf("%.17g ", leg_start[i]);
        std::printf("\n");
        for (int i = 0; i < 2 * L; ++i) std::printf("%.17g ", leg_goal[i]);
        std::printf("\n");
        print_ints(assignment, tplan::MAX_TASKS);
        print_ints(assign_total, 2);
        delete[] pts; delete[] words; delete[] table; delete[] matrix; delete[] order; delete[] scalars; delete[] assignment;
        delete[] assign_total; delete[] leg_start; delete[] leg_goal;
    }
    std::fclose(f);
    delete[] dist;
    return 0;
}
