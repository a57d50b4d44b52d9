// fleet_manager_check.cpp -- csrc/fleet_manager.h on the CPU (tests/test_fleet_manager_cpu.py): runs a scenario of
// tests/fleet_manager_cases.py robot by robot through the header's request / begin / end / next_leg, with the slab's load and store
// in between as a kernel lane has them, and prints the slab after every step, every double with 17 digits.
//   usage: fleet_manager_check <scenario file>
//   file:  B P;  replan_time max_replan_time collision_only stop_inside stop_no_path;  nx ny x_lo y_lo res;  nx * ny distances;  then steps:
//          Q has_starts has_goals   + B lines: mask sx sy syaw gx gy gyaw                              (one request call)
//          T now                    + B lines: px py collision predx predy predyaw search build ok n_pieces T[0 .. P-1]   (one period)
//          L reset_legs             + B lines: px py pyaw task_status n_order, 20 x (gx gy), 20 x yaw                     (next_legs)
//   out:   after every T and L step B lines "11 ints 14 doubles" (the rows of alore_backend_get_manager), then "C" and the 8 counters
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fleet_manager.h"

namespace {
void count(int* counters, int ev)
{
    for (int k = 0; k < 7; ++k)
        if ((ev >> k) & 1) counters[k] += 1;
}
void print(const fleet::Slab& s, int B)
{
    for (int b = 0; b < B; ++b) {
        const int* rows[fleet::SLAB_INT_ROWS] = {s.state, s.have_goal, s.have_start, s.leg, s.action, s.returned, s.plan_mask, s.fresh_mask,
                                                 s.replan_mask, s.stop_mask, s.after_plan_mask};
        for (const int* r : rows) std::printf("%d ", r[b]);
        for (int k = 0; k < fleet::SLAB_DOUBLE_ROWS; ++k) std::printf("%.17g ", s.goal[(long)k * B + b]); // the double rows are one block
        std::printf("\n");
    }
    std::printf("C");
    for (int k = 0; k < fleet::N_COUNTERS; ++k) std::printf(" %d", s.counters[k]);
    std::printf("\n");
}
} // namespace

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int B, P, nx, ny;
    fleet::Params prm;
    fleet::default_params(&prm);
    double x_lo, y_lo, res;
    if (std::fscanf(f, "%d %d", &B, &P) != 2 || B < 1 || P < 1) return 3;
    if (std::fscanf(f, "%lf %lf %d %d %d", &prm.replan_time, &prm.max_replan_time, &prm.replan_on_collision_only, &prm.stop_inside_obstacle,
                    &prm.stop_on_no_path) != 5)
        return 3;
    if (std::fscanf(f, "%d %d %lf %lf %lf", &nx, &ny, &x_lo, &y_lo, &res) != 5 || nx < 1 || ny < 1) return 3;
    // every array on the heap with its exact size: the address sanitizer sees an overrun
    double* dist = new double[(size_t)nx * ny];
    for (size_t c = 0; c < (size_t)nx * ny; ++c)
        if (std::fscanf(f, "%lf", &dist[c]) != 1) return 3;
    int* ints = new int[(size_t)B * fleet::SLAB_INT_ROWS + fleet::N_COUNTERS]();
    double* dbl = new double[(size_t)B * fleet::SLAB_DOUBLE_ROWS]();
    fleet::Slab s{};
    s.B = B;
    s.state = ints; s.have_goal = ints + B; s.have_start = ints + 2 * B; s.leg = ints + 3 * B; s.action = ints + 4 * B; s.returned = ints + 5 * B;
    s.plan_mask = ints + 6 * B; s.fresh_mask = ints + 7 * B; s.replan_mask = ints + 8 * B; s.stop_mask = ints + 9 * B; s.after_plan_mask = ints + 10 * B;
    s.counters = ints + 11 * B;
    s.goal = dbl; s.start = dbl + 3 * B; s.plan_start_xytheta = dbl + 6 * B;
    s.loop_start_time = dbl + 9 * B; s.plan_start_time = dbl + 10 * B; s.traj_start_time = dbl + 11 * B; s.traj_total_time = dbl + 12 * B;
    s.time = dbl + 13 * B;
    for (int b = 0; b < B; ++b) fleet::store(s, b, fleet::initial());
    double* T = new double[(size_t)P];
    char op[8];
    while (std::fscanf(f, "%7s", op) == 1) {
        if (op[0] == 'Q') {
            int hs, hg;
            if (std::fscanf(f, "%d %d", &hs, &hg) != 2) return 3;
            s.counters[6] = 0;
            for (int b = 0; b < B; ++b) {
                int mask;
                double st[3], gl[3];
                if (std::fscanf(f, "%d %lf %lf %lf %lf %lf %lf", &mask, &st[0], &st[1], &st[2], &gl[0], &gl[1], &gl[2]) != 7) return 3;
                if (!mask) continue;
                fleet::Robot r = fleet::load(s, b);
                s.counters[6] += fleet::request(r, hs ? st : nullptr, hg ? gl : nullptr);
                fleet::store(s, b, r);
            }
        } else if (op[0] == 'T') {
            double now;
            if (std::fscanf(f, "%lf", &now) != 1) return 3;
            for (int b = 0; b < B; ++b) {
                double pose[3] = {0, 0, 0}, pred[3];
                int collision, search, build, ok, n;
                if (std::fscanf(f, "%lf %lf %d %lf %lf %lf %d %d %d %d", &pose[0], &pose[1], &collision, &pred[0], &pred[1], &pred[2], &search, &build, &ok,
                                &n) != 10)
                    return 3;
                for (int i = 0; i < P; ++i)
                    if (std::fscanf(f, "%lf", &T[i]) != 1) return 3;
                // begin
                fleet::Robot r = fleet::load(s, b);
                fleet::Flags fl;
                const bool inside = fleet::inside_obstacle(dist, nx, ny, x_lo, y_lo, x_lo + nx * res, y_lo + ny * res, res, pose[0], pose[1]);
                count(s.counters, fleet::begin(r, prm, now, pose, inside, collision != 0, fl));
                fleet::store(s, b, r);
                fleet::store_flags(s, b, fl);
                // starts: the predicted pose of a REPLAN robot
                if (s.action[b] == fleet::ACT_REPLAN)
                    for (int k = 0; k < 3; ++k) s.plan_start_xytheta[(long)k * B + b] = pred[k];
                // end
                r = fleet::load(s, b);
                fl = fleet::load_flags(s, b);
                const bool planned = !r.returned && r.action != fleet::ACT_NONE;
                n = n < 0 ? 0 : (n > P ? P : n);
                count(s.counters, fleet::end(r, prm, now, planned ? search : 0, planned ? build : 0, planned ? ok : 0,
                                             planned ? fleet::total_duration(T, n) : 0.0, fl));
                fleet::store(s, b, r);
                fleet::store_flags(s, b, fl);
            }
            print(s, B);
        } else if (op[0] == 'L') {
            int reset;
            if (std::fscanf(f, "%d", &reset) != 1) return 3;
            double* goals = new double[fleet::MAX_LEGS * 2];
            double* yaws = new double[fleet::MAX_LEGS];
            for (int b = 0; b < B; ++b) {
                double pose[3];
                int status, n_order;
                if (std::fscanf(f, "%lf %lf %lf %d %d", &pose[0], &pose[1], &pose[2], &status, &n_order) != 5) return 3;
                for (int i = 0; i < fleet::MAX_LEGS * 2; ++i)
                    if (std::fscanf(f, "%lf", &goals[i]) != 1) return 3;
                for (int i = 0; i < fleet::MAX_LEGS; ++i)
                    if (std::fscanf(f, "%lf", &yaws[i]) != 1) return 3;
                fleet::Robot r = fleet::load(s, b);
                fleet::next_leg(r, status, n_order, goals, yaws, pose, reset != 0);
                fleet::store(s, b, r);
            }
            delete[] goals; delete[] yaws;
            print(s, B);
        } else
            return 3;
    }
    std::fclose(f);
    delete[] T; delete[] dist; delete[] ints; delete[] dbl;
    return 0;
}
