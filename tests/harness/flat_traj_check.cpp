// flat_traj_check.cpp -- csrc/flat_traj_build.h on the CPU (tests/test_flat_traj_build_cpu.py): builds the problems of the paths
// in a text file with flat_traj::build_problem and prints them, every double with 17 digits.
//   usage: flat_traj_check <paths file>
//   file:  distance_weight yaw_weight traj_cut_length sample_time min_traj_num max_vel max_acc max_pieces count
//          then per path:  n start_yaw end_yaw vaj[3] oaj[3]  x0 y0 ... x(n-1) y(n-1)
//   out:   per path one line: status n_pieces if_cut init_T head[6] tail[6] start_xytheta[3] final_xytheta[3], then n_pieces - 1
//          lines "yaw s x y" and one line "x y" (the final position as the last entry of `positions`)
#include <cstdio>
#include <vector>

#include "flat_traj_build.h"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    flat_traj::Params p;
    int max_pieces = 0, count = 0;
    if (std::fscanf(f, "%lf %lf %lf %lf %d %lf %lf %d %d", &p.distance_weight, &p.yaw_weight, &p.traj_cut_length, &p.sample_time, &p.min_traj_num,
                    &p.max_vel, &p.max_acc, &max_pieces, &count) != 9)
        return 3;
    for (int b = 0; b < count; ++b) {
        int n = 0;
        double sy, ey, vaj[3], oaj[3];
        if (std::fscanf(f, "%d %lf %lf %lf %lf %lf %lf %lf %lf", &n, &sy, &ey, &vaj[0], &vaj[1], &vaj[2], &oaj[0], &oaj[1], &oaj[2]) != 9 || n < 0) return 3;
        std::vector<double> xy(2 * (size_t)n);
        for (double& v : xy)
            if (std::fscanf(f, "%lf", &v) != 1) return 3;
        flat_traj::Problem* q = new flat_traj::Problem(); // on the heap: the address sanitizer sees an overrun of its arrays
        flat_traj::build_problem(p, max_pieces, n, xy.data(), sy, ey, vaj, oaj, q);
        if (q->status != flat_traj::BUILT) {
            std::printf("%d 0 0 0\n", q->status);
            delete q;
            continue;
        }
        std::printf("%d %d %d %.17g", q->status, q->n_pieces, q->if_cut, q->init_T);
        for (int k = 0; k < 6; ++k) std::printf(" %.17g", q->head[k]);
        for (int k = 0; k < 6; ++k) std::printf(" %.17g", q->tail[k]);
        for (int k = 0; k < 3; ++k) std::printf(" %.17g", q->start_xytheta[k]);
        for (int k = 0; k < 3; ++k) std::printf(" %.17g", q->final_xytheta[k]);
        std::printf("\n");
        const int m = q->n_pieces - 1;
        for (int i = 0; i < m; ++i) std::printf("%.17g %.17g %.17g %.17g\n", q->inner[i][0], q->inner[i][1], q->positions[i][0], q->positions[i][1]);
        std::printf("%.17g %.17g\n", q->positions[m][0], q->positions[m][1]);
        delete q;
    }
    std::fclose(f);
    return 0;
}
