// icr_ekf_check.cpp -- csrc/icr_ekf.h on the CPU (tests/test_icr_ekf_cpu.py): runs the groups of a text file through
// icrekf::step_one and prints the state after every step, every double as a hexadecimal float (exact both ways).
//   usage: icr_ekf_check <groups file>
//   file:  n_groups;  per group: q[6] r[3] standard[3]  x[6] P[36] u[2]  n_steps;  per step: wheel[2] dt has_z z[3] mask
//          (mask: -1 none, else the robot's mask byte)
//   out:   per step "status", then x[6] P[36] u[2], then run[3] conv[3] conv_step[3] steps
#include <cstdio>
#include <cstdlib>

#include "icr_ekf.h"

static bool read(std::FILE* f, double* v, int n)
{
    for (int i = 0; i < n; ++i)
        if (std::fscanf(f, "%lf", &v[i]) != 1) return false;
    return true;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int n_groups;
    if (std::fscanf(f, "%d", &n_groups) != 1 || n_groups < 0) return 3;
    for (int g = 0; g < n_groups; ++g) {
        icrekf::Params p;
        // every array on the heap with its exact size: the address sanitizer sees an overrun
        double* x = new double[6];
        double* P = new double[36];
        double* u = new double[2];
        int n_steps;
        if (!read(f, p.q, 6) || !read(f, p.r, 3) || !read(f, p.standard, 3) || !read(f, x, 6) || !read(f, P, 36) || !read(f, u, 2) ||
            std::fscanf(f, "%d", &n_steps) != 1)
            return 3;
        icrekf::Flags fl;
        icrekf::reset_flags(fl);
        for (int s = 0; s < n_steps; ++s) {
            double* wheel = new double[2];
            double* z = new double[3];
            double dt;
            int has_z, mask;
            if (!read(f, wheel, 2) || !read(f, &dt, 1) || std::fscanf(f, "%d", &has_z) != 1 || !read(f, z, 3) || std::fscanf(f, "%d", &mask) != 1)
                return 3;
            const unsigned char m = (unsigned char)(mask > 0);
            const int st = icrekf::step_one(p, x, P, u, fl, wheel, dt, z, has_z != 0, mask < 0 ? nullptr : &m);
            std::printf("%d\n", st);
            for (int i = 0; i < 6; ++i) std::printf("%a ", x[i]);
            for (int i = 0; i < 36; ++i) std::printf("%a ", P[i]);
            std::printf("%a %a\n", u[0], u[1]);
            std::printf("%d %d %d %d %d %d %d %d %d %d\n", fl.run[0], fl.run[1], fl.run[2], fl.conv[0], fl.conv[1], fl.conv[2], fl.conv_step[0],
                        fl.conv_step[1], fl.conv_step[2], fl.steps);
            delete[] wheel; delete[] z;
        }
        delete[] x; delete[] P; delete[] u;
    }
    std::fclose(f);
    return 0;
}
