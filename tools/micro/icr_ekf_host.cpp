// icr_ekf_host.cpp -- csrc/icr_ekf.h on one host core (tools/icr_ekf.py): B robots, `steps` filter steps each (a pose update on
// every `every`-th), wheel speeds and poses from a small generator; prints the nanoseconds per robot-step and a checksum.
//   usage: icr_ekf_host B steps every
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icr_ekf.h"

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const int B = std::atoi(argv[1]), steps = std::atoi(argv[2]), every = std::atoi(argv[3]);
    if (B < 1 || steps < 1 || every < 1) return 2;
    const icrekf::Params p = {{0.5, 0.5, 1.14, 0.1, 0.1, 0.1}, {0.1, 0.1, 0.1}, {-0.3, 0.3, 0.2}};
    std::vector<double> x((size_t)B * 6), P((size_t)B * 36, 0.0), u((size_t)B * 2, 0.0);
    std::vector<icrekf::Flags> f(B);
    for (int b = 0; b < B; ++b) {
        const double x0[6] = {0.01 * b, -0.02 * b, 0.001 * b, -0.25, 0.25, 0.1};
        for (int i = 0; i < 6; ++i) x[(size_t)b * 6 + i] = x0[i];
        icrekf::reset_flags(f[b]);
    }
    int bad = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int s = 0; s < steps; ++s)
        for (int b = 0; b < B; ++b) {
            const double w = 0.5 + 0.001 * (s % 100), wheel[2] = {1.0 - 0.3 * w, 1.0 + 0.3 * w};
            const double* xb = &x[(size_t)b * 6];
            const double z[3] = {xb[0] + 0.001, xb[1] - 0.001, xb[2] + 0.0005};
            bad += icrekf::step_one(p, &x[(size_t)b * 6], &P[(size_t)b * 36], &u[(size_t)b * 2], f[b], wheel, 0.01, z, (s + 1) % every == 0, nullptr) != icrekf::OK;
        }
    const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
    double sum = 0.0;
    for (double v : x) sum += v;
    std::printf("%.4g %d %.17g\n", ns / ((double)B * steps), bad, sum);
    return 0;
}
