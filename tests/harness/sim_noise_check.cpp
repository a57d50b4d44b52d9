// sim_noise_check.cpp -- csrc/sim_noise.h and ltv_plant::step_noisy on the CPU (tests/test_sim_noise_cpu.py).
// usage: sim_noise_check FILE
// FILE: one request per line, answered by one line:
//   P c0 c1 c2 c3 k0 k1 (hex)                  -> the four output words of Philox4x32-10 (hex)
//   W seed robot event stream (decimal)        -> the four words (hex), u1, u2, z0, z1
//   U wa wb (hex)                              -> sim_noise::uniform
//   S max_acc max_domega pose_pub_period state_propa_period substeps follow  has_traj at_goal  cmd_v cmd_w  x y th v w dv dw
//     stddev seed robot event ticks            -> the state after `ticks` noisy control periods (event advances by one per period),
//                                                 then 1 / 0: with stddev == 0, are these the bits of ltv_plant::step? (-1: not asked)
//                                                 (step() is step_noisy with the noise off, so 1 by construction; what checks
//                                                 sigma = 0 is the oracle's plain plant_step, which the test compares the state with)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ltv_plant.h"

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    char kind[8];
    while (std::fscanf(f, "%7s", kind) == 1) {
        if (kind[0] == 'P') {
            uint32_t c[4], k[2], o[4];
            if (std::fscanf(f, "%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &c[0], &c[1], &c[2], &c[3], &k[0], &k[1]) != 6) break;
            sim_noise::philox4x32(c, k, o);
            std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", o[0], o[1], o[2], o[3]);
        } else if (kind[0] == 'W') {
            uint64_t seed, event;
            uint32_t robot, stream, w[4];
            if (std::fscanf(f, "%" SCNu64 " %" SCNu32 " %" SCNu64 " %" SCNu32, &seed, &robot, &event, &stream) != 4) break;
            sim_noise::words(seed, robot, event, stream, w);
            double z0, z1;
            sim_noise::normal2(seed, robot, event, stream, z0, z1);
            std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %.17g %.17g %.17g %.17g\n", w[0], w[1], w[2], w[3],
                        sim_noise::uniform(w[0], w[1]), sim_noise::uniform(w[2], w[3]), z0, z1);
        } else if (kind[0] == 'U') {
            uint32_t wa, wb;
            if (std::fscanf(f, "%" SCNx32 " %" SCNx32, &wa, &wb) != 2) break;
            std::printf("%.17g\n", sim_noise::uniform(wa, wb));
        } else if (kind[0] == 'S') {
            alore_ltv_plant_params p;
            int has = 0, goal = 0, ticks = 0;
            double cv = 0.0, cw = 0.0;
            ltv_plant::State s;
            ltv_plant::Noise n;
            const int got = std::fscanf(f, "%lf %lf %lf %lf %d %d %d %d %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %" SCNu64 " %" SCNu32 " %" SCNu64 " %d",
                                        &p.max_acc, &p.max_domega, &p.pose_pub_period, &p.state_propa_period, &p.substeps, &p.follow, &has, &goal,
                                        &cv, &cw, &s.x, &s.y, &s.th, &s.v, &s.w, &s.dv, &s.dw, &n.stddev, &n.seed, &n.robot, &n.event, &ticks);
            if (got != 22 || !ltv_plant::valid(p)) { std::fprintf(stderr, "malformed scene (%d fields)\n", got); std::fclose(f); return 2; }
            ltv_plant::State plain = s;
            for (int t = 0; t < ticks; ++t) {
                ltv_plant::step_noisy(p, has != 0, goal != 0, cv, cw, n, s);
                ltv_plant::step(p, has != 0, goal != 0, cv, cw, plain);
                n.event += 1;
            }
            const double a[7] = {s.x, s.y, s.th, s.v, s.w, s.dv, s.dw}, b[7] = {plain.x, plain.y, plain.th, plain.v, plain.w, plain.dv, plain.dw};
            const int same = n.stddev == 0.0 ? (std::memcmp(a, b, sizeof(a)) == 0 ? 1 : 0) : -1;
            std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g %d\n", s.x, s.y, s.th, s.v, s.w, s.dv, s.dw, same);
        } else {
            std::fprintf(stderr, "unknown request %s\n", kind);
            std::fclose(f);
            return 2;
        }
    }
    if (!std::feof(f)) { std::fprintf(stderr, "malformed request\n"); std::fclose(f); return 2; }
    std::fclose(f);
    return 0;
}
