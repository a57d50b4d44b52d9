// ltv_plant_check.cpp -- csrc/ltv_plant.h on the CPU (tests/test_ltv_plant_cpu.py).
// usage: ltv_plant_check FILE
// FILE: one scene per line: max_acc max_domega pose_pub_period state_propa_period substeps follow  has_traj at_goal  cmd_v cmd_w
//       x y th v w dv dw  ticks
// Prints, per scene, `valid` (ltv_plant::valid of the parameters) and the state after `ticks` control periods.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ltv_plant.h"

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    for (;;) {
        alore_ltv_plant_params p;
        int has = 0, goal = 0, ticks = 0;
        double cv = 0.0, cw = 0.0;
        ltv_plant::State s;
        const int n = std::fscanf(f, "%lf %lf %lf %lf %d %d %d %d %lf %lf %lf %lf %lf %lf %lf %lf %lf %d", &p.max_acc, &p.max_domega, &p.pose_pub_period,
                                  &p.state_propa_period, &p.substeps, &p.follow, &has, &goal, &cv, &cw, &s.x, &s.y, &s.th, &s.v, &s.w, &s.dv, &s.dw, &ticks);
        if (n == EOF) break;
        if (n != 18) { std::fprintf(stderr, "malformed scene (%d fields)\n", n); std::fclose(f); return 2; }
        const bool ok = ltv_plant::valid(p);
        if (ok)
            for (int t = 0; t < ticks; ++t) ltv_plant::step(p, has != 0, goal != 0, cv, cw, s);
        std::printf("%d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", ok ? 1 : 0, s.x, s.y, s.th, s.v, s.w, s.dv, s.dw);
    }
    std::fclose(f);
    return 0;
}
