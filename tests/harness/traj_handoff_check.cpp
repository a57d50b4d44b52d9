// traj_handoff_check.cpp -- csrc/traj_handoff.h on the CPU (tests/test_traj_handoff_cpu.py builds it with the address and
// undefined-behaviour sanitizers and runs it as a child process).
// usage: traj_handoff_check FILE
// FILE: one request per line, answered by one line; doubles travel as hexadecimal floating point (%a), so every bit arrives:
//   P valid start now forced       -> promote_due: 0 | 1
//   S t0 dt_tick n k start...      -> split_run over k start times: the number of segments, then per segment
//                                     first count promote and the times of its ticks as the run bodies compute them
//                                     (tick_time(t0, dt_tick, first + j), j = 0 .. count - 1)
//   T now k start...               -> PendingTimes after add(start...): due(now), then the entries left after promoted(now)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../alore_legged_manipulator_amd/csrc/traj_handoff.h"

static bool read_doubles(std::FILE* f, int k, std::vector<double>& out)
{
    out.resize((size_t)k);
    for (int i = 0; i < k; ++i)
        if (std::fscanf(f, "%la", &out[(size_t)i]) != 1) return false;
    return true;
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    char kind[8];
    std::vector<double> starts;
    while (std::fscanf(f, "%7s", kind) == 1) {
        if (kind[0] == 'P') {
            int valid, forced;
            double start, now;
            if (std::fscanf(f, "%d %la %la %d", &valid, &start, &now, &forced) != 4) break;
            std::printf("%d\n", traj_handoff::promote_due(valid != 0, start, now, forced != 0) ? 1 : 0);
        } else if (kind[0] == 'S') {
            double t0, dt;
            int n, k;
            if (std::fscanf(f, "%la %la %d %d", &t0, &dt, &n, &k) != 4 || k < 0 || !read_doubles(f, k, starts)) break;
            const std::vector<traj_handoff::Segment> segs = traj_handoff::split_run(t0, dt, n, starts.data(), starts.size());
            std::printf("%zu", segs.size());
            for (const traj_handoff::Segment& g : segs) {
                std::printf(" %d %d %d", g.first, g.count, g.promote ? 1 : 0);
                for (int j = 0; j < g.count; ++j) std::printf(" %a", traj_handoff::tick_time(t0, dt, (long)g.first + j));
            }
            std::printf("\n");
        } else if (kind[0] == 'T') {
            double now;
            int k;
            if (std::fscanf(f, "%la %d", &now, &k) != 2 || k < 0 || !read_doubles(f, k, starts)) break;
            traj_handoff::PendingTimes p;
            for (double s : starts) p.add(s);
            std::printf("%d", p.due(now) ? 1 : 0);
            p.promoted(now);
            for (double s : p.t) std::printf(" %a", s);
            std::printf(" %d\n", p.any() ? 1 : 0);
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
