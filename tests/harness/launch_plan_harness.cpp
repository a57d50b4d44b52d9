// launch_plan_harness.cpp -- csrc/nmpc_launch_plan.h on the CPU (tests/test_launch_plan_cpu.py builds it with the address and
// undefined-behaviour sanitizers and reads what it prints).  One line per case: a tag, the inputs, '=', the results.
#include <cstdio>
#include <cstring>

#include "../../alore_legged_manipulator_amd/csrc/nmpc_launch_plan.h"

using namespace nmpc;

static void stagger(int n_cu, int N, int G, int grid, int count, OptDouble ns)
{
    const StaggerPlan s = plan_stagger(n_cu, N, G, grid, count, ns);
    std::printf("stagger %d %d %d %d %d %d %.17g = %d %d\n", n_cu, N, G, grid, count, (int)ns.set, ns.value, s.stagger_blocks, s.stagger_x1024);
}

static void two_phase(const char* name, TwoPhaseIn in)
{
    const TwoPhasePlan t = plan_two_phase(in);
    std::printf("two_phase %s = %d %d %d %d %zu %lld\n", name, (int)t.on, t.tail, t.lag, t.count2, t.queue_bytes, t.blocks);
}

static void xcd_plan(const char* name, long total, const double speed[8])
{
    const XcdPlan p = plan_xcd_shares(total, speed);
    std::printf("xcd_plan %s %ld", name, total);
    for (int x = 0; x < 8; ++x) std::printf(" %.17g", speed[x]);
    std::printf(" = %d", p.xcd_on);
    for (int x = 0; x < 8; ++x) std::printf(" %d", p.share[x]);
    for (int x = 0; x < 8; ++x) std::printf(" %d", p.base[x]);
    std::printf("\n");
}

static void xcd_update(const char* name, const unsigned long long rec[40], const double start[8], int rounds)
{
    double speed[8];
    std::memcpy(speed, start, sizeof speed);
    int used = 0;
    for (int r = 0; r < rounds; ++r) used += xcd_speed_update(rec, speed) ? 1 : 0;
    std::printf("xcd_update %s = %d", name, used);
    for (int x = 0; x < 8; ++x) std::printf(" %.17g", speed[x]);
    std::printf("\n");
}

static void record(unsigned long long rec[40], unsigned long long t0, const unsigned long long dur[8])
{
    std::memset(rec, 0, sizeof(unsigned long long) * 40);
    rec[32] = t0;
    for (int x = 0; x < 8; ++x)
        for (int i = 0; i < 4; ++i) rec[x * 4 + i] = t0 + dur[x] - (unsigned long long)(3 - i); // the last of the four is the latest
}

static void geometry(int B, int N, int n_cu, int in_flight)
{
    LaunchGeom g{};
    const bool ok = block_geometry(B, N, 0, 160 * 1024, n_cu, &g, in_flight);
    std::printf("geometry %d %d %d %d = %d %d %d %d %d %zu\n", B, N, n_cu, in_flight, (int)ok, g.L, g.RS, g.G, g.grid, g.lds_bytes);
}

int main()
{
    // stagger
    stagger(256, 20, 16, 256, 20, OptDouble{});
    stagger(256, 20, 16, 256, 7, OptDouble{});
    stagger(256, 20, 16, 256, 20, OptDouble{true, 0.0});
    stagger(256, 20, 16, 256, 20, OptDouble{true, 5000.0});
    stagger(256, 20, 16, 256, 8, OptDouble{});

    // two-phase
    const TwoPhaseIn base = {0.30, 256, 16, 20, 256, OptInt{}, OptInt{}, OptInt{}, true, false, false, true};
    TwoPhaseIn in = base;
    two_phase("default", in);
    in = base; in.count = 4; two_phase("count4", in);
    in = base; in.tail = OptInt{true, 1}; two_phase("tail1", in);
    in = base; in.tail = OptInt{true, 0}; two_phase("tail0", in);
    in = base; in.tail = OptInt{true, 100000}; two_phase("tail_huge", in);
    in = base; in.lag = OptInt{true, 0}; two_phase("lag0", in);
    in = base; in.lag = OptInt{true, -3}; two_phase("lag_neg", in);
    in = base; in.single = OptInt{true, -5}; two_phase("single_neg", in);
    in = base; in.single = OptInt{true, 2}; two_phase("single2", in);
    in = base; in.single = OptInt{true, 20}; two_phase("single_all", in);
    in = base; in.conv = true; two_phase("conv", in);
    in = base; in.persistent = true; two_phase("persistent", in);
    in = base; in.supported = false; two_phase("unsupported", in);
    in = base; in.wanted = false; two_phase("unwanted", in);
    in = base; in.count = 7; two_phase("one_residency", in);
    in = base; in.count = 3; in.lag = OptInt{true, 5}; in.single = OptInt{true, 0}; two_phase("lag_past_end", in);
    std::printf("two_phase_blocks = %lld %lld\n", two_phase_blocks(20, 16, 4, 256, 86), two_phase_blocks(3, 3, 5, 256, 86));
    {
        LaunchGeom g{};
        (void)block_geometry(4096, 20, 0, 160 * 1024, 256, &g, 4096 * 20);
        LaunchGeom big = g;
        big.grid = 64 * TP_KMAX + 1;
        LaunchGeom wave = g;
        wave.block = 0;
        std::printf("two_phase_supported = %d %d %d %d %d %d\n", (int)two_phase_supported(g, 20, 1, false), (int)two_phase_supported(g, 20, 2, false),
                    (int)two_phase_supported(g, 20, 1, true), (int)two_phase_supported(g, 19, 1, false), (int)two_phase_supported(big, 20, 1, false),
                    (int)two_phase_supported(wave, 20, 1, false));
    }

    // XCD apportionment
    const double ones[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    xcd_plan("equal", 12290, ones);
    std::printf("xcd_eligible = %d %d %d %d %d %d\n", (int)xcd_shares_eligible(12290, 256, 12), (int)xcd_shares_eligible(12288, 256, 12),
                (int)xcd_shares_eligible(12287, 256, 12), (int)xcd_shares_eligible(2047, 256, 0), (int)xcd_shares_eligible(2048, 256, 0),
                (int)xcd_shares_eligible(1L << 28, 256, 12));
    unsigned long long lcg = 0x9E3779B97F4A7C15ULL;
    for (int draw = 0; draw < 300; ++draw) {
        double speed[8];
        for (int x = 0; x < 8; ++x) {
            lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
            speed[x] = 0.85 + 0.30 * (double)(lcg >> 11) / 9007199254740992.0;
        }
        lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
        const long total = 2048 + (long)((lcg >> 33) % 300000);
        xcd_plan("draw", total, speed);
    }

    // XCD speed update
    unsigned long long rec[40];
    const unsigned long long t0 = 123456789ULL;
    const unsigned long long equal[8] = {20000, 20000, 20000, 20000, 20000, 20000, 20000, 20000};
    record(rec, t0, equal);
    xcd_update("equal", rec, ones, 1);
    const unsigned long long late[8] = {20000, 20000, 20000, 22000, 20000, 20000, 20000, 20000};
    record(rec, t0, late);
    xcd_update("late", rec, ones, 1);
    const unsigned long long very_late[8] = {20000, 20000, 20000, 60000, 20000, 20000, 20000, 20000};
    record(rec, t0, very_late);
    xcd_update("very_late", rec, ones, 1);
    xcd_update("very_late_x20", rec, ones, 20);
    const double skew[8] = {0.85, 1.15, 1.0, 1.1, 0.9, 1.0, 1.05, 0.95};
    record(rec, t0, late);
    rec[32] = 0;
    xcd_update("no_start", rec, skew, 1);
    record(rec, t0, late);
    for (int i = 0; i < 4; ++i) rec[5 * 4 + i] = t0; // an end stamp not after the start
    xcd_update("end_not_after_start", rec, skew, 1);
    const unsigned long long brief[8] = {1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000};
    record(rec, t0, brief);
    xcd_update("too_short", rec, skew, 1);

    // geometry
    geometry(4096, 20, 256, 4096 * 20);
    geometry(4096, 50, 256, 4096 * 20);
    geometry(1, 20, 256, 0);
    geometry(1, 65, 256, 0);
    geometry(4096, 24, 256, 4096 * 20);
    geometry(4096, 20, 256, 0);
    geometry(300, 20, 256, 0);
    std::printf("lds_floats = %d %d %d\n", block_lds_floats(20, 4), block_lds_floats(50, 16), block_lds_floats(20, 32));

    // selection
    std::printf("builds = %d %d\n", kNumBlockBuilds, kNumSamplerBuilds);
    const int maps[5][2] = {{4, 5}, {8, 3}, {16, 2}, {16, 4}, {32, 1}};
    const int Ns[3] = {20, 24, 50}, sqps[2] = {1, 15};
    for (const auto& m : maps)
        for (int N : Ns)
            for (int n_sqp : sqps)
                for (int f = 0; f < 128; ++f) { // bit 6: the grid is dealt by XCD shares
                    BlockBuildRequest r = {m[0], m[1], N, n_sqp, (f & 1) != 0, (f & 2) != 0, (f & 4) != 0, (f & 8) != 0, (f & 16) != 0, (f & 32) != 0};
                    r.xcd_shares = (f & 64) != 0;
                    const int i = select_block_build(r);
                    std::printf("select %d %d %d %d %d =", m[0], m[1], N, n_sqp, f);
                    if (i < 0) {
                        std::printf(" none\n");
                    } else {
                        const BlockBuild& b = kBlockBuilds[i];
                        std::printf(" %d %d %d %d %d %d %d %d %d %d %d\n", i, b.L, b.S, (int)b.DIAG, (int)b.STAMP, (int)b.ONCE, (int)b.FULLN, (int)b.TRACE,
                                    (int)b.PERSIST, (int)b.TWOPH, (int)b.CONV);
                    }
                }
    {
        BlockBuildRequest r = {8, 5, 20, 1, true, false, false, false, false, false};
        std::printf("select_unknown_mapping = %d\n", select_block_build(r));
    }
    for (int i = 0; i < kNumBlockBuilds; ++i) {
        const BlockBuild& b = kBlockBuilds[i];
        std::printf("build %d = %d %d %d %d %d %d %d %d %d %d\n", i, b.L, b.S, (int)b.DIAG, (int)b.STAMP, (int)b.ONCE, (int)b.FULLN, (int)b.TRACE, (int)b.PERSIST,
                    (int)b.TWOPH, (int)b.CONV);
    }
    for (int i = 0; i < kNumSamplerBuilds; ++i)
        std::printf("sampler_build %d = %d %d %d\n", i, kSamplerBuilds[i].L, kSamplerBuilds[i].S, (int)kSamplerBuilds[i].DIAG);
    const int sampler_Ns[3] = {20, 31, 32};
    for (const auto& m : maps)
        for (int N : sampler_Ns)
            for (int n_sqp : sqps)
                for (int f = 0; f < 8; ++f) { // stamp, diag, wavefront kernel
                    LaunchGeom g{};
                    g.L = m[0]; g.RS = m[1]; g.block = (f & 4) ? 0 : 1;
                    std::printf("sampler %d %d %d %d %d = %d %d\n", m[0], m[1], N, n_sqp, f, sampler_supported(g, N, n_sqp, (f & 1) != 0),
                                select_sampler_build(g, N, n_sqp, (f & 1) != 0, (f & 2) != 0));
                }
    return 0;
}
