// nmpc_launch_plan.h -- launch planning of the stage-block kernel as pure functions (internal).
// Plain C++17: no HIP, no environment, no handle.  What a launch looks like -- geometry, stagger of the first residency, two-phase
// sizes, XCD shares, which build of the kernel -- is decided here from numbers alone; nmpc_capi.hip reads the environment and the
// handle, reserves what a plan needs and launches; nmpc_block_kernel.hip owns the kernels.  Diagnostic overrides that come from
// environment variables arrive as OptInt / OptDouble.  tests/harness/launch_plan_harness.cpp runs all of it on the CPU.
#ifndef ALORE_NMPC_LAUNCH_PLAN_H
#define ALORE_NMPC_LAUNCH_PLAN_H

#include <cmath>
#include <cstddef>

namespace nmpc {

struct OptInt { bool set = false; int value = 0; };
struct OptDouble { bool set = false; double value = 0.0; };

constexpr int TP_KMAX = 16; // two-phase grids: a tail workgroup reads the reports of its batch's blocks, up to 64 * TP_KMAX of them

struct LaunchGeom {
    int L;       // lanes per problem
    int G;       // problems per wavefront
    int wpb;     // wavefronts per workgroup (1 or 4)
    int wreg;    // 1: W_k of a stage lives in the registers of its lane, not in the LDS staging area
    int threads; // = L * G, multiple of 64
    int grid;
    int RS;      // wavefront kernel: LDS floats per problem; stage-block kernel: stages per lane (S)
    size_t lds_bytes;
    int block;   // 1: stage-block kernel (nmpc_block_kernel.hip), 0: wavefront kernel (nmpc_kernels.hip)
};

// LDS floats of one wavefront: W and y of its 64 / L problems, each area padded to whole 256-float DMA pieces
inline int block_lds_floats(int N, int L)
{
    const int G = 64 / L;
    return ((G * 25 * N + 255) & ~255) + ((G * 5 * N + 255) & ~255);
}

// (L, S) instantiated: (4, 5) (8, 3) (16, 2) (32, 1) for horizons up to 20 / 24 / 32 / 32, (16, 4) up to 64
inline bool block_geometry(int B, int N, int forced_L, int lds_limit_bytes, int n_cu, LaunchGeom* g, int B_in_flight = 0)
{
    if (B <= 0 || N <= 0) return false;
    const int cus = n_cu > 0 ? n_cu : 256;
    int L = forced_L;
    if (L == 0) {
        // the sweeps cost N scalar stage steps per wavefront whatever L is: spread a small batch over all SIMDs
        // (one wavefront each), pack a large one
        // (measured, profiles/r03_c_block_kernel_experiments.txt: two wavefronts on a SIMD do not issue faster than one,
        // so L = 32 only pays while every wavefront still has a CU to itself)
        // B_in_flight: problems of all launches that run concurrently with this one (alore_nmpc_rti_many) -- what fills
        // the chip is their sum
        const long Bo = (B_in_flight > B) ? B_in_flight : B;
        L = 16;
        while (L > 4 && (Bo + 64 / L - 1) / (64 / L) > 4L * cus) L >>= 1;
        while (L < 16 && N > L * (L == 4 ? 5 : 3)) L <<= 1;
        if (L == 16 && N <= 32 && (Bo + 1) / 2 <= (long)cus) L = 32;
        // (long horizons -- the reference's N = 50 -- stay on (16, 4): 8 lanes x 7 stages with W_k in registers instead of LDS was built in
        // round 6 and spills 880 registers: 49.6 against 35 us per batch in flight; what took (16, 4) to 26 us is the scan of nmpc_scan.h)
    }
    int S = 0;
    if (L == 4 && N <= 20) S = 5;
    else if (L == 8 && N <= 24) S = 3;
    else if (L == 16 && N <= 32) S = 2;
    else if (L == 16 && N <= 64) S = 4;
    else if (L == 32 && N <= 32) S = 1;
    if (S == 0) return false;
    const size_t lds = (size_t)block_lds_floats(N, L) * 4;
    if ((long)lds > lds_limit_bytes) return false;
    g->L = L;
    g->G = 64 / L;
    g->wpb = 1;
    g->wreg = 0;
    g->threads = 64;
    g->grid = (B + g->G - 1) / g->G;
    g->RS = S; // stages per lane
    g->lds_bytes = lds;
    g->block = 1;
    return true;
}

// Staggered start of the first residency (see the kernel): one wavefront per SIMD at this kernel's register count, spread over the
// time HBM needs for their inputs at ~5 TB/s; only for grids of at least two residencies.  `spread_ns`: diagnostic, total spread
// in ns (0 = off).
struct StaggerPlan { int stagger_blocks, stagger_x1024; };
inline StaggerPlan plan_stagger(int n_cu, int N, int G, int grid, int count, OptDouble spread_override_ns)
{
    StaggerPlan s{0, 0};
    const long resident = 4L * n_cu;
    const double bytes_per_block = 4.0 * (51.0 * N + 28.0) * G;
    // bytes / (7.5e12 B/s) in ns: 9 us for 1024 wavefronts x 67 KB (round 5, profiles/r05_b_stagger_and_pg_sweep.txt: 6 .. 11 us are
    // equally good, 0 costs 15 us per 20-batch grid, 14 and more 1 .. 3 us)
    double spread_ns = resident * bytes_per_block / 7.5e3;
    if (spread_override_ns.set) spread_ns = spread_override_ns.value;
    if ((long)grid * count >= 2 * resident && spread_ns > 0.0) {
        s.stagger_blocks = (int)resident;
        s.stagger_x1024 = (int)(spread_ns / 10.0 / resident * 1024.0 + 0.5); // ticks of 10 ns per block, x 1024
    }
    return s;
}

// may a grid of this geometry run in two phases (RtiGroup::tp_*)?
inline bool two_phase_supported(const LaunchGeom& g, int N, int n_sqp, bool stamp)
{
    return g.block && g.L == 4 && g.RS == 5 && N == 20 && n_sqp == 1 && !stamp && g.grid <= 64 * TP_KMAX;
}

// workgroups of a two-phase grid: units of (blocks of a batch, tail of the batch `lag` units before), see nmpc_block_body.inc
inline long long two_phase_blocks(int count, int count2, int lag, int grid, int tail)
{
    const long long units = (long long)count > (long long)count2 + lag ? (long long)count : (long long)count2 + lag;
    return units * ((long long)grid + tail);
}

// Two-phase grid (see the kernel): grids of several residencies of the (4, 5) grid build whose batches are many enough that the tail
// of a batch can follow its first pass at a distance of more than a residency and the last batches can run in one pass.
struct TwoPhaseIn {
    double tp_share;          // share of a batch's problems the tail is sized for
    int grid, G, count, n_cu;
    OptInt tail, lag, single; // diagnostic: tail workgroups per batch, units between a first pass and its tail, one-pass batches at the end
    bool wanted, conv, persistent, supported;
};
struct TwoPhasePlan {
    bool on;
    int tail, lag, count2;
    size_t queue_bytes; // exits (a line each), reports, entries
    long long blocks;   // workgroups launched
};
inline TwoPhasePlan plan_two_phase(const TwoPhaseIn& in)
{
    TwoPhasePlan t{false, 0, 0, 0, 0, 0};
    const long resident = 4L * in.n_cu;
    bool on = in.wanted && !in.conv && !in.persistent && in.supported && (long)in.grid * in.count >= 2 * resident;
    if (!on) return t;
    int tail = (int)std::ceil(in.tp_share * 1.08 * in.grid) + 3;
    if (in.tail.set) tail = in.tail.value;
    tail = tail < 1 ? 1 : (tail > in.grid ? in.grid : tail);
    const long unit = (long)in.grid + tail;
    int lag = (int)((resident + resident / 8 + unit - 1) / unit);
    if (in.lag.set) lag = in.lag.value;
    lag = lag < 1 ? 1 : lag;
    int single = lag;
    if (in.single.set) single = in.single.value;
    single = single < 0 ? 0 : single;
    const int count2 = in.count - single;
    on = count2 >= 1;
    if (!on) return t;
    t.on = true;
    t.tail = tail;
    t.lag = lag;
    t.count2 = count2;
    t.queue_bytes = (size_t)count2 * sizeof(int) * (16 + (size_t)in.grid * (1 + in.G));
    t.blocks = two_phase_blocks(in.count, count2, lag, in.grid, tail);
    return t;
}

// XCD shares (see the kernel).  The record a launch leaves: [8][4] finishing times (100 MHz counter) of the last four workgroups of
// every XCD, [32] its start.  An XCD that finished late is slower than its share assumed: the speeds move (damped), are normalised
// to mean 1 and kept within [0.85, 1.15].  false: the record says nothing (no start stamp, an end not after the start, or shorter
// than 10 us) and the speeds stay.
inline bool xcd_speed_update(const unsigned long long rec[40], double speed[8])
{
    const unsigned long long t0 = rec[32];
    double dur[8], mean = 0.0;
    bool ok = t0 != 0;
    for (int x = 0; x < 8 && ok; ++x) {
        unsigned long long e = 0;
        for (int i = 0; i < 4; ++i) e = rec[x * 4 + i] > e ? rec[x * 4 + i] : e;
        ok = e > t0;
        dur[x] = (double)(e - t0);
        mean += dur[x] / 8.0;
    }
    if (!(ok && mean > 1000.0)) return false; // 10 us of the 100 MHz counter: anything shorter says nothing
    double norm = 0.0;
    for (int x = 0; x < 8; ++x) {
        double v = speed[x] * std::pow(mean / dur[x], 0.7);
        speed[x] = v;
        norm += v / 8.0;
    }
    for (int x = 0; x < 8; ++x) {
        double v = speed[x] / norm;
        speed[x] = v < 0.85 ? 0.85 : (v > 1.15 ? 1.15 : v);
    }
    return true;
}

// Only grids of at least `min_res` residencies (default 12) and at least two.  A grid of five residencies ends when its last
// wavefronts end wherever the shares put them, and shares fitted on a long grid cost the next short one 3 % (20 batches right after
// 200: 142 us against 137.5 with equal shares, four runs each; repeated 20-batch grids: 132.4 - 134.2 with shares, 131.4 - 132.8
// without); the 200-batch grid keeps its 0.5 % (5.39 against 5.42 us per batch).  profiles/r06_contract_first_region.txt
inline bool xcd_shares_eligible(long total_items, int n_cu, long min_res)
{
    return total_items >= min_res * 4 * n_cu && total_items >= 2L * 4 * n_cu && total_items < (1L << 28);
}

// `total_items` blocks over the eight XCDs in proportion to their speeds, by largest remainder: XCD x works on share[x]
// consecutive blocks from base[x]
struct XcdPlan { int xcd_on; int share[8], base[8]; };
inline XcdPlan plan_xcd_shares(long total_items, const double speed[8])
{
    XcdPlan p{};
    double sum = 0.0;
    for (int x = 0; x < 8; ++x) sum += speed[x];
    long given = 0;
    double frac[8];
    for (int x = 0; x < 8; ++x) {
        const double want = (double)total_items * speed[x] / sum;
        p.share[x] = (int)want;
        frac[x] = want - (double)p.share[x];
        given += p.share[x];
    }
    while (given < total_items) { // the remainder to the largest fractions
        int bx = 0;
        for (int x = 1; x < 8; ++x) bx = frac[x] > frac[bx] ? x : bx;
        ++p.share[bx]; frac[bx] = -1.0; ++given;
    }
    while (given > total_items) { // rounding can only ever give too few; if it ever gave too many, the largest share gives them back
        int bx = 0;
        for (int x = 1; x < 8; ++x) bx = p.share[x] > p.share[bx] ? x : bx;
        --p.share[bx]; --given;
    }
    int base = 0;
    for (int x = 0; x < 8; ++x) { p.base[x] = base; base += p.share[x]; }
    p.xcd_on = base == total_items ? 1 : 0;
    return p;
}

// ---- which build of the kernel ---------------------------------------------------------------------------------------------------
// The template arguments of rti_block_kernel, spelt out.  kBlockBuilds is the whole set of instantiations: nmpc_block_kernel.hip makes
// its table of kernels from it, entry for entry, and a build's index here is its slot there.
struct BlockBuild {
    int L, S;
    bool DIAG, STAMP, ONCE, FULLN, TRACE, PERSIST, TWOPH, CONV;
};
constexpr bool operator==(const BlockBuild& a, const BlockBuild& b)
{
    return a.L == b.L && a.S == b.S && a.DIAG == b.DIAG && a.STAMP == b.STAMP && a.ONCE == b.ONCE && a.FULLN == b.FULLN && a.TRACE == b.TRACE &&
           a.PERSIST == b.PERSIST && a.TWOPH == b.TWOPH && a.CONV == b.CONV;
}
inline constexpr BlockBuild kBlockBuilds[] = {
    // every mapping: several iterations (with / without KKT value and objective), one iteration (with / without), phase stamps, converged solve
    //     DIAG   STAMP  ONCE   FULLN  TRACE  PERSIST TWOPH CONV
    {4, 5, true, false, false, false, false, false, false, false},
    {4, 5, false, false, false, false, false, false, false, false},
    {4, 5, true, false, true, false, false, false, false, false},
    {4, 5, false, false, true, false, false, false, false, false},
    {4, 5, true, true, false, false, false, false, false, false},
    {4, 5, true, false, false, false, false, false, false, true},
    {8, 3, true, false, false, false, false, false, false, false},
    {8, 3, false, false, false, false, false, false, false, false},
    {8, 3, true, false, true, false, false, false, false, false},
    {8, 3, false, false, true, false, false, false, false, false},
    {8, 3, true, true, false, false, false, false, false, false},
    {8, 3, true, false, false, false, false, false, false, true},
    {16, 2, true, false, false, false, false, false, false, false},
    {16, 2, false, false, false, false, false, false, false, false},
    {16, 2, true, false, true, false, false, false, false, false},
    {16, 2, false, false, true, false, false, false, false, false},
    {16, 2, true, true, false, false, false, false, false, false},
    {16, 2, true, false, false, false, false, false, false, true},
    {16, 4, true, false, false, false, false, false, false, false},
    {16, 4, false, false, false, false, false, false, false, false},
    {16, 4, true, false, true, false, false, false, false, false},
    {16, 4, false, false, true, false, false, false, false, false},
    {16, 4, true, true, false, false, false, false, false, false},
    {16, 4, true, false, false, false, false, false, false, true},
    {32, 1, true, false, false, false, false, false, false, false},
    {32, 1, false, false, false, false, false, false, false, false},
    {32, 1, true, false, true, false, false, false, false, false},
    {32, 1, false, false, true, false, false, false, false, false},
    {32, 1, true, true, false, false, false, false, false, false},
    {32, 1, true, false, false, false, false, false, false, true},
    // N = 20 on (4, 5), the horizon that fills the mapping (FULLN)
    {4, 5, true, false, true, true, false, false, false, false}, // the control tick
    {4, 5, false, false, true, true, false, false, false, false},
    {4, 5, true, false, false, true, false, false, false, false}, // several iterations per launch
    {4, 5, false, false, false, true, false, false, false, false},
    {4, 5, true, false, false, true, false, false, false, true}, // converged solve
    {4, 5, true, false, true, true, false, true, false, false}, // persistent grid
    {4, 5, false, false, true, true, false, true, false, false},
    {4, 5, true, false, true, true, false, false, true, false}, // two-phase grid
    {4, 5, false, false, true, true, false, false, true, false},
    {4, 5, true, false, true, true, true, false, false, false}, // instrumented twins of the tick and of the persistent grid (ALORE_NMPC_TRACE)
    {4, 5, true, false, true, true, true, true, false, false},
};
constexpr int kNumBlockBuilds = (int)(sizeof(kBlockBuilds) / sizeof(kBlockBuilds[0]));

// what a launch asks for.  diag: the batches carry kkt or obj; xcd_shares: the grid is dealt by XCD shares (RtiGroup::xcd_on)
struct BlockBuildRequest {
    int L, S, N, n_sqp;
    bool diag, stamp, conv, persist, twoph, trace;
    bool xcd_shares = false;
};
// index into kBlockBuilds, or -1: no such build
inline int select_block_build(const BlockBuildRequest& r)
{
    if (r.conv && (r.stamp || r.persist || r.twoph || r.trace)) return -1; // converged solve: the CONV builds only (a launch of one iteration too)
    const bool diag = r.diag || r.stamp;
    const bool once = r.n_sqp == 1 && !r.conv;
    const bool fulln = r.L == 4 && r.S == 5 && r.N == 20 && !r.stamp;
    const bool tick = fulln && once; // the control tick at the horizon that fills the (4, 5) mapping: what the grid builds are made of
    if (r.persist && !tick) return -1;
    if (r.twoph && (!tick || r.persist || r.trace || r.xcd_shares)) return -1;
    if (r.trace && !(tick && diag)) return -1; // diagnostic: only the grid builds have an instrumented twin
    const BlockBuild want = {r.L, r.S, diag || r.conv, r.stamp, once && !r.stamp, fulln, r.trace, r.persist, r.twoph, r.conv};
    for (int i = 0; i < kNumBlockBuilds; ++i)
        if (kBlockBuilds[i] == want) return i;
    return -1;
}

// The solve of one batch with the reference sampler's workgroups behind it in the same grid (rti_block_sampler_kernel)
struct SamplerBuild { int L, S; bool DIAG; };
inline constexpr SamplerBuild kSamplerBuilds[] = {{16, 2, true}, {16, 2, false}, {32, 1, true}, {32, 1, false}, {8, 3, true}, {8, 3, false}};
constexpr int kNumSamplerBuilds = (int)(sizeof(kSamplerBuilds) / sizeof(kSamplerBuilds[0]));
// 2: the sampler's workgroups run beside the solver's (builds of at most 256 registers: a SIMD holds one wavefront of each); 1: the
// grid carries the plant step only (the (8, 3) build takes 303 registers: the sampler's wavefronts would queue behind the solver's
// with one slot per SIMD -- as a kernel of its own the sampler has eight); 0: neither
inline int sampler_supported(const LaunchGeom& g, int N, int n_sqp, bool stamp)
{
    if (!(g.block && n_sqp == 1 && !stamp && N + 1 <= 32)) return 0;
    if ((g.L == 16 && g.RS == 2) || (g.L == 32 && g.RS == 1)) return 2;
    if (g.L == 8 && g.RS == 3) return 1;
    return 0;
}
// index into kSamplerBuilds, or -1: no such build
inline int select_sampler_build(const LaunchGeom& g, int N, int n_sqp, bool stamp, bool diag)
{
    if (sampler_supported(g, N, n_sqp, stamp) == 0) return -1;
    for (int i = 0; i < kNumSamplerBuilds; ++i)
        if (kSamplerBuilds[i].L == g.L && kSamplerBuilds[i].S == g.RS && kSamplerBuilds[i].DIAG == diag) return i;
    return -1;
}

} // namespace nmpc
#endif
