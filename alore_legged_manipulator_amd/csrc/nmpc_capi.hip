// nmpc_capi.hip -- implementation of the C ABI declared in include/alore_nmpc.h.
// Thin host layer: argument checks, launch geometry, HIP stream/event plumbing.
// There is no CPU path behind this ABI: without a GPU alore_nmpc_create fails.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <new>
#include <string>

#include "nmpc_solver.h"
#include "nmpc_core.h"

using namespace nmpc_capi;

extern "C" {

const char* alore_nmpc_version(void) { return "alore_nmpc 0.1 (gfx950)"; }

int alore_nmpc_create(const alore_nmpc_config* cfg, alore_nmpc_handle* out)
{
    if (!cfg || !out) return ALORE_NMPC_E_INVALID;
    *out = nullptr;
    if (cfg->N < 1 || !(cfg->dt > 0.0f)) return ALORE_NMPC_E_INVALID;
    {
        const int lp = cfg->lanes_per_problem, lw = lp & ~0x100;
        const bool blk = (lp & 0x100) != 0;
        if (lp != 0 && !(blk ? (lw == 4 || lw == 8 || lw == 16 || lw == 32) : (lw == 4 || lw == 8 || lw == 16 || lw == 32 || lw == 64)))
            return ALORE_NMPC_E_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ALORE_NMPC_E_NO_DEVICE;
    if (cfg->device < 0 || cfg->device >= ndev) return ALORE_NMPC_E_INVALID;
    if (hipSetDevice(cfg->device) != hipSuccess) return ALORE_NMPC_E_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return ALORE_NMPC_E_NO_DEVICE;
    alore_nmpc_solver* h = new (std::nothrow) alore_nmpc_solver;
    if (!h) return ALORE_NMPC_E_NOMEM;
    h->cfg = *cfg;
    if (h->cfg.max_as_iter <= 0) h->cfg.max_as_iter = 128;
    h->auto_pg = h->cfg.warm_start_steps < 0;
    // swept on MI355X: N = 20 -- 4 / 6 / 8 steps: 23.8 / 21.8 / 22.6 us per in-order launch of 4096; N = 50 (round 6, with the scanned backward
    // sweep a prediction step is cheap beside a second sweep) -- 4 / 6 / 8 / 10: 52.4 / 48.8 / 45.7 / 47.8 us (tools/horizon_in_flight.py)
    if (h->auto_pg) h->cfg.warm_start_steps = h->cfg.N > 32 ? 8 : 6;
    h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    h->lds_limit = (int)prop.sharedMemPerBlock > 0 ? (int)prop.sharedMemPerBlock : 64 * 1024;
    if (prop.maxSharedMemoryPerMultiProcessor > (size_t)h->lds_limit)
        h->lds_limit = (int)prop.maxSharedMemoryPerMultiProcessor;
    if (h->lds_limit > 160 * 1024) h->lds_limit = 160 * 1024;
    // the horizon must fit the on-chip layout with at least one geometry
    nmpc::LaunchGeom g;
    const bool fits = (cfg->lanes_per_problem & 0x100)
                          ? nmpc::block_geometry(1, cfg->N, cfg->lanes_per_problem & 0xff, h->lds_limit, h->n_cu, &g)
                          : nmpc::rti_geometry(1, cfg->N, cfg->lanes_per_problem, h->lds_limit, h->n_cu, &g);
    if (!fits) {
        delete h;
        return ALORE_NMPC_E_UNSUPPORTED;
    }
    if (hipEventCreate(&h->timing.ev0) != hipSuccess || hipEventCreate(&h->timing.ev1) != hipSuccess) {
        delete h;
        return ALORE_NMPC_E_HIP;
    }
    // streams / events of alore_nmpc_rti_many: made here, not at first use, so that a first use inside a stream capture
    // creates nothing
    bool forks_ok = hipEventCreateWithFlags(&h->forks.fork_ev, hipEventDisableTiming) == hipSuccess;
    for (int w = 0; w < 31 && forks_ok; ++w)
        forks_ok = hipStreamCreateWithFlags(&h->forks.side[w], hipStreamNonBlocking) == hipSuccess &&
                   hipEventCreateWithFlags(&h->forks.join_ev[w], hipEventDisableTiming) == hipSuccess;
    if (!forks_ok) {
        (void)alore_nmpc_destroy(h);
        return ALORE_NMPC_E_HIP;
    }
    if (hipMalloc((void**)&h->tickets.d_tickets, sizeof(int) * 2 * alore_nmpc_solver::Tickets::kRing) != hipSuccess ||
        hipMemset(h->tickets.d_tickets, 0, sizeof(int) * 2 * alore_nmpc_solver::Tickets::kRing) != hipSuccess) {
        (void)alore_nmpc_destroy(h);
        return ALORE_NMPC_E_HIP;
    }
    if (hipHostMalloc((void**)&h->xcd.rec, sizeof(unsigned long long) * 40, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&h->xcd.ev, hipEventDisableTiming) != hipSuccess) {
        (void)alore_nmpc_destroy(h);
        return ALORE_NMPC_E_HIP;
    }
    std::memset(h->xcd.rec, 0, sizeof(unsigned long long) * 40);
    if (hipHostMalloc((void**)&h->tp.rec, sizeof(int) * 40, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&h->tp.rec_ev, hipEventDisableTiming) != hipSuccess) {
        (void)alore_nmpc_destroy(h);
        return ALORE_NMPC_E_HIP;
    }
    std::memset(h->tp.rec, 0, sizeof(int) * 40);
    for (int i = 0; i < alore_nmpc_solver::TwoPhaseRing::kRing; ++i)
        if (hipEventCreateWithFlags(&h->tp.ev[i], hipEventDisableTiming) != hipSuccess) {
            (void)alore_nmpc_destroy(h);
            return ALORE_NMPC_E_HIP;
        }
    if (const char* sp = std::getenv("ALORE_NMPC_XCD_SPEEDS")) { // diagnostic / tests: preset relative speeds "a,b,c,d,e,f,g,h"
        double v[8];
        if (std::sscanf(sp, "%lf,%lf,%lf,%lf,%lf,%lf,%lf,%lf", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7) == 8)
            for (int x = 0; x < 8; ++x) h->xcd.speed[x] = v[x] > 0.05 ? v[x] : 0.05;
    }
    const char* st = std::getenv("ALORE_NMPC_STAMPS");
    h->stamps.on = st && st[0] == '1';
    *out = h;
    return ALORE_NMPC_OK;
}

int alore_nmpc_destroy(alore_nmpc_handle h)
{
    if (!h) return ALORE_NMPC_E_INVALID;
    h->stamps.release();
    h->tickets.release();
    h->xcd.release();
    h->tp.release();
    h->forks.release();
    h->refs.release();
    h->handoff.release();
    h->poly.release();
    h->timing.release();
    h->pinned.release();
    h->ekf.release();
    delete h;
    return ALORE_NMPC_OK;
}

const char* alore_nmpc_last_error(alore_nmpc_handle h) { return h ? h->err.c_str() : "null handle"; }

int alore_nmpc_batch_alloc(alore_nmpc_handle h, int B, alore_nmpc_batch* out)
{
    if (!h || !out || B <= 0) return fail(h, ALORE_NMPC_E_INVALID, "batch_alloc: bad argument");
    std::memset(out, 0, sizeof(*out));
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    for (int i = 0; i < kNumMembers; ++i) {
        const Member& m = kMembers[i];
        const size_t bytes = (size_t)B * m.per_problem(h->cfg.N) * 4;
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            alore_nmpc_batch_free(h, out);
            return fail(h, ALORE_NMPC_E_NOMEM, "hipMalloc", e);
        }
        (void)hipMemset(p, 0, bytes);
        member_ptr(out, m) = p;
    }
    return ALORE_NMPC_OK;
}

int alore_nmpc_batch_free(alore_nmpc_handle h, alore_nmpc_batch* b)
{
    if (!h || !b) return ALORE_NMPC_E_INVALID;
    for (int i = 0; i < kNumMembers; ++i) {
        void*& p = member_ptr(b, kMembers[i]);
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    return ALORE_NMPC_OK;
}

// Pageable host members go through one pinned staging buffer per direction (a hipMemcpyAsync from pageable memory
// is staged by the runtime in 4 MB pieces with a host wait per piece: 2-3 x slower and never asynchronous);
// members already in pinned memory (alore_nmpc_host_alloc) are copied in place.
static int batch_copy(alore_nmpc_handle h, const alore_nmpc_batch* dev, const alore_nmpc_batch* host, int B,
                      void* stream, bool to_device)
{
    if (!h || !dev || !host || B <= 0) return fail(h, ALORE_NMPC_E_INVALID, "batch copy: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    size_t staged = 0;
    bool pinned[kNumMembers];
    for (int i = 0; i < kNumMembers; ++i) {
        const Member& m = kMembers[i];
        void* hp = member_ptr(host, m);
        pinned[i] = false;
        if (!member_ptr(dev, m) || !hp) continue;
        pinned[i] = host_is_pinned(hp);
        if (!pinned[i]) staged += (((size_t)B * m.per_problem(h->cfg.N) * 4) + 255) & ~(size_t)255;
    }
    char* stage = nullptr;
    if (staged) {
        if (to_device) {
            if (h->pinned.up_done) HIP_TRY(h, hipEventSynchronize(h->pinned.up_done)); // the previous upload still reads it
            if (int rc = grow_stage(h, h->pinned.up, h->pinned.up_cap, staged)) return rc;
            stage = h->pinned.up;
        } else {
            if (int rc = grow_stage(h, h->pinned.down, h->pinned.down_cap, staged)) return rc;
            stage = h->pinned.down;
        }
    }
    size_t off = 0;
    for (int i = 0; i < kNumMembers; ++i) {
        const Member& m = kMembers[i];
        void* d = member_ptr(dev, m);
        void* hp = member_ptr(host, m);
        if (!d || !hp) continue;
        const size_t bytes = (size_t)B * m.per_problem(h->cfg.N) * 4;
        void* src_dst = hp;
        if (!pinned[i]) {
            src_dst = stage + off;
            off += (bytes + 255) & ~(size_t)255;
            if (to_device) std::memcpy(src_dst, hp, bytes);
        }
        if (to_device)
            HIP_TRY(h, hipMemcpyAsync(d, src_dst, bytes, hipMemcpyHostToDevice, s));
        else
            HIP_TRY(h, hipMemcpyAsync(src_dst, d, bytes, hipMemcpyDeviceToHost, s));
    }
    if (staged && to_device) {
        if (!h->pinned.up_done) HIP_TRY(h, hipEventCreateWithFlags(&h->pinned.up_done, hipEventDisableTiming));
        HIP_TRY(h, hipEventRecord(h->pinned.up_done, s));
    }
    if (staged && !to_device) { // pageable destinations: complete the transfer, then hand the data over
        HIP_TRY(h, hipStreamSynchronize(s));
        off = 0;
        for (int i = 0; i < kNumMembers; ++i) {
            const Member& m = kMembers[i];
            void* hp = member_ptr(host, m);
            if (!member_ptr(dev, m) || !hp || pinned[i]) continue;
            const size_t bytes = (size_t)B * m.per_problem(h->cfg.N) * 4;
            std::memcpy(hp, stage + off, bytes);
            off += (bytes + 255) & ~(size_t)255;
        }
    }
    return ALORE_NMPC_OK;
}

int alore_nmpc_host_alloc(size_t bytes, void** out)
{
    if (!out || bytes == 0) return ALORE_NMPC_E_INVALID;
    *out = nullptr;
    return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? ALORE_NMPC_OK : ALORE_NMPC_E_NOMEM;
}

int alore_nmpc_host_free(void* p)
{
    if (!p) return ALORE_NMPC_OK;
    return hipHostFree(p) == hipSuccess ? ALORE_NMPC_OK : ALORE_NMPC_E_HIP;
}

int alore_nmpc_batch_upload(alore_nmpc_handle h, const alore_nmpc_batch* dev, const alore_nmpc_batch* host, int B,
                            void* stream)
{
    return batch_copy(h, dev, host, B, stream, true);
}

int alore_nmpc_batch_download(alore_nmpc_handle h, const alore_nmpc_batch* dev, const alore_nmpc_batch* host, int B,
                              void* stream)
{
    return batch_copy(h, dev, host, B, stream, false);
}

int alore_nmpc_batch_default_bounds(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, void* stream)
{
    if (!h || !dev || B <= 0 || !dev->lbValues || !dev->ubValues)
        return fail(h, ALORE_NMPC_E_INVALID, "default_bounds: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t n = (size_t)B * h->cfg.N * 2;
    HIP_TRY(h, nmpc::launch_fill(const_cast<float*>(dev->lbValues), -3.0f, n, (hipStream_t)stream));
    HIP_TRY(h, nmpc::launch_fill(const_cast<float*>(dev->ubValues), 3.0f, n, (hipStream_t)stream));
    return ALORE_NMPC_OK;
}

} // extern "C"

namespace {

// may this batch run on the stage-block kernel (nmpc_block_kernel.hip)?  Not when the caller forces lanes of the wavefront
// kernel, a separate linearisation point is set, or a member is not 16-byte aligned.
bool block_eligible(alore_nmpc_handle h, const alore_nmpc_batch* dev)
{
    static const char* force_kernel = getenv("ALORE_NMPC_KERNEL"); // diagnostic: "wave" or "block"
    const int lp = h->cfg.lanes_per_problem;
    bool ok = (lp == 0 || (lp & 0x100)) && !(force_kernel && force_kernel[0] == 'w') && !h->lin_x;
    const void* ptrs[] = {dev->x, dev->u, dev->od, dev->y, dev->W, dev->lbValues, dev->ubValues, dev->dual};
    for (const void* q : ptrs) ok = ok && ((reinterpret_cast<size_t>(q) & 15) == 0);
    return ok;
}

void fill_params(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, int n_sqp, const nmpc::LaunchGeom& g, nmpc::RtiParams* p)
{
    p->b = *dev;
    p->B = B;
    p->N = h->cfg.N;
    p->n_sqp = n_sqp;
    p->max_as_iter = h->cfg.max_as_iter;
    p->pg_steps = h->cfg.warm_start_steps;
    p->shared = h->shared;
    static const bool no_scan = getenv("ALORE_NMPC_SCAN") && atoi(getenv("ALORE_NMPC_SCAN")) == 0; // diagnostic: backward sweeps never as a scan over the lanes
    if (no_scan) p->shared |= 0x80000000u;
    p->RS = g.RS;
    const nmpc::IrkConst K = nmpc::make_irk(h->cfg.dt);
    p->h = K.h; p->hh = K.hh; p->c1h = K.c1h; p->c2h = K.c2h;
    p->stamps = nullptr;
    p->lin_x = h->lin_x;
    p->lin_u = h->lin_u;
    p->mask = nullptr;
    p->kkt_tol = h->conv_tol;
    p->sqp_iters = (h->conv_tol >= 0.0f && h->conv_iters) ? h->conv_iters + (size_t)h->conv_row * B : nullptr;
}

// several batches in one grid (below); rti_one hands it a batch that is a grid of several residencies by itself
int rti_group(alore_nmpc_handle h, const alore_nmpc_batch* batches, int count, int B, int n_sqp, void* stream, int B_in_flight,
              const long long* stride);

} // namespace

// (declared in nmpc_solver.h: alore_nmpc_closed_loop_run of nmpc_refs_capi.hip calls it too)
int nmpc_capi::rti_one(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, int n_sqp, void* stream, int B_in_flight, const nmpc::AheadSampler* co,
                       bool* co_done, const nmpc::PlantAhead* plant)
{
    if (co_done) *co_done = false;
    if (!batch_complete(dev)) return fail(h, ALORE_NMPC_E_INVALID, "rti: batch has NULL members");
    nmpc::LaunchGeom g;
    static const int forced_wpb = getenv("ALORE_NMPC_WPB") ? atoi(getenv("ALORE_NMPC_WPB")) : 0; // diagnostic: 1 or 4
    const int lp = h->cfg.lanes_per_problem;
    const bool use_block = block_eligible(h, dev) &&
                           nmpc::block_geometry(B, h->cfg.N, lp & 0xff, h->lds_limit, h->n_cu, &g, B_in_flight);
    if (!use_block && !nmpc::rti_geometry(B, h->cfg.N, (lp & 0x100) ? 0 : lp, h->lds_limit, h->n_cu, &g, forced_wpb))
        return fail(h, ALORE_NMPC_E_UNSUPPORTED, "rti: horizon does not fit the LDS layout");
    nmpc::RtiParams p;
    fill_params(h, dev, B, n_sqp, g, &p);
    p.mask = h->mask;
    // one robot / a handful (a few wavefronts, each alone on its SIMD): a second, partial sweep costs less than the prediction steps that
    // would avoid it -- B = 1, N = 20, cold start, synchronous launch p50: 3 / 4 / 6 / 8 steps 22.7 / 23.6 / 23.8 / 24.8 us (round 6)
    if (h->auto_pg && B <= 64 && h->cfg.N <= 32) p.pg_steps = 3;
    hipStream_t s = (hipStream_t)stream;
    const bool stamps = h->stamps.on && p.kkt_tol < 0.0f; // converged solves have no stamped build
    if (stamps) {
        const size_t need = (size_t)g.grid * g.wpb * 8; // one record per wavefront
        if (need > h->stamps.cap) {
            if (h->stamps.d_stamps) (void)hipFree(h->stamps.d_stamps);
            h->stamps.d_stamps = nullptr;
            h->stamps.cap = 0;
            HIP_TRY(h, hipMalloc((void**)&h->stamps.d_stamps, need * sizeof(long long)));
            h->stamps.cap = need;
        }
        p.stamps = h->stamps.d_stamps;
    }
    if (h->timing.on) HIP_TRY(h, hipEventRecord(h->timing.ev0, s));
    // one batch that is a grid of several residencies by itself (B >= 32768 on the packed mapping): what alore_nmpc_rti_many gives the
    // batches of a call -- staggered first residency, XCD shares, the prediction length of a full chip -- applies to it as it stands
    static const bool big_as_group = !(getenv("ALORE_NMPC_BIG_AS_GROUP") && atoi(getenv("ALORE_NMPC_BIG_AS_GROUP")) == 0);
    const int fused = (co && !h->timing.on) ? nmpc::rti_block_sampler_supported(p, g) : 0;
    if (big_as_group && use_block && g.L == 4 && g.RS == 5 && !stamps && !co && !plant && (long)g.grid >= 2L * 4 * h->n_cu) {
        if (const int rc = rti_group(h, dev, 1, B, n_sqp, stream, B, nullptr)) return rc;
    } else if (fused == 2 || (fused == 1 && plant)) {
        nmpc::AheadSampler sa = *co;
        if (fused == 1) sa.B = 0; // this build has no room for the sampler's wavefronts: the caller launches it behind the solve
        HIP_TRY(h, nmpc::launch_rti_block_sampler(p, g, sa, plant, s));
        *co_done = fused == 2 || co->B == 0;
    } else {
        if (plant) HIP_TRY(h, nmpc::launch_plant_ahead(*plant, s)); // no build of this mapping carries it: its own launch, in front of the solve
        HIP_TRY(h, g.block ? nmpc::launch_rti_block(p, g, s) : nmpc::launch_rti(p, g, s));
    }
    if (h->timing.on) {
        HIP_TRY(h, hipEventRecord(h->timing.ev1, s));
        h->timing.pending = true;
    }
    h->last_geom = g;
    h->have_geom = true;
    if (stamps) { // diagnostic mode: synchronous, never used for timing
        const int n_waves = g.grid * g.wpb;
        std::vector<long long> host((size_t)n_waves * 8);
        HIP_TRY(h, hipStreamSynchronize(s));
        HIP_TRY(h, hipMemcpy(host.data(), h->stamps.d_stamps, host.size() * sizeof(long long), hipMemcpyDeviceToHost));
        if (const char* dump = getenv("ALORE_NMPC_STAMPS_DUMP")) { // raw per-wavefront stamps of the last launch
            if (FILE* f = std::fopen(dump, "wb")) { std::fwrite(host.data(), sizeof(long long), host.size(), f); std::fclose(f); }
        }
        for (int b = 0; b < n_waves; ++b) {
            for (int i = 0; i < 7; ++i) h->stamps.sum[i] += (double)host[(size_t)b * 8 + i];
            for (int i = 0; i < 7; ++i)
                if ((double)host[(size_t)b * 8 + i] > h->stamps.max[i]) h->stamps.max[i] = (double)host[(size_t)b * 8 + i];
            if ((double)host[(size_t)b * 8 + 5] > h->stamps.max_total) {
                h->stamps.max_total = (double)host[(size_t)b * 8 + 5];
                for (int i = 0; i < 7; ++i) h->stamps.slowest[i] = (double)host[(size_t)b * 8 + i];
            }
        }
        h->stamps.n += n_waves;
    }
    return ALORE_NMPC_OK;
}

namespace {

// Are the batches independent problem sets?  Every array a batch WRITES (x, u, dual, status, n_iter, kkt, obj) must be
// disjoint, as an address range, from every array another batch reads or writes.  One sort of the 15 x count ranges and a
// sweep that remembers, for writes and for all ranges, the two furthest-reaching ranges of distinct batches.
bool batches_independent(alore_nmpc_handle h, const alore_nmpc_batch* batches, int count, int B)
{
    struct Range { size_t lo, hi; int id; bool write; };
    std::vector<Range> r;
    r.reserve((size_t)count * kNumMembers);
    const int N = h->cfg.N;
    for (int i = 0; i < count; ++i) {
        for (int m = 0; m < kNumMembers; ++m) {
            const void* q = member_ptr(batches + i, kMembers[m]);
            if (!q) continue;
            const size_t off = kMembers[m].offset;
            const bool write = off == offsetof(alore_nmpc_batch, x) || off == offsetof(alore_nmpc_batch, u) ||
                               off == offsetof(alore_nmpc_batch, dual) || off == offsetof(alore_nmpc_batch, status) ||
                               off == offsetof(alore_nmpc_batch, n_iter) || off == offsetof(alore_nmpc_batch, kkt) ||
                               off == offsetof(alore_nmpc_batch, obj);
            bool one_copy = false; // members that are ONE copy for the batch (alore_nmpc_set_shared_members)
            if (h->shared & ALORE_NMPC_SHARED_W) one_copy = one_copy || off == offsetof(alore_nmpc_batch, W) || off == offsetof(alore_nmpc_batch, WN);
            if (h->shared & ALORE_NMPC_SHARED_BOUNDS) one_copy = one_copy || off == offsetof(alore_nmpc_batch, lbValues) || off == offsetof(alore_nmpc_batch, ubValues);
            if (h->shared & ALORE_NMPC_SHARED_OD) one_copy = one_copy || off == offsetof(alore_nmpc_batch, od);
            const size_t bytes = (size_t)(one_copy ? 1 : B) * kMembers[m].per_problem(N) * 4;
            const size_t lo = reinterpret_cast<size_t>(q);
            r.push_back({lo, lo + bytes, i, write});
        }
    }
    std::sort(r.begin(), r.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
    struct Top2 { size_t hi[2] = {0, 0}; int id[2] = {-1, -1};
        void add(size_t h_, int i_) {
            if (i_ == id[0]) { if (h_ > hi[0]) hi[0] = h_; }
            else if (h_ > hi[0]) { if (id[0] != -1) { hi[1] = hi[0]; id[1] = id[0]; } hi[0] = h_; id[0] = i_; }
            else if (i_ == id[1]) { if (h_ > hi[1]) hi[1] = h_; }
            else if (h_ > hi[1]) { hi[1] = h_; id[1] = i_; }
        }
        bool other_reaches(size_t lo, int i_) const { return (id[0] != -1 && id[0] != i_ && hi[0] > lo) || (id[1] != -1 && id[1] != i_ && hi[1] > lo); }
    } writes, all;
    for (const Range& q : r) {
        if (writes.other_reaches(q.lo, q.id)) return false;          // somebody else writes into what this batch touches
        if (q.write && all.other_reaches(q.lo, q.id)) return false;  // this batch writes into what somebody else touches
        all.add(q.hi, q.id);
        if (q.write) writes.add(q.hi, q.id);
    }
    return true;
}

// Is (batches, count) a contiguous run of the descriptor set that last passed the check, for the same B and shared members?  The
// descriptors are compared, not a digest of them.
bool known_independent(alore_nmpc_handle h, const alore_nmpc_batch* batches, int count, int B)
{
    for (int k = 0; k < alore_nmpc_solver::IndepCache::kSets; ++k) {
        const size_t n = h->indep.set[k].size();
        if (n == 0 || (size_t)count > n || h->indep.B[k] != B || h->indep.shared[k] != h->shared) continue;
        for (size_t i0 = 0; i0 + (size_t)count <= n; ++i0)
            if (h->indep.set[k][i0].x == batches[0].x && std::memcmp(&h->indep.set[k][i0], batches, (size_t)count * sizeof(alore_nmpc_batch)) == 0) {
                h->indep.used[k] = ++h->indep.clock;
                return true;
            }
    }
    return false;
}
void remember_independent(alore_nmpc_handle h, const alore_nmpc_batch* batches, int count, int B)
{
    int k = 0;
    for (int i = 1; i < alore_nmpc_solver::IndepCache::kSets; ++i)
        if (h->indep.used[i] < h->indep.used[k]) k = i;
    h->indep.set[k].assign(batches, batches + count);
    h->indep.B[k] = B;
    h->indep.shared[k] = h->shared;
    h->indep.used[k] = ++h->indep.clock;
}

// Converged solves: does the iteration-count array of the call ([count][B] ints) stay clear of every array of every batch?  (Its rows
// are disjoint by construction; one pass over the 15 x count ranges.)
bool iters_independent(alore_nmpc_handle h, const alore_nmpc_batch* batches, int count, int B)
{
    const size_t lo = reinterpret_cast<size_t>(h->conv_iters), hi = lo + (size_t)count * B * sizeof(int);
    const int N = h->cfg.N;
    for (int i = 0; i < count; ++i) {
        for (int m = 0; m < kNumMembers; ++m) {
            const void* q = member_ptr(batches + i, kMembers[m]);
            if (!q) continue;
            const size_t a = reinterpret_cast<size_t>(q), b = a + (size_t)B * kMembers[m].per_problem(N) * 4; // (a shared member's one copy lies inside)
            if (a < hi && lo < b) return false;
        }
    }
    return true;
}

nmpc::OptInt env_int(const char* v)
{
    nmpc::OptInt o;
    if (v) { o.set = true; o.value = atoi(v); }
    return o;
}

// The record of the last two-phase grid, once that grid has finished: the fullest queue sizes the next tail.  An error it left (a tail
// workgroup gave up waiting): the queues are put back in order and the call fails loudly.
int tp_take_record(alore_nmpc_handle h, int B)
{
    if (!(h->tp.rec_pending && hipEventQuery(h->tp.rec_ev) == hipSuccess)) return ALORE_NMPC_OK;
    h->tp.rec_pending = false;
    if (h->tp.rec[32] != 0) {
        const int code = h->tp.rec[32];
        h->tp.rec[32] = 0;
        (void)hipDeviceSynchronize();
        for (int i = 0; i < alore_nmpc_solver::TwoPhaseRing::kRing; ++i)
            if (h->tp.queue[i]) (void)hipMemset(h->tp.queue[i], 0, h->tp.cap[i]);
        char msg[256];
        std::snprintf(msg, sizeof msg, "rti_many: a tail workgroup of the previous two-phase grid gave up waiting for its queue (code %d); "
                                       "that grid left problems unsolved (alore_nmpc_set_two_phase(h, 0) turns the mode off)", code);
        return fail(h, ALORE_NMPC_E_HIP, msg);
    }
    int mx = 0;
    for (int i = 0; i < 32; ++i) mx = h->tp.rec[i] > mx ? h->tp.rec[i] : mx;
    if (mx > 0) h->tp.share = (double)mx / (double)B; // the fullest queue of the last grid
    return ALORE_NMPC_OK;
}

// What the two-phase plan is made from.  alore_nmpc_set_two_phase / ALORE_NMPC_TWO_PHASE (diagnostic): 0 never, 1 wherever the build exists.
nmpc::TwoPhaseIn two_phase_request(alore_nmpc_handle h, const nmpc::RtiParams& p, const nmpc::LaunchGeom& g, int count, bool conv, bool persistent)
{
    static const char* env_tp = getenv("ALORE_NMPC_TWO_PHASE");
    static const char* env_lag = getenv("ALORE_NMPC_TP_LAG");       // diagnostic: units between a first pass and its tail
    static const char* env_single = getenv("ALORE_NMPC_TP_SINGLE"); // diagnostic: batches at the end of the grid that run in one pass
    static const char* env_tail = getenv("ALORE_NMPC_TP_TAIL");     // diagnostic: tail workgroups per batch
    // automatic = off: measured on the bench distribution (a fifth of the problems queued) the mode loses 8 % -- the queued problems pay
    // the 5 - 9 us between a workgroup's start and its inputs a second time (profiles/r06_two_phase.txt); it gains below ~a tenth queued
    const int want = env_tp ? atoi(env_tp) : (h->tp.mode < 0 ? 0 : h->tp.mode);
    nmpc::TwoPhaseIn in{};
    in.tp_share = h->tp.share;
    in.grid = g.grid; in.G = g.G; in.count = count; in.n_cu = h->n_cu;
    in.tail = env_int(env_tail); in.lag = env_int(env_lag); in.single = env_int(env_single);
    in.wanted = want != 0; in.conv = conv; in.persistent = persistent;
    in.supported = nmpc::rti_block_two_phase_supported(p, g);
    return in;
}

// A queue region of `need` bytes for a two-phase grid on stream `s`: the next of the ring whose last user is this stream or has
// finished, grown if it is too small (never inside a capture).  -1: none to be had, the grid runs in one phase.
int tp_acquire_slot(alore_nmpc_handle h, hipStream_t s, size_t need, bool capturing)
{
    for (int tries = 0; tries < alore_nmpc_solver::TwoPhaseRing::kRing; ++tries) {
        const int i = (int)(h->tp.turn++ % alore_nmpc_solver::TwoPhaseRing::kRing);
        if (h->tp.used[i] && h->tp.stream[i] != s && hipEventQuery(h->tp.ev[i]) != hipSuccess) continue;
        if (h->tp.cap[i] < need) {
            if (capturing) continue; // no allocation inside a capture
            if (h->tp.used[i]) (void)hipEventSynchronize(h->tp.ev[i]);
            if (h->tp.queue[i]) (void)hipFree(h->tp.queue[i]);
            h->tp.queue[i] = nullptr; h->tp.cap[i] = 0; h->tp.used[i] = false;
            const size_t want_bytes = need + need / 4;
            if (hipMalloc((void**)&h->tp.queue[i], want_bytes) != hipSuccess) { (void)hipGetLastError(); continue; }
            if (hipMemset(h->tp.queue[i], 0, want_bytes) != hipSuccess) { (void)hipFree(h->tp.queue[i]); h->tp.queue[i] = nullptr; continue; }
            h->tp.cap[i] = want_bytes;
        }
        return i;
    }
    return -1;
}

// Diagnostic launches (never under a stream capture): the grid runs synchronously with a buffer of `words` words at *buf (a member of
// `grp`) that its workgroups fill; the buffer goes to the file <path>.<n>, n counting the traced grids of that path, behind `hdr`.
int traced_launch(alore_nmpc_handle h, const nmpc::RtiParams& p, nmpc::RtiGroup& grp, const nmpc::LaunchGeom& g, hipStream_t s, long long** buf,
                  size_t words, const long long (&hdr)[8], const char* path, int* seq, const char* what)
{
    long long* d_trace = nullptr;
    HIP_TRY(h, hipMalloc((void**)&d_trace, words * sizeof(long long)));
    *buf = d_trace;
    hipError_t e = hipMemsetAsync(d_trace, 0, words * sizeof(long long), s);
    if (e == hipSuccess) e = nmpc::launch_rti_block_group(p, grp, g, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    std::vector<long long> host(words);
    if (e == hipSuccess) e = hipMemcpy(host.data(), d_trace, words * sizeof(long long), hipMemcpyDeviceToHost);
    (void)hipFree(d_trace);
    if (e != hipSuccess) return fail(h, ALORE_NMPC_E_HIP, what, e);
    const std::string fname = std::string(path) + "." + std::to_string((*seq)++);
    if (FILE* f = std::fopen(fname.c_str(), "wb")) {
        std::fwrite(hdr, sizeof(long long), 8, f);
        std::fwrite(host.data(), sizeof(long long), host.size(), f);
        std::fclose(f);
    }
    return ALORE_NMPC_OK;
}

// `count` independent batches on the stage-block kernel as ONE grid (nmpc_block_kernel.hip: RtiGroup): by table
// (count <= GROUP_MAX) or, with `stride`, by constant member strides (any count).
// Geometry and parameters; the plans (nmpc_launch_plan.h: stagger, two phases, XCD shares); what a plan needs reserved; one launch;
// the events that mark its records pending.
int rti_group(alore_nmpc_handle h, const alore_nmpc_batch* batches, int count, int B, int n_sqp, void* stream, int B_in_flight,
              const long long* stride)
{
    // 1. geometry and parameters
    nmpc::LaunchGeom g;
    if (!nmpc::block_geometry(B, h->cfg.N, h->cfg.lanes_per_problem & 0xff, h->lds_limit, h->n_cu, &g, B_in_flight))
        return fail(h, ALORE_NMPC_E_UNSUPPORTED, "rti_many: horizon does not fit the stage-block kernel");
    hipStream_t s = (hipStream_t)stream;
    nmpc::RtiParams p;
    fill_params(h, batches, B, n_sqp, g, &p);
    p.mask = h->mask; // problem b of EVERY batch of the call (alore_nmpc_set_problem_mask)
    // a launch on its own lasts as long as its slowest wavefront, so the prediction runs until (nearly) no problem needs a
    // second sweep (6 .. 9 steps); when the chip is full of wavefronts the 2 % of problems that get one with 3 .. 4 steps cost
    // less than the steps saved (profiles/r04_block_kernel_experiments.txt)
    if (h->auto_pg && (long)B * count >= 16384) p.pg_steps = 4; // round 5 (a prediction step costs 443 instructions, was 573): 2 / 3 / 4 / 5 / 6 steps: 5.97 / 5.61 / 5.50 / 5.72 / 6.20 us per batch
    const bool conv = p.kkt_tol >= 0.0f; // converged solve: none of the persistent, two-phase or traced builds exists for it
    const bool tick_build = g.L == 4 && g.RS == 5 && h->cfg.N == 20 && n_sqp == 1; // the build that fills the (4, 5) mapping: what the grid modes are made for
    const long total_items = (long)g.grid * count;
    nmpc::RtiGroup grp;
    grp.count = count;
    grp.blocks_per_batch = g.grid;
    grp.strided = stride ? 1 : 0;
    if (stride) for (int m = 0; m < 15; ++m) grp.stride[m] = stride[m];
    const int n_tab = stride ? 1 : count;
    for (int i = 0; i < n_tab; ++i) grp.b[i] = batches[i];
    int capture = -1; // the stream's capture status, asked for once and only if something depends on it
    auto capturing = [&] {
        if (capture < 0) {
            hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
            (void)hipStreamIsCapturing(s, &cap);
            capture = cap == hipStreamCaptureStatusNone ? 0 : 1;
        }
        return capture == 1;
    };

    // 2. the plans
    static const char* env_ns = getenv("ALORE_NMPC_STAGGER_NS"); // diagnostic: total spread in ns (0 = off)
    nmpc::OptDouble spread_ns;
    if (env_ns) { spread_ns.set = true; spread_ns.value = atof(env_ns); }
    const nmpc::StaggerPlan stagger = nmpc::plan_stagger(h->n_cu, h->cfg.N, g.G, g.grid, count, spread_ns);
    grp.stagger_blocks = stagger.stagger_blocks;
    grp.stagger_x1024 = stagger.stagger_x1024;
    // ALORE_NMPC_PERSIST=1 (measured alternative, off by default): grids of at least two residencies of the build that fills the
    // (4, 5) mapping run persistent -- one workgroup per SIMD slot, blocks of problems taken by ticket (see the kernel).  It evens out
    // the XCDs (the hardware deals a plain grid to them in fixed shares and they differ by ~5 % in speed: tail 3.6 -> 1.4 % of a
    // 200-batch grid), but the loop around the body costs the register allocation more than that: profiles/r05_persistent_grid.txt
    static const bool persist_on = getenv("ALORE_NMPC_PERSIST") && atoi(getenv("ALORE_NMPC_PERSIST")) == 1;
    const bool persistent = persist_on && !conv && tick_build && total_items >= 2L * 4 * h->n_cu;
    h->tp.last = 0;
    if (const int rc = tp_take_record(h, B)) return rc;
    const nmpc::TwoPhasePlan tp = nmpc::plan_two_phase(two_phase_request(h, p, g, count, conv, persistent));
    // XCD shares (see the kernel): grids of enough residencies of the build that fills the (4, 5) mapping, neither persistent nor in two
    // phases (decided below, once the two-phase grid has its queue).  ALORE_NMPC_XCD_SHARES=0 (diagnostic): equal shares, as the hardware deals them.
    static const bool xcd_shares_on = !(getenv("ALORE_NMPC_XCD_SHARES") && atoi(getenv("ALORE_NMPC_XCD_SHARES")) == 0);
    static const long xcd_min_res = getenv("ALORE_NMPC_XCD_MIN_RES") ? atol(getenv("ALORE_NMPC_XCD_MIN_RES")) : 12;

    // 3. what the plans need: the ticket pair, the queue slot, the host records
    if (persistent) { // a ring of pairs, one per launch in turn
        grp.counter = h->tickets.d_tickets + 2 * (h->tickets.turn++ % alore_nmpc_solver::Tickets::kRing);
        grp.persist_blocks = 4 * h->n_cu;
    }
    const int slot = tp.on ? tp_acquire_slot(h, s, tp.queue_bytes, capturing()) : -1;
    if (slot >= 0) {
        grp.tp_count2 = tp.count2;
        grp.tp_tail = tp.tail;
        grp.tp_lag = tp.lag;
        grp.tp_timeout = 20 * 1000 * 100; // 20 ms of the 100 MHz counter
        grp.tp_exits = reinterpret_cast<int*>(h->tp.queue[slot]);
        grp.tp_cnt = grp.tp_exits + (size_t)tp.count2 * 16;
        grp.tp_entries = grp.tp_cnt + (size_t)tp.count2 * g.grid;
        if (!capturing() && !h->tp.rec_pending) { // the record: eager launches only, one in flight at a time
            std::memset(h->tp.rec, 0, sizeof(int) * 40);
            void* alias = nullptr;
            if (hipHostGetDevicePointer(&alias, h->tp.rec, 0) == hipSuccess) grp.tp_rec = (int*)alias;
        }
        h->tp.used[slot] = true;
        h->tp.stream[slot] = s;
        h->tp.last = 1;
        h->tp.info[0] = tp.count2; h->tp.info[1] = tp.tail; h->tp.info[2] = tp.lag;
    }
    h->tp.slot_of_launch = slot;
    if (xcd_shares_on && !persistent && slot < 0 && tick_build && nmpc::xcd_shares_eligible(total_items, h->n_cu, xcd_min_res)) {
        // the record of the previous such launch, if it has finished, moves the speed estimates; this launch leaves its own record
        // unless the previous one is still being written (then: the shares as they are, no new record)
        bool record = true;
        if (h->xcd.pending) {
            if (hipEventQuery(h->xcd.ev) == hipSuccess) {
                if (nmpc::xcd_speed_update(h->xcd.rec, h->xcd.speed)) ++h->xcd.updates;
                h->xcd.pending = false;
            } else {
                record = false;
            }
        }
        const nmpc::XcdPlan xp = nmpc::plan_xcd_shares(total_items, h->xcd.speed);
        grp.xcd_on = xp.xcd_on;
        std::memcpy(grp.xcd_share, xp.share, sizeof xp.share);
        std::memcpy(grp.xcd_base, xp.base, sizeof xp.base);
        // never inside a stream capture: every replay would write the host record with no event to tell when
        if (record && !capturing()) {
            std::memset(h->xcd.rec, 0, sizeof(unsigned long long) * 40);
            void* alias = nullptr;
            if (hipHostGetDevicePointer(&alias, h->xcd.rec, 0) == hipSuccess) grp.xcd_end = (unsigned long long*)alias;
        }
    }

    // 4. one launch.  Diagnostic twins (synchronous, a file per grid): ALORE_NMPC_TRACE=<file> -- 8 words per workgroup of the grid
    // build (real-time counter at start / after the stagger / inputs landed / last store / stores acknowledged, HW_ID, sweeps, diagonal
    // path; tools/trace_timeline.py); ALORE_NMPC_TP_TRACE=<file> -- 4 words per workgroup of a two-phase grid (real-time counter at
    // its start / inputs landed / end, its role; tools/tp_trace.py)
    static const char* trace_path = getenv("ALORE_NMPC_TRACE");
    static const char* tp_trace_path = getenv("ALORE_NMPC_TP_TRACE");
    static int trace_seq = 0, tp_trace_seq = 0;
    const bool traced = trace_path && !conv && slot < 0 && tick_build && batches[0].kkt && batches[0].obj;
    const bool tp_traced = !traced && tp_trace_path && slot >= 0;
    if (traced) {
        const long long hdr[8] = {0x4543415254LL /* "TRACE" */, (long long)g.grid * count, count, g.grid, grp.stagger_blocks, grp.stagger_x1024, p.pg_steps, 0};
        if (const int rc = traced_launch(h, p, grp, g, s, &grp.trace, (size_t)g.grid * count * 8, hdr, trace_path, &trace_seq, "rti_many: traced launch")) return rc;
    } else if (tp_traced) {
        const long long hdr[8] = {0x5054LL, tp.blocks, count, g.grid, grp.tp_count2, grp.tp_tail, grp.tp_lag, 0};
        if (const int rc = traced_launch(h, p, grp, g, s, &grp.tp_trace, (size_t)tp.blocks * 4, hdr, tp_trace_path, &tp_trace_seq, "rti_many: traced two-phase launch")) return rc;
    } else {
        HIP_TRY(h, nmpc::launch_rti_block_group(p, grp, g, s));
    }

    // 5. the events that mark this launch's records pending: eager launches only.  (A traced grid has been waited for: its queue slot is
    // free and its XCD record -- the instrumented build's -- is not used.)
    if (slot >= 0 && !traced && !capturing()) {
        if (!tp_traced) (void)hipEventRecord(h->tp.ev[slot], s);
        if (grp.tp_rec && hipEventRecord(h->tp.rec_ev, s) == hipSuccess) h->tp.rec_pending = true;
    }
    if (grp.xcd_end && !traced && !capturing() && hipEventRecord(h->xcd.ev, s) == hipSuccess) h->xcd.pending = true;
    h->last_geom = g;
    h->last_geom.grid = g.grid * count;
    h->have_geom = true;
    return ALORE_NMPC_OK;
}

// Do the batches sit at constant strides -- batch i = batch 0 with every member pointer advanced by i * stride[member] bytes
// (the slots of one arena, the slices of one tensor per member)?  stride[] in the member order of alore_nmpc_batch.
bool constant_strides(const alore_nmpc_batch* batches, int count, long long* stride)
{
    if (count < 2) return false;
    const char* const* p0 = reinterpret_cast<const char* const*>(batches);
    const char* const* p1 = reinterpret_cast<const char* const*>(batches + 1);
    for (int m = 0; m < 15; ++m) {
        if ((p0[m] == nullptr) != (p1[m] == nullptr)) return false;
        stride[m] = p0[m] ? (long long)(p1[m] - p0[m]) : 0;
    }
    for (int i = 2; i < count; ++i) {
        const char* const* pi = reinterpret_cast<const char* const*>(batches + i);
        for (int m = 0; m < 15; ++m) {
            if ((pi[m] == nullptr) != (p0[m] == nullptr)) return false;
            if (p0[m] && pi[m] != p0[m] + (long long)i * stride[m]) return false;
        }
    }
    return true;
}

} // namespace

extern "C" {

int alore_nmpc_rti(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, int n_sqp, void* stream)
{
    if (!h || !dev || B <= 0 || n_sqp < 1) return fail(h, ALORE_NMPC_E_INVALID, "rti: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return rti_one(h, dev, B, n_sqp, stream, 0);
}

int alore_nmpc_rti_many(alore_nmpc_handle h, const alore_nmpc_batch* batches, int count, int B, int n_sqp, void* stream)
{
    if (!h || !batches || count < 1 || B <= 0 || n_sqp < 1) return fail(h, ALORE_NMPC_E_INVALID, "rti_many: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    for (int i = 0; i < count; ++i)
        if (!batch_complete(batches + i)) return fail(h, ALORE_NMPC_E_INVALID, "rti_many: batch has NULL members");
    // Independent batches (checked: address ranges) are kept in flight together.  Default: GROUPS -- up to GROUP_MAX batches
    // per grid of the stage-block kernel (one launch, one graph node, no ramp and drain between the batches; the lane
    // mapping is chosen for all problems of the grid).  alore_nmpc_set_many_mode(h, 1): STREAMS -- one launch per batch,
    // round-robin over `overlap` internal streams forked from and joined back into the caller's (the round-3 form; also
    // what batches that cannot use the stage-block kernel get).  A batch listed twice (successive iterations of the same
    // problems), overlap = 1 or per-launch timing keep the launches in order on `stream`.
    int ways = h->overlap;
    if (const char* e = std::getenv("ALORE_NMPC_OVERLAP")) ways = std::atoi(e);
    ways = ways < 1 ? 1 : (ways > 32 ? 32 : ways);
    if (ways > count) ways = count;
    if (ways > 1 && h->stamps.on) ways = 1;
    if (ways > 1 && h->timing.on && h->many_mode != 0) ways = 1; // per-launch timing of the streams mode: in order; the groups mode times its grid(s) as one
    if (ways > 1) {
        // the independence check (a sort of 15 x count address ranges) is remembered for the descriptor set it passed on: a host
        // that steps the same slots every tick pays for it once (alore_nmpc_rti_many_prepare: before the first tick)
        if (!known_independent(h, batches, count, B)) {
            if (batches_independent(h, batches, count, B)) remember_independent(h, batches, count, B);
            else ways = 1;
        }
        // a converged solve also writes its iteration counts: they must not overlap any array of the call either
        if (ways > 1 && h->conv_tol >= 0.0f && h->conv_iters && !iters_independent(h, batches, count, B)) ways = 1;
    }
    if (ways == 1) {
        for (int i = 0; i < count; ++i) {
            h->conv_row = i;
            const int rc = rti_one(h, batches + i, B, n_sqp, stream, 0);
            if (rc != ALORE_NMPC_OK) return rc;
        }
        return ALORE_NMPC_OK;
    }
    int mode = h->many_mode;
    if (const char* e = std::getenv("ALORE_NMPC_MANY")) mode = (e[0] == 's') ? 1 : 0; // diagnostic: "streams" / "groups"
    bool groups = mode == 0;
    if (groups) {
        nmpc::LaunchGeom g;
        groups = nmpc::block_geometry(B, h->cfg.N, h->cfg.lanes_per_problem & 0xff, h->lds_limit, h->n_cu, &g, B);
        for (int i = 0; i < count && groups; ++i)
            groups = block_eligible(h, batches + i) && (batches[i].kkt != nullptr) == (batches[0].kkt != nullptr) &&
                     (batches[i].obj != nullptr) == (batches[0].obj != nullptr);
    }
    hipStream_t main_s = (hipStream_t)stream;
    const long clampB = 0x7fffffffL;
    if (groups) {
        // Batches at constant strides (the slots of one arena): ONE grid for all of them, whatever their number.  Otherwise
        // equal groups of at most GROUP_MAX batches (descriptor table in the kernel arguments), one grid each, in order on the
        // caller's stream.  ALORE_NMPC_GROUP_STREAMS=2 (diagnostic): successive table groups alternate between the caller's
        // stream and one side stream so that the tail of one grid runs under the head of the next.
        long long stride[15];
        nmpc::LaunchGeom g1;
        (void)nmpc::block_geometry(B, h->cfg.N, h->cfg.lanes_per_problem & 0xff, h->lds_limit, h->n_cu, &g1, B);
        if (constant_strides(batches, count, stride) && (long long)g1.grid * count <= 0x7fffffffLL) {
            const long inflight = (long)B * count;
            // alore_nmpc_set_timing: HIP events on the launch stream directly around the grid (alore_nmpc_get_launch_info: last_kernel_ms is
            // then the duration of the ONE grid that served the `count` batches)
            if (h->timing.on) HIP_TRY(h, hipEventRecord(h->timing.ev0, main_s));
            h->conv_row = 0;
            const int rc = rti_group(h, batches, count, B, n_sqp, stream, (int)(inflight > clampB ? clampB : inflight), stride);
            if (h->timing.on && rc == ALORE_NMPC_OK) {
                HIP_TRY(h, hipEventRecord(h->timing.ev1, main_s));
                h->timing.pending = true;
            }
            return rc;
        }
        static const bool alternate = getenv("ALORE_NMPC_GROUP_STREAMS") && atoi(getenv("ALORE_NMPC_GROUP_STREAMS")) == 2;
        const int n_groups = (count + nmpc::GROUP_MAX - 1) / nmpc::GROUP_MAX;
        const int per = (count + n_groups - 1) / n_groups;
        const bool two = alternate && n_groups > 1;
        const long inflight = (long)B * per * (two ? 2 : 1);
        const int Bf = (int)(inflight > clampB ? clampB : inflight);
        // alore_nmpc_set_timing: the events go on the caller's stream around ALL grids of the call (in front of the fork, behind the join)
        if (h->timing.on) HIP_TRY(h, hipEventRecord(h->timing.ev0, main_s));
        if (two) {
            HIP_TRY(h, hipEventRecord(h->forks.fork_ev, main_s));
            HIP_TRY(h, hipStreamWaitEvent(h->forks.side[0], h->forks.fork_ev, 0));
        }
        int rc = ALORE_NMPC_OK;
        for (int gi = 0, first = 0; first < count && rc == ALORE_NMPC_OK; ++gi, first += per) {
            const int n = (count - first < per) ? count - first : per;
            h->conv_row = first;
            rc = rti_group(h, batches + first, n, B, n_sqp, (two && (gi & 1)) ? (void*)h->forks.side[0] : (void*)main_s, Bf, nullptr);
        }
        if (two) { // join even after a failed launch: the side stream must not stay forked (an open capture would be lost)
            const hipError_t e1 = hipEventRecord(h->forks.join_ev[0], h->forks.side[0]);
            const hipError_t e2 = hipStreamWaitEvent(main_s, h->forks.join_ev[0], 0);
            if (rc == ALORE_NMPC_OK && e1 != hipSuccess) return fail(h, ALORE_NMPC_E_HIP, "rti_many: join", e1);
            if (rc == ALORE_NMPC_OK && e2 != hipSuccess) return fail(h, ALORE_NMPC_E_HIP, "rti_many: join", e2);
        }
        if (h->timing.on && rc == ALORE_NMPC_OK) {
            HIP_TRY(h, hipEventRecord(h->timing.ev1, main_s));
            h->timing.pending = true;
        }
        return rc;
    }
    // STREAMS.  With timing on the launches of this path never fork (rti_one records the handle's ONE pair of events: two of them on
    // different streams would pair events of different launches): in order on the caller's stream.
    if (h->timing.on) {
        for (int i = 0; i < count; ++i) {
            h->conv_row = i;
            const int rc1 = rti_one(h, batches + i, B, n_sqp, stream, 0);
            if (rc1 != ALORE_NMPC_OK) return rc1;
        }
        return ALORE_NMPC_OK;
    }
    HIP_TRY(h, hipEventRecord(h->forks.fork_ev, main_s));
    int forked = 0;
    int rc = ALORE_NMPC_OK;
    for (int w = 1; w < ways && rc == ALORE_NMPC_OK; ++w) {
        const hipError_t e = hipStreamWaitEvent(h->forks.side[w - 1], h->forks.fork_ev, 0);
        if (e != hipSuccess) rc = fail(h, ALORE_NMPC_E_HIP, "rti_many: fork", e);
        else forked = w;
    }
    const long inflight = (long)B * ways;
    const int Bf = (int)(inflight > clampB ? clampB : inflight); // the automatic lane mapping packs for all of them
    for (int i = 0; i < count && rc == ALORE_NMPC_OK; ++i) {
        const int w = i % ways;
        h->conv_row = i;
        rc = rti_one(h, batches + i, B, n_sqp, w == 0 ? (void*)main_s : (void*)h->forks.side[w - 1], Bf);
    }
    for (int w = 1; w <= forked; ++w) { // join every forked stream, whatever happened above
        const hipError_t e1 = hipEventRecord(h->forks.join_ev[w - 1], h->forks.side[w - 1]);
        const hipError_t e2 = hipStreamWaitEvent(main_s, h->forks.join_ev[w - 1], 0);
        if (rc == ALORE_NMPC_OK && e1 != hipSuccess) rc = fail(h, ALORE_NMPC_E_HIP, "rti_many: join", e1);
        if (rc == ALORE_NMPC_OK && e2 != hipSuccess) rc = fail(h, ALORE_NMPC_E_HIP, "rti_many: join", e2);
    }
    return rc;
}

namespace {
// the converge request of one call: on the handle while the launches are enqueued (fill_params reads it), gone when the call returns
struct ConvScope {
    alore_nmpc_handle h;
    ConvScope(alore_nmpc_handle h_, float tol, int* iters) : h(h_) { h->conv_tol = tol; h->conv_iters = iters; h->conv_row = 0; }
    ~ConvScope() { h->conv_tol = -1.0f; h->conv_iters = nullptr; h->conv_row = 0; }
};
} // namespace

int alore_nmpc_rti_converge(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, int max_sqp, float kkt_tol, int* sqp_iters, void* stream)
{
    if (!h || !dev || B <= 0 || max_sqp < 1 || !(kkt_tol >= 0.0f)) return fail(h, ALORE_NMPC_E_INVALID, "rti_converge: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    ConvScope cs(h, kkt_tol, sqp_iters);
    return rti_one(h, dev, B, max_sqp, stream, 0);
}

int alore_nmpc_rti_many_converge(alore_nmpc_handle h, const alore_nmpc_batch* batches, int count, int B, int max_sqp, float kkt_tol,
                                 int* sqp_iters, void* stream)
{
    if (!h || !batches || count < 1 || B <= 0 || max_sqp < 1 || !(kkt_tol >= 0.0f))
        return fail(h, ALORE_NMPC_E_INVALID, "rti_many_converge: bad argument");
    ConvScope cs(h, kkt_tol, sqp_iters);
    return alore_nmpc_rti_many(h, batches, count, B, max_sqp, stream);
}

int alore_nmpc_synchronize(alore_nmpc_handle h, void* stream)
{
    if (!h) return ALORE_NMPC_E_INVALID;
    HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));
    return ALORE_NMPC_OK;
}

int alore_nmpc_rti_many_prepare(alore_nmpc_handle h, const alore_nmpc_batch* batches, int count, int B)
{
    if (!h || !batches || count < 1 || B <= 0) return fail(h, ALORE_NMPC_E_INVALID, "rti_many_prepare: bad argument");
    for (int i = 0; i < count; ++i)
        if (!batch_complete(batches + i)) return fail(h, ALORE_NMPC_E_INVALID, "rti_many_prepare: batch has NULL members");
    if (known_independent(h, batches, count, B)) return ALORE_NMPC_OK;
    if (!batches_independent(h, batches, count, B))
        return fail(h, ALORE_NMPC_E_INVALID, "rti_many_prepare: the batches overlap (alore_nmpc_rti_many would run them in order)");
    remember_independent(h, batches, count, B);
    return ALORE_NMPC_OK;
}

int alore_nmpc_set_problem_mask(alore_nmpc_handle h, const unsigned char* mask)
{
    if (!h) return ALORE_NMPC_E_INVALID;
    h->mask = mask;
    return ALORE_NMPC_OK;
}

int alore_nmpc_set_many_mode(alore_nmpc_handle h, int mode)
{
    if (!h || mode < 0 || mode > 1) return fail(h, ALORE_NMPC_E_INVALID, "set_many_mode: 0 (groups) or 1 (streams)");
    h->many_mode = mode;
    return ALORE_NMPC_OK;
}

int alore_nmpc_set_two_phase(alore_nmpc_handle h, int mode)
{
    if (!h || mode < -1 || mode > 1) return fail(h, ALORE_NMPC_E_INVALID, "set_two_phase: -1 (automatic), 0 (never) or 1 (wherever the build exists)");
    h->tp.mode = mode;
    return ALORE_NMPC_OK;
}

int alore_nmpc_get_two_phase_info(alore_nmpc_handle h, alore_nmpc_two_phase_info* out)
{
    if (!h || !out) return ALORE_NMPC_E_INVALID;
    out->last_grid_two_phase = h->tp.last;
    out->two_phase_batches = h->tp.info[0];
    out->tail_workgroups_per_batch = h->tp.info[1];
    out->lag_units = h->tp.info[2];
    out->tail_share = (float)h->tp.share;
    return ALORE_NMPC_OK;
}

int alore_nmpc_set_launch_overlap(alore_nmpc_handle h, int ways)
{
    if (!h || ways < 1 || ways > 32) return fail(h, ALORE_NMPC_E_INVALID, "set_launch_overlap: ways must be 1 .. 32");
    h->overlap = ways;
    return ALORE_NMPC_OK;
}

int alore_nmpc_linearize(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, const alore_nmpc_lin_out* out,
                         void* stream)
{
    if (!h || !dev || !out || B <= 0 || !dev->x || !dev->u || !dev->od)
        return fail(h, ALORE_NMPC_E_INVALID, "linearize: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, nmpc::launch_linearize(*dev, B, h->cfg.N, h->cfg.dt, *out, (hipStream_t)stream));
    return ALORE_NMPC_OK;
}

int alore_nmpc_condense(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, const alore_nmpc_dense_qp_data* out, void* stream)
{
    if (!h || !dev || !out || B <= 0 || !out->H || !out->g || !out->lb || !out->ub || !dev->x || !dev->u || !dev->od || !dev->y || !dev->yN ||
        !dev->W || !dev->WN || !dev->x0 || !dev->lbValues || !dev->ubValues)
        return fail(h, ALORE_NMPC_E_INVALID, "condense: bad argument");
    if (h->cfg.N > 64 || (long)nmpc::condense_lds_bytes(h->cfg.N) > (long)h->lds_limit)
        return fail(h, ALORE_NMPC_E_UNSUPPORTED, "condense: horizons up to 64 (the E blocks of a problem live in LDS) and within this device's LDS per workgroup");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, nmpc::launch_condense(*dev, h->lin_x, h->lin_u, B, h->cfg.N, h->cfg.dt, h->shared, out->H, out->g, out->lb, out->ub, (hipStream_t)stream));
    return ALORE_NMPC_OK;
}

int alore_nmpc_dense_qp(alore_nmpc_handle h, int B, int n, const alore_nmpc_dense_qp_data* qp, float* x, float* y, int* status, int* n_iter,
                        void* stream)
{
    if (!h || !qp || B <= 0 || n < 1 || n > 128 || !qp->H || !qp->g || !qp->lb || !qp->ub || !x || !y || !status || !n_iter)
        return fail(h, ALORE_NMPC_E_INVALID, "dense_qp: bad argument (n <= 128)");
    if ((long)nmpc::dense_qp_lds_bytes(n) > (long)h->lds_limit)
        return fail(h, ALORE_NMPC_E_UNSUPPORTED, "dense_qp: the factor of an n x n Hessian does not fit this device's LDS per workgroup (n = 128 needs 68 KB)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, nmpc::launch_dense_qp(B, n, qp->H, qp->g, qp->lb, qp->ub, x, y, status, n_iter, h->cfg.max_as_iter, (hipStream_t)stream));
    return ALORE_NMPC_OK;
}

int alore_nmpc_forward_simulate(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, void* stream)
{
    if (!h || !dev || B <= 0 || !dev->x || !dev->u || !dev->od)
        return fail(h, ALORE_NMPC_E_INVALID, "forward_simulate: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, nmpc::launch_forward_simulate(*dev, B, h->cfg.N, h->cfg.dt, (hipStream_t)stream));
    return ALORE_NMPC_OK;
}

int alore_nmpc_shift(alore_nmpc_handle h, const alore_nmpc_batch* dev, int B, int strategy, const float* xEnd,
                     const float* uEnd, void* stream)
{
    if (!h || !dev || B <= 0 || !dev->x || !dev->u || !dev->od)
        return fail(h, ALORE_NMPC_E_INVALID, "shift: bad argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, nmpc::launch_shift(*dev, B, h->cfg.N, h->cfg.dt, strategy, xEnd, uEnd, (hipStream_t)stream));
    return ALORE_NMPC_OK;
}

int alore_nmpc_set_shared_members(alore_nmpc_handle h, unsigned mask)
{
    if (!h || (mask & ~(unsigned)(ALORE_NMPC_SHARED_W | ALORE_NMPC_SHARED_BOUNDS | ALORE_NMPC_SHARED_OD)))
        return fail(h, ALORE_NMPC_E_INVALID, "set_shared_members: unknown bit");
    h->shared = mask;
    return ALORE_NMPC_OK;
}

int alore_nmpc_set_linearization_point(alore_nmpc_handle h, const float* x_lin, const float* u_lin)
{
    if (!h || ((x_lin == nullptr) != (u_lin == nullptr))) return fail(h, ALORE_NMPC_E_INVALID, "linearization point: bad argument");
    h->lin_x = x_lin;
    h->lin_u = u_lin;
    return ALORE_NMPC_OK;
}

int alore_nmpc_set_timing(alore_nmpc_handle h, int enable)
{
    if (!h) return ALORE_NMPC_E_INVALID;
    h->timing.on = enable != 0;
    h->timing.pending = false;
    h->timing.last_ms = -1.0f;
    return ALORE_NMPC_OK;
}

int alore_nmpc_get_launch_info(alore_nmpc_handle h, alore_nmpc_launch_info* out)
{
    if (!h || !out) return ALORE_NMPC_E_INVALID;
    if (!h->have_geom) return fail(h, ALORE_NMPC_E_INVALID, "launch_info: no launch yet");
    if (h->timing.on && h->timing.pending) {
        HIP_TRY(h, hipEventSynchronize(h->timing.ev1));
        HIP_TRY(h, hipEventElapsedTime(&h->timing.last_ms, h->timing.ev0, h->timing.ev1));
        h->timing.pending = false;
    }
    out->lanes_per_problem = h->last_geom.L | (h->last_geom.block ? 0x100 : 0);
    out->problems_per_block = h->last_geom.G * h->last_geom.wpb;
    out->threads_per_block = h->last_geom.threads;
    out->grid = h->last_geom.grid;
    out->lds_bytes_per_block = (int)h->last_geom.lds_bytes;
    out->last_kernel_ms = h->timing.on ? h->timing.last_ms : -1.0f;
    return ALORE_NMPC_OK;
}

} // extern "C"
