// group_ops_check.hip -- csrc/nmpc_group_ops.h on the device, one wavefront (tests/test_group_ops.py builds and runs it).
//
//   L = 4   every quad-native form (quad_prefix, _prefix2, _prefix3, quad_total, _total2, quad_above, _above2, quad_prefix_max, quad_max,
//           quad_fetch_map<1>, <2>) against the generic text, kept here as ref_*: bit for bit, over NV vectors of 64 lanes that hold
//           +-0, denormals, values of mixed magnitude, and Inf / NaN in whole quads only.  The same vectors with the non-finite
//           quads replaced by 1.0f must give the same bits in every other quad: a quad never sees its neighbour.
//   L = 8, 16  gprefix, gtotal against serial sums in double within (L - 1) * 2^-24 * sum |x_i| (any order of a float32 sum of L
//           terms is that close to the exact one, to first order; 2 % on top for the second), gprefix_max and gmax exactly: the
//           move into the header did not change them.
// Exit status 0: all equal.  1: a mismatch (the first few are printed).  2: a HIP error.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nmpc_group_ops.h"

namespace {

using namespace nmpc;

// ---- the generic forms under another name (the text of gprefix<L>, gprefix_max<L>, gtotal<L>, gmax<L> and of the forward scan's
// fetch, which L = 4 took before it had forms of its own)
template <int L>
__device__ __forceinline__ float ref_gprefix(float x, int j)
{
    float v;
    v = dppk<0x111>(0.0f, x); if (L < 16) v = (j >= 1) ? v : 0.0f; x += v;
    v = dppk<0x112>(0.0f, x); if (L < 16) v = (j >= 2) ? v : 0.0f; x += v;
    if constexpr (L >= 8) { v = dppk<0x114>(0.0f, x); if (L < 16) v = (j >= 4) ? v : 0.0f; x += v; }
    if constexpr (L >= 16) { v = dppk<0x118>(0.0f, x); x += v; }
    return x;
}
template <int L>
__device__ __forceinline__ int ref_gprefix_max(int x, int j)
{
    constexpr int NEG = -2147483647 - 1;
    int v;
    v = dppk_i<0x111>(NEG, x); if (L < 16) v = (j >= 1) ? v : NEG; x = max(x, v);
    v = dppk_i<0x112>(NEG, x); if (L < 16) v = (j >= 2) ? v : NEG; x = max(x, v);
    if constexpr (L >= 8) { v = dppk_i<0x114>(NEG, x); if (L < 16) v = (j >= 4) ? v : NEG; x = max(x, v); }
    if constexpr (L >= 16) { v = dppk_i<0x118>(NEG, x); x = max(x, v); }
    return x;
}
__device__ __forceinline__ float ref_glast4(float x) { return dppk<0xFF>(x, x); }
__device__ __forceinline__ float ref_gtotal4(float x, int j) { return ref_glast4(ref_gprefix<4>(x, j)); }
__device__ __forceinline__ int ref_gmax4(int x, int j) { return __float_as_int(ref_glast4(__int_as_float(ref_gprefix_max<4>(x, j)))); }
__device__ __forceinline__ float ref_gabove4(float x, int j) { const float pr = ref_gprefix<4>(x, j); return ref_glast4(pr) - pr; }
template <int CTRL>
__device__ __forceinline__ float ref_fetch(float v, float ident, bool has) { const float r = dppr<CTRL, 0xF>(ident, v); return has ? r : ident; }

constexpr int NV = 320;    // vectors of 64 lanes
constexpr int COLS4 = 38;  // outputs per lane and vector of the L = 4 part
constexpr int COLS8 = 8;   // of the L = 8 / 16 part

__device__ __forceinline__ unsigned bits(float x) { return (unsigned)__float_as_int(x); }

// in: 3 * NV * 64 floats (a, b, c).  got / want: COLS4 * NV * 64 words each.
__global__ void __launch_bounds__(64) quad_kernel(const float* in, unsigned* got, unsigned* want)
{
    const int lane = threadIdx.x, j = lane & 3;
    for (int v = 0; v < NV; ++v) {
        const float a = in[(0 * NV + v) * 64 + lane], b = in[(1 * NV + v) * 64 + lane], c = in[(2 * NV + v) * 64 + lane];
        int col = 0;
        auto put = [&](unsigned g, unsigned w) {
            got[(col * NV + v) * 64 + lane] = g;
            want[(col * NV + v) * 64 + lane] = w;
            ++col;
        };
        put(bits(quad_prefix(a, j)), bits(ref_gprefix<4>(a, j)));
        { float p = a, q = b; quad_prefix2(p, q, j); put(bits(p), bits(ref_gprefix<4>(a, j))); put(bits(q), bits(ref_gprefix<4>(b, j))); }
        {
            float p = a, q = b, r = c;
            quad_prefix3(p, q, r, j);
            put(bits(p), bits(ref_gprefix<4>(a, j))); put(bits(q), bits(ref_gprefix<4>(b, j))); put(bits(r), bits(ref_gprefix<4>(c, j)));
        }
        put(bits(quad_total(c)), bits(ref_gtotal4(c, j)));
        { float p = a, q = b; quad_total2(p, q); put(bits(p), bits(ref_gtotal4(a, j))); put(bits(q), bits(ref_gtotal4(b, j))); }
        put(bits(quad_above(b, j)), bits(ref_gabove4(b, j)));
        { float p = c, q = a; quad_above2(p, q, j); put(bits(p), bits(ref_gabove4(c, j))); put(bits(q), bits(ref_gabove4(a, j))); }
        const int ia = __float_as_int(a), ib = __float_as_int(b);
        put((unsigned)quad_prefix_max(ia), (unsigned)ref_gprefix_max<4>(ia, j));
        put((unsigned)quad_max(ib), (unsigned)ref_gmax4(ib, j));
        // the forward scan's fetch: twelve values, the next vectors' among them
        float m[12], g1[12], g2[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) m[i] = in[((i % 3) * NV + (v + i / 3) % NV) * 64 + lane];
        quad_fetch_map<1>(m, g1, j);
        quad_fetch_map<2>(m, g2, j);
        for (int i = 0; i < 12; ++i) put(bits(g1[i]), bits(ref_fetch<0x111>(m[i], (i == 0 || i == 4 || i == 8) ? 1.f : 0.f, j >= 1)));
        for (int i = 0; i < 12; ++i) put(bits(g2[i]), bits(ref_fetch<0x112>(m[i], (i == 0 || i == 4 || i == 8) ? 1.f : 0.f, j >= 2)));
    }
}

// in: NV * 64 finite floats.  out: COLS8 * NV * 64 words: prefix8, total8, pmax8, max8, prefix16, total16, pmax16, max16
__global__ void __launch_bounds__(64) wide_kernel(const float* in, unsigned* out)
{
    const int lane = threadIdx.x;
    for (int v = 0; v < NV; ++v) {
        const float a = in[v * 64 + lane];
        const int ia = __float_as_int(a);
        int col = 0;
        auto put = [&](unsigned g) { out[(col * NV + v) * 64 + lane] = g; ++col; };
        put(bits(gprefix<8>(a, lane & 7))); put(bits(gtotal<8>(a, lane & 7, lane)));
        put((unsigned)gprefix_max<8>(ia, lane & 7)); put((unsigned)gmax<8>(ia, lane & 7, lane));
        put(bits(gprefix<16>(a, lane & 15))); put(bits(gtotal<16>(a, lane & 15, lane)));
        put((unsigned)gprefix_max<16>(ia, lane & 15)); put((unsigned)gmax<16>(ia, lane & 15, lane));
    }
}

#define HIP_OK(e)                                                                                  \
    do {                                                                                           \
        const hipError_t err_ = (e);                                                               \
        if (err_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(err_), __LINE__); return 2; } \
    } while (0)

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 32); }
    float unit() { return (float)(next() & 0xFFFFFF) / 16777216.0f; } // [0, 1)
};
float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

// a finite value of mixed magnitude and sign
float mixed(Rng& r)
{
    const float m = 1.0f + r.unit();
    const int e = (int)(r.next() % 41) - 20;
    return ((r.next() & 1) ? -m : m) * std::ldexp(1.0f, e);
}
// the value of lane `lane` of vector `v` of member `k`: the kind of vector goes by v % 8
float special(Rng& r, int v, int lane)
{
    switch (v % 8) {
    case 0: return mixed(r);
    case 1: return (r.next() & 1) ? -0.0f : 0.0f;                                   // +-0 only
    case 2: return -0.0f;                                                           // a quad of -0: the scan's + 0.0f makes + 0 of lane 0
    case 3: return from_bits((r.next() & 0x807FFFFFu));                             // denormals (and +-0)
    case 4: return (r.next() % 3 == 0) ? ((r.next() & 1) ? -0.0f : 0.0f) : mixed(r); // zeros among values
    case 5: return (r.next() & 1) ? from_bits(r.next() & 0x807FFFFFu) : mixed(r) * 1e-30f; // denormals among tiny values
    case 6: { const float x = mixed(r); return (lane & 1) ? -x : x * (1.0f + 1e-6f); } // cancelling neighbours
    default: return mixed(r) * ((r.next() & 3) == 0 ? 1e20f : 1.0f);                // large among small (finite sums: < 2^90)
    }
}

} // namespace

int main()
{
    Rng rng{20261019ull};
    const size_t nin = (size_t)3 * NV * 64, nout = (size_t)COLS4 * NV * 64;
    std::vector<float> in(nin), clean(nin);
    std::vector<char> poisoned((size_t)NV * 16, 0); // per vector and quad
    for (int k = 0; k < 3; ++k)
        for (int v = 0; v < NV; ++v)
            for (int lane = 0; lane < 64; ++lane) in[((size_t)k * NV + v) * 64 + lane] = special(rng, v, lane);
    clean = in;
    // non-finite values in whole quads of every second vector: one or two quads, all three members, Inf / -Inf / NaN by lane
    for (int v = 1; v < NV; v += 2) {
        const int nq = 1 + (v / 2) % 2;
        for (int q = 0; q < nq; ++q) {
            const int quad = (v * 7 + q * 5) % 16;
            poisoned[(size_t)v * 16 + quad] = 1;
            for (int k = 0; k < 3; ++k)
                for (int l = 0; l < 4; ++l) {
                    const size_t i = ((size_t)k * NV + v) * 64 + quad * 4 + l;
                    const int kind = (v + k + l) % 4;
                    in[i] = kind == 0 ? INFINITY : kind == 1 ? -INFINITY : kind == 2 ? NAN : in[i];
                    clean[i] = 1.0f;
                }
        }
    }
    float *d_in = nullptr, *d_clean = nullptr, *d_fin = nullptr;
    unsigned *d_got = nullptr, *d_want = nullptr, *d_got2 = nullptr, *d_want2 = nullptr, *d_wide = nullptr;
    HIP_OK(hipMalloc(&d_in, nin * 4)); HIP_OK(hipMalloc(&d_clean, nin * 4));
    HIP_OK(hipMalloc(&d_got, nout * 4)); HIP_OK(hipMalloc(&d_want, nout * 4));
    HIP_OK(hipMalloc(&d_got2, nout * 4)); HIP_OK(hipMalloc(&d_want2, nout * 4));
    HIP_OK(hipMemcpy(d_in, in.data(), nin * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_clean, clean.data(), nin * 4, hipMemcpyHostToDevice));
    quad_kernel<<<1, 64>>>(d_in, d_got, d_want);
    HIP_OK(hipGetLastError());
    quad_kernel<<<1, 64>>>(d_clean, d_got2, d_want2);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<unsigned> got(nout), want(nout), got2(nout), want2(nout);
    HIP_OK(hipMemcpy(got.data(), d_got, nout * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(want.data(), d_want, nout * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(got2.data(), d_got2, nout * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(want2.data(), d_want2, nout * 4, hipMemcpyDeviceToHost));

    int bad = 0;
    auto is_nan = [](unsigned u) { return (u & 0x7F800000u) == 0x7F800000u && (u & 0x007FFFFFu) != 0; };
    long compared = 0;
    for (int col = 0; col < COLS4; ++col)
        for (int v = 0; v < NV; ++v)
            for (int lane = 0; lane < 64; ++lane) {
                const size_t i = ((size_t)col * NV + v) * 64 + lane;
                // the forward fetch reads the members of vectors v .. v + 3: a quad counts as poisoned if it is in any of them
                bool pq = false;
                for (int dv = 0; dv < 4; ++dv) pq = pq || poisoned[(size_t)((v + dv) % NV) * 16 + lane / 4];
                const bool float_col = !(col == 13 || col == 12); // gprefix_max, gmax: integers
                // inside a non-finite quad a sum may be the NaN of either operand: both NaN is agreement there
                const bool same = got[i] == want[i] || (pq && float_col && is_nan(got[i]) && is_nan(want[i]));
                ++compared;
                if (!same && bad++ < 10) std::printf("L=4 col %d vector %d lane %d: got %08x want %08x\n", col, v, lane, got[i], want[i]);
                if (got2[i] != want2[i] && bad++ < 10)
                    std::printf("L=4 (finite) col %d vector %d lane %d: got %08x want %08x\n", col, v, lane, got2[i], want2[i]);
                if (!pq && got[i] != got2[i] && bad++ < 10)
                    std::printf("L=4 col %d vector %d lane %d: %08x beside a non-finite quad, %08x beside 1.0f\n", col, v, lane, got[i], got2[i]);
            }

    // ---- L = 8, 16 against serial sums
    const size_t nf = (size_t)NV * 64, nw = (size_t)COLS8 * NV * 64;
    std::vector<float> fin(nf);
    for (int v = 0; v < NV; ++v)
        for (int lane = 0; lane < 64; ++lane) fin[(size_t)v * 64 + lane] = (v % 4 == 3) ? mixed(rng) * ((rng.next() & 3) == 0 ? 1e20f : 1.0f) : mixed(rng);
    HIP_OK(hipMalloc(&d_fin, nf * 4)); HIP_OK(hipMalloc(&d_wide, nw * 4));
    HIP_OK(hipMemcpy(d_fin, fin.data(), nf * 4, hipMemcpyHostToDevice));
    wide_kernel<<<1, 64>>>(d_fin, d_wide);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<unsigned> wide(nw);
    HIP_OK(hipMemcpy(wide.data(), d_wide, nw * 4, hipMemcpyDeviceToHost));
    double worst = 0.0;
    for (int li = 0; li < 2; ++li) {
        const int L = li == 0 ? 8 : 16;
        for (int v = 0; v < NV; ++v)
            for (int base = 0; base < 64; base += L) {
                double sum = 0.0, mag = 0.0;
                int mx = INT32_MIN;
                std::vector<double> pre(L), pmag(L);
                std::vector<int> pmx(L);
                for (int j = 0; j < L; ++j) {
                    const float x = fin[(size_t)v * 64 + base + j];
                    int ix; std::memcpy(&ix, &x, 4);
                    sum += x; mag += std::fabs((double)x); mx = ix > mx ? ix : mx;
                    pre[j] = sum; pmag[j] = mag; pmx[j] = mx;
                }
                for (int j = 0; j < L; ++j) {
                    auto at = [&](int col) { return wide[((size_t)(li * 4 + col) * NV + v) * 64 + base + j]; };
                    const double tol = (L - 1) * 1.02 * std::ldexp(1.0, -24);
                    const double ep = std::fabs((double)from_bits(at(0)) - pre[j]), et = std::fabs((double)from_bits(at(1)) - sum);
                    if (pmag[j] > 0) worst = std::fmax(worst, ep / (tol * pmag[j]));
                    if (mag > 0) worst = std::fmax(worst, et / (tol * mag));
                    if ((ep > tol * pmag[j] || et > tol * mag || (int)at(2) != pmx[j] || (int)at(3) != mx) && bad++ < 10)
                        std::printf("L=%d vector %d lane %d: prefix %g (%g) total %g (%g) pmax %d (%d) max %d (%d)\n", L, v, base + j,
                                    from_bits(at(0)), pre[j], from_bits(at(1)), sum, (int)at(2), pmx[j], (int)at(3), mx);
                    ++compared;
                }
            }
    }
    std::printf("group_ops_check: %ld comparisons, %d mismatches, L = 8 / 16 sums at %.3f of their bound\n", compared, bad, worst);
    (void)hipFree(d_in); (void)hipFree(d_clean); (void)hipFree(d_got); (void)hipFree(d_want); (void)hipFree(d_got2); (void)hipFree(d_want2);
    (void)hipFree(d_fin); (void)hipFree(d_wide);
    return bad ? 1 : 0;
}
