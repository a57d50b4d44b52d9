// nmpc_group_ops.h -- moves, scans and reductions over the L lanes that share a problem in nmpc::rti_block_kernel (gfx950).
//
// A group is L = 4, 8, 16 or 32 consecutive lanes, aligned, lane j of the group at wavefront lane base + j.  The generic forms
// are DPP row shifts with a select for the lanes whose source would lie outside the group.  A group of 4 is exactly a DPP quad:
// the L = 4 forms further down permute inside the quad (quad_perm never reads another problem's lane), need no select and no
// zeroed `old` register, and carry the permutation as the DPP operand of the instruction that consumes it.  The compiler does not
// fold a DPP move into its consumer and pays v_mov + s_nop + v_mov_b32_dpp + v_cndmask per level of a scan; for the lone wavefront
// of a SIMD each of those is a full issue slot.  The L = 4 forms compute the bits of the generic ones (same sums in the same
// association, the same + 0.0f where the generic form adds its zero); tests/harness/group_ops_check.hip compares them.
//
// Every L = 4 form (quad_*) is one asm block, called with whole quads active (all call sites are stage-parallel code, outside the
// masked sweeps).  gfx9 hazard: a VALU write of a register followed by a DPP read of it needs two wait states.  The compiler does
// not look into an asm block, so each block opens with s_nop 1 (its inputs may have been written by the instruction in front of it)
// and keeps two issue slots between a write and the DPP read of it inside: the instructions of the other value(s) of a fused form
// (quad_prefix2, quad_prefix3, quad_total2, quad_above2), else an s_nop.  For the same reason a RESULT of a block must not be the
// source of a DPP move in the two instructions behind it (the compiler does not know that a vector instruction wrote it): every call
// site feeds the results to ordinary arithmetic.
// The kernel body calls gprefix1 / gprefix2 / gprefix3 / gtotal1 / gtotal2 / gabove / gabove2 / gmax1 <L, QUAD>: the quad form where
// QUAD, else the generic calls one after the other.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

namespace nmpc {
namespace {

// DPP move inside a row of 16 lanes; lanes without a source keep `old`
template <int CTRL>
__device__ __forceinline__ float dppk(float old, float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(x), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ int dppk_i(int old, int x)
{
    return __builtin_amdgcn_update_dpp(old, x, CTRL, 0xF, 0xF, false);
}
// DPP move with a row mask: rows outside the mask keep `old`
template <int CTRL, int ROWS>
__device__ __forceinline__ float dppr(float old, float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(x), CTRL, ROWS, 0xF, false));
}
template <int CTRL, int ROWS>
__device__ __forceinline__ int dppr_i(int old, int x)
{
    return __builtin_amdgcn_update_dpp(old, x, CTRL, ROWS, 0xF, false);
}
// lane i <- lane i + 1 / lane i - 1.  Groups of up to 16 lanes sit inside a DPP row (row_shl / row_shr: the lane at the
// end of a row keeps its value); a group of 32 spans two rows and uses the wavefront shifts of gfx9 (the lane at the end
// of a group then sees its neighbour group's value: every caller treats the edge lanes separately).
template <int L>
__device__ __forceinline__ float lane_next(float x)
{
    if constexpr (L == 32) return dppk<0x130>(x, x); // wave_shl:1
    else return dppk<0x101>(x, x);                    // row_shl:1
}
template <int L>
__device__ __forceinline__ float lane_prev(float x)
{
    if constexpr (L == 32) return dppk<0x138>(x, x); // wave_shr:1
    else return dppk<0x111>(x, x);                    // row_shr:1
}

// value of the first / last lane of the group of L lanes (L = 4: quad_perm; 8, 16: row_newbcast, gfx90a+; 32: the two
// group ends through scalar registers)
template <int L>
__device__ __forceinline__ float gfirst(float x, int lane)
{
    if constexpr (L == 4) return dppk<0x00>(x, x);
    else if constexpr (L == 16) return dppk<0x150>(x, x);
    else if constexpr (L == 32) {
        const int lo = __builtin_amdgcn_readlane(__float_as_int(x), 0), hi = __builtin_amdgcn_readlane(__float_as_int(x), 32);
        return __int_as_float((lane & 32) ? hi : lo);
    } else { const float lo = dppk<0x150>(x, x), hi = dppk<0x158>(x, x); return (lane & 8) ? hi : lo; }
}
template <int L>
__device__ __forceinline__ float glast(float x, int lane)
{
    if constexpr (L == 4) return dppk<0xFF>(x, x);
    else if constexpr (L == 16) return dppk<0x15F>(x, x);
    else if constexpr (L == 32) {
        const int lo = __builtin_amdgcn_readlane(__float_as_int(x), 31), hi = __builtin_amdgcn_readlane(__float_as_int(x), 63);
        return __int_as_float((lane & 32) ? hi : lo);
    } else { const float lo = dppk<0x157>(x, x), hi = dppk<0x15F>(x, x); return (lane & 8) ? hi : lo; }
}
// inclusive prefix sum over the lanes of a group (row_shr:1, 2, 4, 8; groups are aligned inside DPP rows; a group of 32
// adds the total of its first row to its second: row_bcast:15 into rows 1 and 3)
template <int L>
__device__ __forceinline__ float gprefix(float x, int j)
{
    float v;
    v = dppk<0x111>(0.0f, x); if (L < 16) v = (j >= 1) ? v : 0.0f; x += v;
    v = dppk<0x112>(0.0f, x); if (L < 16) v = (j >= 2) ? v : 0.0f; x += v;
    if constexpr (L >= 8) { v = dppk<0x114>(0.0f, x); if (L < 16) v = (j >= 4) ? v : 0.0f; x += v; }
    if constexpr (L >= 16) { v = dppk<0x118>(0.0f, x); x += v; }
    if constexpr (L >= 32) { v = dppr<0x142, 0xA>(0.0f, x); x += v; }
    return x;
}
template <int L>
__device__ __forceinline__ int gprefix_max(int x, int j)
{
    constexpr int NEG = -2147483647 - 1;
    int v;
    v = dppk_i<0x111>(NEG, x); if (L < 16) v = (j >= 1) ? v : NEG; x = max(x, v);
    v = dppk_i<0x112>(NEG, x); if (L < 16) v = (j >= 2) ? v : NEG; x = max(x, v);
    if constexpr (L >= 8) { v = dppk_i<0x114>(NEG, x); if (L < 16) v = (j >= 4) ? v : NEG; x = max(x, v); }
    if constexpr (L >= 16) { v = dppk_i<0x118>(NEG, x); x = max(x, v); }
    if constexpr (L >= 32) { v = dppr_i<0x142, 0xA>(NEG, x); x = max(x, v); }
    return x;
}
template <int L>
__device__ __forceinline__ float gtotal(float x, int j, int lane) { return glast<L>(gprefix<L>(x, j), lane); }
template <int L>
__device__ __forceinline__ int gmax(int x, int j, int lane)
{
    return __float_as_int(glast<L>(__int_as_float(gprefix_max<L>(x, j)), lane));
}
// lexicographic minimum of (v, key) over the lanes of a group, in every lane
template <int L>
__device__ __forceinline__ void gmin_pair(float& v, int& key, int j, int lane)
{
    auto step = [&](auto tag, auto rows, int dist) {
        constexpr int CTRL = decltype(tag)::value;
        constexpr int ROWS = decltype(rows)::value;
        const float pv = dppr<CTRL, ROWS>(v, v);
        const int pk = dppr_i<CTRL, ROWS>(key, key);
        const bool has = (L >= 16) || (j >= dist);
        const bool take = has && ((pv < v) || (pv == v && pk < key));
        v = take ? pv : v;
        key = take ? pk : key;
    };
    using all = std::integral_constant<int, 0xF>;
    step(std::integral_constant<int, 0x111>{}, all{}, 1);
    step(std::integral_constant<int, 0x112>{}, all{}, 2);
    if constexpr (L >= 8) step(std::integral_constant<int, 0x114>{}, all{}, 4);
    if constexpr (L >= 16) step(std::integral_constant<int, 0x118>{}, all{}, 8);
    if constexpr (L >= 32) step(std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xA>{}, 16);
    v = glast<L>(v, lane);
    key = __float_as_int(glast<L>(__int_as_float(key), lane));
}
template <int L>
__device__ __forceinline__ bool gany(bool pred, int base)
{
    const unsigned long long m = __ballot(pred);
    constexpr unsigned long long MASK = (L >= 64) ? ~0ull : ((1ull << (L & 63)) - 1ull);
    return ((m >> base) & MASK) != 0ull;
}

// ---- L = 4: inside the quad -----------------------------------------------------------------------------------------------
// Scan, level 1: lane j takes lane j - 1 (quad_perm:[0,0,1,2]), level 2: lane j - 2 (quad_perm:[0,1,0,1]); lanes 0 / 0, 1 have no
// such lane, read one of their own quad and AND it away with a lane constant (all ones for j >= 1 / j >= 2, else zero): the
// addend is the neighbour's bits or + 0.0f, which is what the generic select gives, non-finite values and the + 0.0f that turns a
// - 0 partial sum into + 0 included.  bound_ctrl: a source lane that is switched off reads as zero, like the generic `old`.
#define ALORE_Q_SHR1 "quad_perm:[0,0,1,2] row_mask:0xf bank_mask:0xf bound_ctrl:1"
#define ALORE_Q_SHR2 "quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1"
// Reductions wanted in every lane, butterfly: lane j takes lane j ^ 1, then lane j ^ 2.  Lane 3 of the generic scan computes
// (x3 + x2) + (x1 + x0) and never adds a zero; the butterfly computes that sum, or the one with the operands of an addition swapped,
// in all four lanes.
#define ALORE_Q_XOR1 "quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
#define ALORE_Q_XOR2 "quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf"
#define ALORE_Q_LAST "quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf"

__device__ __forceinline__ int quad_mask1(int j) { return (j >= 1) ? -1 : 0; }
__device__ __forceinline__ int quad_mask2(int j) { return (j >= 2) ? -1 : 0; }

// The results go to registers of their own: an input that is still wanted afterwards costs no copy.
// inclusive prefix sums of one, two, three independent values: gprefix<4>
__device__ __forceinline__ float quad_prefix(float x, int j)
{
    float r, t;
    asm("s_nop 1\n\t"
        "v_and_b32_dpp %1, %2, %3 " ALORE_Q_SHR1 "\n\t"
        "v_add_f32_e32 %0, %2, %1\n\t"
        "s_nop 1\n\t"
        "v_and_b32_dpp %1, %0, %4 " ALORE_Q_SHR2 "\n\t"
        "v_add_f32_e32 %0, %0, %1"
        : "=&v"(r), "=&v"(t) : "v"(x), "v"(quad_mask1(j)), "v"(quad_mask2(j)));
    return r;
}
__device__ __forceinline__ void quad_prefix2(float& a, float& b, int j)
{
    float ra, rb, s, t;
    asm("s_nop 1\n\t"
        "v_and_b32_dpp %2, %4, %6 " ALORE_Q_SHR1 "\n\t"
        "v_and_b32_dpp %3, %5, %6 " ALORE_Q_SHR1 "\n\t"
        "v_add_f32_e32 %0, %4, %2\n\t"
        "v_add_f32_e32 %1, %5, %3\n\t"
        "s_nop 0\n\t"
        "v_and_b32_dpp %2, %0, %7 " ALORE_Q_SHR2 "\n\t"
        "v_and_b32_dpp %3, %1, %7 " ALORE_Q_SHR2 "\n\t"
        "v_add_f32_e32 %0, %0, %2\n\t"
        "v_add_f32_e32 %1, %1, %3"
        : "=&v"(ra), "=&v"(rb), "=&v"(s), "=&v"(t) : "v"(a), "v"(b), "v"(quad_mask1(j)), "v"(quad_mask2(j)));
    a = ra; b = rb;
}
__device__ __forceinline__ void quad_prefix3(float& a, float& b, float& c, int j)
{
    float ra, rb, rc, s, t, u;
    asm("s_nop 1\n\t"
        "v_and_b32_dpp %3, %6, %9 " ALORE_Q_SHR1 "\n\t"
        "v_and_b32_dpp %4, %7, %9 " ALORE_Q_SHR1 "\n\t"
        "v_and_b32_dpp %5, %8, %9 " ALORE_Q_SHR1 "\n\t"
        "v_add_f32_e32 %0, %6, %3\n\t"
        "v_add_f32_e32 %1, %7, %4\n\t"
        "v_add_f32_e32 %2, %8, %5\n\t"
        "v_and_b32_dpp %3, %0, %10 " ALORE_Q_SHR2 "\n\t"
        "v_and_b32_dpp %4, %1, %10 " ALORE_Q_SHR2 "\n\t"
        "v_and_b32_dpp %5, %2, %10 " ALORE_Q_SHR2 "\n\t"
        "v_add_f32_e32 %0, %0, %3\n\t"
        "v_add_f32_e32 %1, %1, %4\n\t"
        "v_add_f32_e32 %2, %2, %5"
        : "=&v"(ra), "=&v"(rb), "=&v"(rc), "=&v"(s), "=&v"(t), "=&v"(u)
        : "v"(a), "v"(b), "v"(c), "v"(quad_mask1(j)), "v"(quad_mask2(j)));
    a = ra; b = rb; c = rc;
}
// totals in every lane: gtotal<4>
__device__ __forceinline__ float quad_total(float x)
{
    float r;
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %0, %1, %1 " ALORE_Q_XOR1 "\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 " ALORE_Q_XOR2
        : "=&v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ void quad_total2(float& a, float& b)
{
    float ra, rb;
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %0, %2, %2 " ALORE_Q_XOR1 "\n\t"
        "v_add_f32_dpp %1, %3, %3 " ALORE_Q_XOR1 "\n\t"
        "s_nop 0\n\t"
        "v_add_f32_dpp %0, %0, %0 " ALORE_Q_XOR2 "\n\t"
        "v_add_f32_dpp %1, %1, %1 " ALORE_Q_XOR2
        : "=&v"(ra), "=&v"(rb) : "v"(a), "v"(b));
    a = ra; b = rb;
}
// total - prefix: the total is lane 3's prefix, v_sub_f32_dpp takes it as its first operand
__device__ __forceinline__ float quad_above(float x, int j)
{
    float r, t;
    asm("s_nop 1\n\t"
        "v_and_b32_dpp %1, %2, %3 " ALORE_Q_SHR1 "\n\t"
        "v_add_f32_e32 %0, %2, %1\n\t"
        "s_nop 1\n\t"
        "v_and_b32_dpp %1, %0, %4 " ALORE_Q_SHR2 "\n\t"
        "v_add_f32_e32 %0, %0, %1\n\t"
        "s_nop 1\n\t"
        "v_sub_f32_dpp %0, %0, %0 " ALORE_Q_LAST
        : "=&v"(r), "=&v"(t) : "v"(x), "v"(quad_mask1(j)), "v"(quad_mask2(j)));
    return r;
}
__device__ __forceinline__ void quad_above2(float& a, float& b, int j)
{
    float ra, rb, s, t;
    asm("s_nop 1\n\t"
        "v_and_b32_dpp %2, %4, %6 " ALORE_Q_SHR1 "\n\t"
        "v_and_b32_dpp %3, %5, %6 " ALORE_Q_SHR1 "\n\t"
        "v_add_f32_e32 %0, %4, %2\n\t"
        "v_add_f32_e32 %1, %5, %3\n\t"
        "s_nop 0\n\t"
        "v_and_b32_dpp %2, %0, %7 " ALORE_Q_SHR2 "\n\t"
        "v_and_b32_dpp %3, %1, %7 " ALORE_Q_SHR2 "\n\t"
        "v_add_f32_e32 %0, %0, %2\n\t"
        "v_add_f32_e32 %1, %1, %3\n\t"
        "s_nop 0\n\t"
        "v_sub_f32_dpp %0, %0, %0 " ALORE_Q_LAST "\n\t"
        "v_sub_f32_dpp %1, %1, %1 " ALORE_Q_LAST
        : "=&v"(ra), "=&v"(rb), "=&v"(s), "=&v"(t) : "v"(a), "v"(b), "v"(quad_mask1(j)), "v"(quad_mask2(j)));
    a = ra; b = rb;
}
// One level of the forward sweep's scan of affine maps (a 3 x 3 matrix, row-major, and a vector): every lane takes the twelve values
// of lane j - DIST of its quad, DIST = 1 or 2; a lane that has no such lane takes the identity map (1.0f on the diagonal, + 0.0f
// elsewhere).  `mask` is quad_mask1 / quad_mask2.  Off the diagonal the AND gives the neighbour's bits or + 0.0f; on it v_bfi_b32
// picks the neighbour's bits or 1.0f.  Twelve independent values: no wait states inside.
#define ALORE_QUAD_FETCH_MAP(PERM)                                                                                                  \
    asm("s_nop 1\n\t"                                                                                                               \
        "v_mov_b32_dpp %0, %12 " PERM "\n\t"                                                                                        \
        "v_mov_b32_dpp %4, %16 " PERM "\n\t"                                                                                        \
        "v_mov_b32_dpp %8, %20 " PERM "\n\t"                                                                                        \
        "v_and_b32_dpp %1, %13, %24 " PERM "\n\t"                                                                                   \
        "v_and_b32_dpp %2, %14, %24 " PERM "\n\t"                                                                                   \
        "v_and_b32_dpp %3, %15, %24 " PERM "\n\t"                                                                                   \
        "v_and_b32_dpp %5, %17, %24 " PERM "\n\t"                                                                                   \
        "v_and_b32_dpp %6, %18, %24 " PERM "\n\t"                                                                                   \
        "v_and_b32_dpp %7, %19, %24 " PERM "\n\t"                                                                                   \
        "v_and_b32_dpp %9, %21, %24 " PERM "\n\t"                                                                                   \
        "v_and_b32_dpp %10, %22, %24 " PERM "\n\t"                                                                                  \
        "v_and_b32_dpp %11, %23, %24 " PERM "\n\t"                                                                                  \
        "v_bfi_b32 %0, %24, %0, 1.0\n\t"                                                                                            \
        "v_bfi_b32 %4, %24, %4, 1.0\n\t"                                                                                            \
        "v_bfi_b32 %8, %24, %8, 1.0"                                                                                                \
        : "=&v"(g[0]), "=&v"(g[1]), "=&v"(g[2]), "=&v"(g[3]), "=&v"(g[4]), "=&v"(g[5]), "=&v"(g[6]), "=&v"(g[7]), "=&v"(g[8]),      \
          "=&v"(g[9]), "=&v"(g[10]), "=&v"(g[11])                                                                                   \
        : "v"(m[0]), "v"(m[1]), "v"(m[2]), "v"(m[3]), "v"(m[4]), "v"(m[5]), "v"(m[6]), "v"(m[7]), "v"(m[8]), "v"(m[9]), "v"(m[10]), \
          "v"(m[11]), "v"(mask))
template <int DIST>
__device__ __forceinline__ void quad_fetch_map(const float (&m)[12], float (&g)[12], int j)
{
    static_assert(DIST == 1 || DIST == 2, "inside a quad");
    if constexpr (DIST == 1) { const int mask = quad_mask1(j); ALORE_QUAD_FETCH_MAP(ALORE_Q_SHR1); }
    else { const int mask = quad_mask2(j); ALORE_QUAD_FETCH_MAP(ALORE_Q_SHR2); }
}
// maxima of integers are exact in any order: the butterfly leaves the group's maximum in every lane (gmax<4>).  The scan
// (gprefix_max<4>) needs no mask when the lanes without a predecessor read themselves.
__device__ __forceinline__ int quad_prefix_max(int x)
{
    int r;
    asm("s_nop 1\n\t"
        "v_max_i32_dpp %0, %1, %1 quad_perm:[0,0,1,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_i32_dpp %0, %0, %0 quad_perm:[0,1,0,1] row_mask:0xf bank_mask:0xf"
        : "=&v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ int quad_max(int x)
{
    int r;
    asm("s_nop 1\n\t"
        "v_max_i32_dpp %0, %1, %1 " ALORE_Q_XOR1 "\n\t"
        "s_nop 1\n\t"
        "v_max_i32_dpp %0, %0, %0 " ALORE_Q_XOR2
        : "=&v"(r) : "v"(x));
    return r;
}

// ---- what the kernel body calls: the quad form where QUAD (L = 4 and the body has the registers for it), else the generic
// calls they replace, one after the other ------------------------------------------------------------------------------------
template <int L, bool QUAD>
__device__ __forceinline__ float gprefix1(float x, int j)
{
    static_assert(!QUAD || L == 4, "a quad is a group of 4");
    if constexpr (QUAD) return quad_prefix(x, j);
    else return gprefix<L>(x, j);
}
template <int L, bool QUAD>
__device__ __forceinline__ void gprefix2(float& a, float& b, int j)
{
    static_assert(!QUAD || L == 4, "a quad is a group of 4");
    if constexpr (QUAD) quad_prefix2(a, b, j);
    else { a = gprefix<L>(a, j); b = gprefix<L>(b, j); }
}
template <int L, bool QUAD>
__device__ __forceinline__ void gprefix3(float& a, float& b, float& c, int j)
{
    static_assert(!QUAD || L == 4, "a quad is a group of 4");
    if constexpr (QUAD) quad_prefix3(a, b, c, j);
    else { a = gprefix<L>(a, j); b = gprefix<L>(b, j); c = gprefix<L>(c, j); }
}
template <int L, bool QUAD>
__device__ __forceinline__ float gtotal1(float x, int j, int lane)
{
    static_assert(!QUAD || L == 4, "a quad is a group of 4");
    if constexpr (QUAD) return quad_total(x);
    else return gtotal<L>(x, j, lane);
}
template <int L, bool QUAD>
__device__ __forceinline__ void gtotal2(float& a, float& b, int j, int lane)
{
    static_assert(!QUAD || L == 4, "a quad is a group of 4");
    if constexpr (QUAD) quad_total2(a, b);
    else { a = gtotal<L>(a, j, lane); b = gtotal<L>(b, j, lane); }
}
// sum over the lanes ABOVE the lane, as total - inclusive prefix (the suffix sums of the prediction's adjoint)
template <int L, bool QUAD>
__device__ __forceinline__ float gabove(float x, int j, int lane)
{
    static_assert(!QUAD || L == 4, "a quad is a group of 4");
    if constexpr (QUAD) return quad_above(x, j);
    else { const float pr = gprefix<L>(x, j); return glast<L>(pr, lane) - pr; }
}
template <int L, bool QUAD>
__device__ __forceinline__ void gabove2(float& a, float& b, int j, int lane)
{
    static_assert(!QUAD || L == 4, "a quad is a group of 4");
    if constexpr (QUAD) quad_above2(a, b, j);
    else {
        const float pa = gprefix<L>(a, j), pb = gprefix<L>(b, j);
        a = glast<L>(pa, lane) - pa; b = glast<L>(pb, lane) - pb;
    }
}
template <int L, bool QUAD>
__device__ __forceinline__ int gmax1(int x, int j, int lane)
{
    static_assert(!QUAD || L == 4, "a quad is a group of 4");
    if constexpr (QUAD) return quad_max(x);
    else return gmax<L>(x, j, lane);
}

} // namespace
} // namespace nmpc
