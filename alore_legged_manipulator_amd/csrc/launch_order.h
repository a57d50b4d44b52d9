// launch_order.h -- the arithmetic of launch_order_kernel (flat_traj_build.hip), host and device: the slots of a launch by piece
// count, most pieces first, stable in the slot index -- the order of the std::stable_sort in alore_backend_set_problems -- by a
// counting sort in one workgroup.  Every thread owns a contiguous run of slots and counts its pieces into its own row of a
// histogram [thread][bucket]; an exclusive prefix per bucket over the threads (slot order) and over the buckets (descending) gives
// every thread its first position per bucket.
//
// The histogram is static LDS, so the build's piece capacity decides the shape: 33 buckets (counts 0 .. 32) and 256 threads for
// the 16- and 32-piece builds (33 792 B), 65 buckets (counts 0 .. 64) and 128 threads for the 64-piece build (33 280 B; 256 rows
// of 65 would be 66 560 B).  The order is a property of the input alone: both shapes give the same order wherever no count
// exceeds 32.  order_on_host runs the kernel's phases thread by thread on the CPU (tests/harness/launch_order_check.cpp).
#pragma once

#if defined(__HIPCC__)
#define LORDER_HD __host__ __device__ inline
#else
#define LORDER_HD inline
#endif

namespace launch_order {

constexpr int buckets_of(int P) { return P <= 32 ? 33 : 65; }
constexpr int threads_of(int P) { return P <= 32 ? 256 : 128; }
static_assert(threads_of(32) >= buckets_of(32) && threads_of(64) >= buckets_of(64), "one thread per bucket takes the prefix over the threads");
static_assert(threads_of(32) * buckets_of(32) * 4 <= 48 * 1024 && threads_of(64) * buckets_of(64) * 4 <= 48 * 1024, "the histogram is static LDS");

// a piece count outside 0 .. BUCKETS - 1 (a slot that was never built) sorts with the nearest count
template <int BUCKETS>
LORDER_HD int bucket(int pieces)
{
    return pieces < 0 ? 0 : (pieces > BUCKETS - 1 ? BUCKETS - 1 : pieces);
}

// the run of slots [lo, hi) of thread tid
LORDER_HD void run_of(int tid, int count, int threads, int* lo, int* hi)
{
    const int per = (count + threads - 1) / threads;
    const long long first = (long long)tid * per;
    *lo = first < count ? (int)first : count;
    *hi = *lo + per < count ? *lo + per : count;
}

// phase 1, every thread: row[m] = the slots of its run with m pieces
template <int BUCKETS>
LORDER_HD void count_run(const int* pieces, int lo, int hi, int* row)
{
    for (int m = 0; m < BUCKETS; ++m) row[m] = 0;
    for (int s = lo; s < hi; ++s) row[bucket<BUCKETS>(pieces[s])] += 1;
}

// phase 2, thread m < BUCKETS: the exclusive prefix of column m over the threads, i.e. in slot order; returns the column's total
template <int BUCKETS>
LORDER_HD int prefix_threads(int (*hist)[BUCKETS], int threads, int m)
{
    int acc = 0;
    for (int q = 0; q < threads; ++q) {
        const int c = hist[q][m];
        hist[q][m] = acc;
        acc += c;
    }
    return acc;
}

// phase 3, one thread: total[m] <- the first position of bucket m, most pieces first
template <int BUCKETS>
LORDER_HD void prefix_buckets(int* total)
{
    int acc = 0;
    for (int m = BUCKETS - 1; m >= 0; --m) {
        const int c = total[m];
        total[m] = acc;
        acc += c;
    }
}

// phase 4, every thread: its slots to their positions
template <int BUCKETS>
LORDER_HD void scatter_run(const int* pieces, int lo, int hi, int* row, const int* total, int* order)
{
    for (int s = lo; s < hi; ++s) {
        const int m = bucket<BUCKETS>(pieces[s]);
        order[total[m] + row[m]++] = s;
    }
}

#if !defined(__HIP_DEVICE_COMPILE__)
// the kernel's phases with its threads in turn; hist: THREADS * BUCKETS ints of scratch
template <int BUCKETS, int THREADS>
inline void order_on_host(const int* pieces, int count, int* order, int* hist_flat)
{
    int (*hist)[BUCKETS] = reinterpret_cast<int (*)[BUCKETS]>(hist_flat);
    int total[BUCKETS];
    int lo, hi;
    for (int tid = 0; tid < THREADS; ++tid) {
        run_of(tid, count, THREADS, &lo, &hi);
        count_run<BUCKETS>(pieces, lo, hi, hist[tid]);
    }
    for (int m = 0; m < BUCKETS; ++m) total[m] = prefix_threads<BUCKETS>(hist, THREADS, m);
    prefix_buckets<BUCKETS>(total);
    for (int tid = 0; tid < THREADS; ++tid) {
        run_of(tid, count, THREADS, &lo, &hi);
        scatter_run<BUCKETS>(pieces, lo, hi, hist[tid], total, order);
    }
}
// the launch order of a handle of piece capacity P (16, 32 or 64)
inline void order_on_host(const int* pieces, int count, int P, int* order, int* hist_flat)
{
    if (P <= 32) order_on_host<buckets_of(32), threads_of(32)>(pieces, count, order, hist_flat);
    else order_on_host<buckets_of(64), threads_of(64)>(pieces, count, order, hist_flat);
}
#endif

} // namespace launch_order
