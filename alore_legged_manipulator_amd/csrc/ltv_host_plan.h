// ltv_host_plan.h -- the host bookkeeping of the closed loops as pure functions (internal): the trace ring, the filter's update
// schedule, the staging slab.  Plain C++17: no HIP, no handle type, no environment -- tests/harness/ltv_host_plan_check.cpp compiles
// it with g++ alone.  Read by ltv_mpc_capi.hip (all three) and icr_ekf.hip (the schedule).
#ifndef ALORE_LTV_HOST_PLAN_H
#define ALORE_LTV_HOST_PLAN_H

#include <cstddef>
#include <cstdint>

namespace ltv_plan {

// ---- the trace ring: `cap` slots, record number n (n = 0, 1, ... since the trace was emptied) lies in slot n % cap

// the slot the next record takes after `total` records; -1: no ring (cap == 0), nothing is recorded
inline long long ring_next_slot(long long total, long long cap) { return cap > 0 ? total % cap : -1; }

// the newest min(total, cap, max_ticks) records, oldest first: `count` of them in n <= 2 runs of consecutive slots (the range wraps
// at most once)
struct RingRuns {
    long long count;
    int n;
    struct Run { long long slot, rows; } run[2];
};
inline RingRuns ring_newest(long long total, long long cap, long long max_ticks)
{
    RingRuns r = {0, 0, {{0, 0}, {0, 0}}};
    long long count = total < cap ? total : cap;
    if (count > max_ticks) count = max_ticks;
    if (count <= 0) return r; // (cap == 0 ends here: no division by it below)
    r.count = count;
    const long long first = (total - count) % cap;
    const long long head = cap - first < count ? cap - first : count;
    r.run[r.n++] = {first, head};
    if (head < count) r.run[r.n++] = {0, count - head};
    return r;
}

// ---- the filter's update schedule: the handle counts closed-loop ticks 1, 2, ... since the filter's reset; every odom_every-th
// (odom_every >= 1) carries a pose update

inline bool is_update_tick(long n, int odom_every) { return n % odom_every == 0; }
// updates among ticks a + 1 .. b (0 <= a <= b)
inline long updates_within(long a, long b, int odom_every) { return b / odom_every - a / odom_every; }

// ---- the pinned staging slab of an LTV handle made for B robots and a horizon of T

// large enough for every carve of the C ABI; the largest is alore_ltv_results': output [B][T][2], xopt [B][T + 1][3], 2 B ints
inline size_t stage_bytes(size_t B, size_t T) { return sizeof(double) * B * ((T + 1) * 3 + T * 5 + 8) + sizeof(int) * B * 4 + 1024; }

// hands out typed regions of (base, capacity) one behind the other, each aligned for its type.  A region that does not fit is
// refused: take() returns null, nothing behind the slab is touched, and ok() stays false.
class StageCursor {
public:
    StageCursor(void* base, size_t capacity) : base_(static_cast<char*>(base)), cap_(capacity) {}
    template <class T>
    T* take(size_t n)
    {
        const size_t pad = (alignof(T) - (reinterpret_cast<uintptr_t>(base_) + used_) % alignof(T)) % alignof(T);
        if (!ok_ || pad > cap_ - used_ || n > (cap_ - used_ - pad) / sizeof(T)) { ok_ = false; return nullptr; }
        T* p = reinterpret_cast<T*>(base_ + used_ + pad);
        used_ += pad + n * sizeof(T);
        return p;
    }
    bool ok() const { return ok_; }
    size_t used() const { return used_; }

private:
    char* base_;
    size_t cap_, used_ = 0;
    bool ok_ = true;
};

} // namespace ltv_plan
#endif
