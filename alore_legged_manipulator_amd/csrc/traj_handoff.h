// traj_handoff.h -- the host-side rules of the hand-over to a replanned trajectory (no HIP: tests/test_traj_handoff_cpu.py compiles
// it with g++ alone).  The device part is traj_handoff.hip; the calls are alore_nmpc_refs_set_pending_* / alore_nmpc_refs_promote.
//
// The reference's controller keeps a new trajectory in new_traj_ and goes on tracking traj_ until now > new_traj_start_time_
// (nmpc_controller/src/mpc.cpp:177-182); a message that arrives while another is still pending promotes the older one first,
// whatever its start time (mpc.cpp:151-156).  Here every robot has a pending slot beside its active one, and
//   * promote_due       is that rule for one robot (the kernel evaluates the same expression),
//   * PendingTimes      is what the handle remembers of the start times it was given, so that a tick enqueues a promotion only
//                       while one can still be due,
//   * split_run         cuts a run of n ticks where a promotion has to go between two ticks.
#ifndef ALORE_TRAJ_HANDOFF_H
#define ALORE_TRAJ_HANDOFF_H

#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#define TRAJ_HANDOFF_HD __host__ __device__
#else
#define TRAJ_HANDOFF_HD
#endif

namespace traj_handoff {

// status word of a slot after alore_nmpc_refs_set_pending_* (include/alore_nmpc.h: ALORE_NMPC_PENDING_*)
enum : int { kWritten = 0, kNotAddressed = 1, kTooManyPieces = -1, kTooManyCheckpoints = -2 };

// the comparison is strict, as in the reference: a tick AT the start time still tracks the old trajectory
TRAJ_HANDOFF_HD inline bool promote_due(bool pending_valid, double pending_start, double now, bool forced)
{
    return pending_valid && (forced || now > pending_start);
}

// the time of tick t of a run: always from the run's own t0 and the GLOBAL tick index.  (t0 + dt_tick * k) + dt_tick * j differs from
// t0 + dt_tick * (k + j) in the last bits, and so would the references sampled at it.
inline double tick_time(double t0, double dt_tick, long t) { return t0 + dt_tick * (double)t; }

// the start times of pending entries that may not have been promoted yet
struct PendingTimes {
    std::vector<double> t;
    bool any() const { return !t.empty(); }
    void add(double start)
    {
        for (double s : t)
            if (s == start) return;
        t.push_back(start);
    }
    bool due(double now) const
    {
        for (double s : t)
            if (now > s) return true;
        return false;
    }
    // a promotion for `now` over every robot has been enqueued: whatever started before it is active
    void promoted(double now)
    {
        size_t k = 0;
        for (double s : t)
            if (!(now > s)) t[k++] = s;
        t.resize(k);
    }
};

// ticks [first, first + count) of a run; promote: a promotion with now = tick_time(t0, dt_tick, first) goes in front of them
struct Segment {
    int first, count;
    bool promote;
};

// A run of n ticks at tick_time(t0, dt_tick, 0 .. n - 1) with the outstanding start times `starts`: for every start time the FIRST
// tick whose time exceeds it carries the promotion (a tick-by-tick run promotes there, and finds nothing to do afterwards).  A start
// before tick 0 promotes in front of the run and cuts nothing, one after the last tick does nothing, several in one tick cut once.
// Every segment is issued as a complete run of its own (with its trailing plant step), so the fused runs never read the store for
// two ticks across a promotion.
inline std::vector<Segment> split_run(double t0, double dt_tick, int n, const double* starts, size_t n_starts)
{
    std::vector<Segment> out;
    if (n <= 0) return out;
    std::vector<char> cut((size_t)n, 0);
    for (size_t i = 0; i < n_starts; ++i)
        for (int t = 0; t < n; ++t)
            if (tick_time(t0, dt_tick, t) > starts[i]) { cut[(size_t)t] = 1; break; }
    Segment cur{0, 0, cut[0] != 0};
    for (int t = 0; t < n; ++t) {
        if (t > 0 && cut[(size_t)t]) {
            out.push_back(cur);
            cur = Segment{t, 0, true};
        }
        ++cur.count;
    }
    out.push_back(cur);
    return out;
}

} // namespace traj_handoff
#endif
