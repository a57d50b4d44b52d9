// ltv_host_plan_check.cpp -- csrc/ltv_host_plan.h on the CPU (tests/test_ltv_host_plan_cpu.py builds it with the address and
// undefined-behaviour sanitizers and runs it as a child process).
// usage: ltv_host_plan_check FILE
// FILE: one request per line, answered by one line:
//   R cap total max_ticks      -> next_slot count n_runs {slot rows}...
//   U odom_every a b           -> updates_within(a, b), then the update ticks among a + 1 .. b
//   G B T                      -> stage_bytes(B, T)
//   C capacity {d|i}N ...      -> a cursor over `capacity` bytes takes the regions in order (d: N doubles, i: N ints); per region its
//                                 offset from the base, or -1 where it was refused; then ok() and used().  Every region handed out is
//                                 written from end to end: a region past the slab is the sanitizer's to find.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../alore_legged_manipulator_amd/csrc/ltv_host_plan.h"

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    char kind[8];
    while (std::fscanf(f, "%7s", kind) == 1) {
        if (kind[0] == 'R') {
            long long cap, total, max_ticks;
            if (std::fscanf(f, "%lld %lld %lld", &cap, &total, &max_ticks) != 3) break;
            const ltv_plan::RingRuns r = ltv_plan::ring_newest(total, cap, max_ticks);
            std::printf("%lld %lld %d", ltv_plan::ring_next_slot(total, cap), r.count, r.n);
            for (int k = 0; k < r.n; ++k) std::printf(" %lld %lld", r.run[k].slot, r.run[k].rows);
            std::printf("\n");
        } else if (kind[0] == 'U') {
            int every;
            long a, b;
            if (std::fscanf(f, "%d %ld %ld", &every, &a, &b) != 3) break;
            std::printf("%ld", ltv_plan::updates_within(a, b, every));
            for (long n = a + 1; n <= b; ++n)
                if (ltv_plan::is_update_tick(n, every)) std::printf(" %ld", n);
            std::printf("\n");
        } else if (kind[0] == 'G') {
            unsigned long long B, T;
            if (std::fscanf(f, "%llu %llu", &B, &T) != 2) break;
            std::printf("%zu\n", ltv_plan::stage_bytes((size_t)B, (size_t)T));
        } else if (kind[0] == 'C') {
            unsigned long long capacity;
            if (std::fscanf(f, "%llu", &capacity) != 1) break;
            char* slab = static_cast<char*>(::operator new(capacity ? (size_t)capacity : 1)); // exactly the capacity: a byte more is out of bounds
            ltv_plan::StageCursor cur(slab, (size_t)capacity);
            char what;
            unsigned long long n;
            int c;
            while ((c = std::fgetc(f)) == ' ')
                if (std::fscanf(f, "%c%llu", &what, &n) == 2) {
                    char* p = what == 'd' ? reinterpret_cast<char*>(cur.take<double>((size_t)n)) : reinterpret_cast<char*>(cur.take<int>((size_t)n));
                    if (p) std::memset(p, 0x5a, (size_t)n * (what == 'd' ? sizeof(double) : sizeof(int)));
                    std::printf("%lld ", p ? (long long)(p - slab) : -1ll);
                }
            std::printf("%d %zu\n", cur.ok() ? 1 : 0, cur.used());
            ::operator delete(slab);
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
