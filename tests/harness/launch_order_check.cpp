// launch_order_check.cpp -- csrc/launch_order.h on the CPU (tests/test_backend_long_cpu.py): the launch order of the piece counts in
// a text file by launch_order::order_on_host, the phases of launch_order_kernel with its threads in turn.
//   usage: launch_order_check <file>
//   file:  P count, then `count` piece counts
//   out:   the order, one slot per line
#include <cstdio>
#include <vector>

#include "launch_order.h"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int P = 0, count = 0;
    if (std::fscanf(f, "%d %d", &P, &count) != 2 || count < 0) return 3;
    std::vector<int> pieces((size_t)count), order((size_t)count, -1);
    for (int& v : pieces)
        if (std::fscanf(f, "%d", &v) != 1) return 3;
    std::fclose(f);
    // on the heap, at its exact size: the address sanitizer sees an overrun of the histogram
    std::vector<int> hist((size_t)launch_order::threads_of(P) * launch_order::buckets_of(P));
    launch_order::order_on_host(pieces.data(), count, P, order.data(), hist.data());
    for (int v : order) std::printf("%d\n", v);
    return 0;
}
