// backend_classes_check.cpp -- csrc/backend_classes.h on the CPU (tests/test_backend_classes_cpu.py): the validation of a class
// against the handle's config, the effective xv of a config, and the per-class reduction of status records.
//   backend_classes_check classes IN OUT   IN: int n, the handle's alore_backend_config, n class configs
//                                          OUT (text): per class "k field|ok xv" (xv with 17 significant digits)
//   backend_classes_check reduce IN OUT    IN: int count, n_classes, P, has_class_of; class_of [count]; status [count]; T [count][P]
//                                          OUT (binary): alore_backend_class_stat [n_classes]
// g++ -std=c++17 -ffp-contract=off -I alore_legged_manipulator_amd/csrc; stand-alone, no GPU, no HIP.
#include <cstdio>
#include <cstring>
#include <vector>

#include "backend_classes.h"

static_assert(sizeof(alore_backend_class_stat) == 48, "alore_backend_class_stat");
static_assert(sizeof(alore_backend_class_view) == 48, "alore_backend_class_view");

template <class T>
static bool get(std::FILE* f, T* p, size_t n)
{
    return n == 0 || std::fread(p, sizeof(T), n, f) == n;
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    std::FILE* in = std::fopen(argv[2], "rb");
    std::FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    int rc = 0;
    if (!std::strcmp(argv[1], "classes")) {
        int n = 0;
        alore_backend_config handle;
        if (!get(in, &n, 1) || n < 0 || n > bclass::MAX_CLASSES || !get(in, &handle, 1)) return 3;
        std::vector<alore_backend_config> k((size_t)n);
        if (!get(in, k.data(), (size_t)n)) return 3;
        for (int i = 0; i < n; ++i) {
            const char* f = bclass::class_error(k[(size_t)i], handle);
            std::fprintf(out, "%d %s %.17g\n", i, f ? f : "ok", bclass::effective_xv(k[(size_t)i]));
        }
    } else if (!std::strcmp(argv[1], "reduce")) {
        int hdr[4];
        if (!get(in, hdr, 4) || hdr[0] < 0 || hdr[1] < 1 || hdr[1] > bclass::MAX_CLASSES || hdr[2] < 1) return 3;
        const size_t count = (size_t)hdr[0], P = (size_t)hdr[2];
        std::vector<int> class_of(count);
        std::vector<alore_backend_status> status(count);
        std::vector<double> T(count * P);
        if (!get(in, class_of.data(), count) || !get(in, status.data(), count) || !get(in, T.data(), count * P)) return 3;
        std::vector<alore_backend_class_stat> stat((size_t)hdr[1]);
        bclass::reduce(hdr[3] ? class_of.data() : nullptr, status.data(), T.data(), hdr[2], hdr[0], hdr[1], stat.data());
        if (std::fwrite(stat.data(), sizeof(alore_backend_class_stat), stat.size(), out) != stat.size()) rc = 4;
    } else {
        rc = 2;
    }
    std::fclose(in);
    if (std::fclose(out) != 0) rc = 4;
    return rc;
}
