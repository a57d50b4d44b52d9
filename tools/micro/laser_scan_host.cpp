// laser_scan_host.cpp -- csrc/laser_scan.h on one host core: the time of laser::scan_one per pose, for the comparison that
// tools/laser_scan.py prints.
//   usage: laser_scan_host <cloud file: n x 3 float32> <poses file: m x 3 float64> horizon pc_resolution hrz vtc vtc_range_dgr
//          hrz_limited hrz_range_dgr filter perspective capacity runs
//   out:   the time of every run over all poses in us, then "poses points sum_of_counts"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "laser_scan.h"

template <class T>
static bool read_all(const char* path, std::vector<T>& out, size_t per)
{
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::vector<T> buf(per);
    while (std::fread(buf.data(), sizeof(T), per, f) == per) out.insert(out.end(), buf.begin(), buf.end());
    std::fclose(f);
    return true;
}

int main(int argc, char** argv)
{
    if (argc != 14) return 2;
    std::vector<float> cloud;
    std::vector<double> poses;
    if (!read_all(argv[1], cloud, 3) || !read_all(argv[2], poses, 3)) return 2;
    const laser::Params p{std::atof(argv[3]), std::atof(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]), std::atof(argv[7]),
                          std::atoi(argv[8]), std::atof(argv[9]), std::atoi(argv[10]), std::atoi(argv[11])};
    const int capacity = std::atoi(argv[12]), runs = std::atoi(argv[13]);
    if (!laser::valid(p) || capacity < 0 || runs < 1) return 2;
    const laser::Derived d = laser::derive(p);
    std::vector<double> tables((size_t)laser::table_doubles(d));
    laser::make_tables(d, tables.data());
    const int n = (int)(cloud.size() / 3), m = (int)(poses.size() / 3);
    const size_t bins = (size_t)d.hrz * d.vtc, slots = d.perspective ? (size_t)capacity : bins;
    std::vector<double> image(bins);
    std::vector<float> lp(3 * slots + 3), wp(3 * slots + 3), cp(3 * slots + 3);
    std::vector<int> index(slots + 1);
    long total = 0;
    for (int r = 0; r < runs; ++r) {
        total = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < m; ++k) {
            int count = 0;
            laser::scan_one(d, tables.data(), cloud.data(), n, poses[3 * k], poses[3 * k + 1], poses[3 * k + 2], capacity, image.data(), lp.data(),
                            wp.data(), index.data(), cp.data(), &count);
            total += count;
        }
        const auto t1 = std::chrono::steady_clock::now();
        std::printf("%.1f ", std::chrono::duration<double, std::micro>(t1 - t0).count());
    }
    std::printf("\n%d %d %ld\n", m, n, total);
    return 0;
}
