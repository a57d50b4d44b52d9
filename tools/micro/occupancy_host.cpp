// occupancy_host.cpp -- csrc/occupancy_update.h on one host core: the time of occ::integrate_scan per scan, for the comparison
// that tools/map_integrate.py prints.
//   usage: occupancy_host <points file: n float32 pairs> nx ny x_lo y_lo res range perspective odom_x odom_y runs
//   out:   one line, microseconds per scan for every run
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "occupancy_update.h"

int main(int argc, char** argv)
{
    if (argc != 12) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<float> pts;
    float buf[2];
    while (std::fread(buf, sizeof(float), 2, f) == 2) { pts.push_back(buf[0]); pts.push_back(buf[1]); }
    std::fclose(f);
    const int nx = std::atoi(argv[2]), ny = std::atoi(argv[3]);
    const double x_lo = std::atof(argv[4]), y_lo = std::atof(argv[5]), res = std::atof(argv[6]), range = std::atof(argv[7]);
    const bool perspective = std::atoi(argv[8]) != 0;
    const double ox = std::atof(argv[9]), oy = std::atof(argv[10]);
    const int runs = std::atoi(argv[11]);
    if (nx < 2 || ny < 2 || !(res > 0.0) || runs < 1) return 2;
    const size_t cells = (size_t)nx * ny;
    occ::Map m{};
    m.g = occ::make_geom(nx, ny, x_lo, y_lo, res);
    m.L = occ::LogOdds{occ::logit(0.99), occ::logit(0.35), occ::logit(0.12), occ::logit(0.90), occ::logit(0.80)};
    std::vector<unsigned char> grid(cells, 0), mx(nx), my(ny);
    std::vector<double> lo(cells, m.L.min - occ::UNKNOWN_FLAG), row(occ::lattice_cap(range, res));
    std::vector<int> hit(cells, 0), all(cells, 0);
    m.grid = grid.data(); m.log_odds = lo.data(); m.count_hit = hit.data(); m.count_all = all.data();
    m.mark_x = mx.data(); m.mark_y = my.data(); m.row = row.data();
    for (int r = 0; r < runs; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        if (occ::integrate_scan(m, pts.data(), (int)(pts.size() / 2), 8, ox, oy, range, perspective) != occ::SCAN_OK) return 3;
        const auto t1 = std::chrono::steady_clock::now();
        std::printf("%.1f ", std::chrono::duration<double, std::micro>(t1 - t0).count());
    }
    long occupied = 0;
    for (size_t c = 0; c < cells; ++c) occupied += grid[c] == occ::OCCUPIED;
    std::printf("\n%ld\n", occupied);
    return 0;
}
