// occupancy_check.cpp -- csrc/occupancy_update.h on the CPU (tests/test_occupancy_cpu.py): runs the scans of a text file through
// occ::integrate_scan and prints the map after every scan, every double with 17 digits.
//   usage: occupancy_check <scans file>
//   file:  nx ny x_lo y_lo res range perspective  hit miss min max occ  floats_per_point seeded n_scans
//          with seeded != 0: nx * ny cell states;  then per scan:  n ox oy  x0 y0 ... x(n-1) y(n-1)
//   out:   per scan "status cells_with_a_count_left", then nx lines of ny states and nx lines of ny log-odds
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "occupancy_update.h"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int nx, ny, perspective, floats, seeded, n_scans;
    double x_lo, y_lo, res, range;
    occ::Map m{};
    if (std::fscanf(f, "%d %d %lf %lf %lf %lf %d %lf %lf %lf %lf %lf %d %d %d", &nx, &ny, &x_lo, &y_lo, &res, &range, &perspective, &m.L.hit,
                    &m.L.miss, &m.L.min, &m.L.max, &m.L.occ, &floats, &seeded, &n_scans) != 15 || nx < 2 || ny < 2 || floats < 2)
        return 3;
    m.g = occ::make_geom(nx, ny, x_lo, y_lo, res);
    const size_t cells = (size_t)nx * ny;
    // every array on the heap with its exact size: the address sanitizer sees an overrun
    m.grid = new unsigned char[cells]();
    m.log_odds = new double[cells];
    m.count_hit = new int[cells]();
    m.count_all = new int[cells]();
    m.mark_x = new unsigned char[nx];
    m.mark_y = new unsigned char[ny];
    m.row = new double[occ::lattice_cap(range, res)];
    for (size_t c = 0; c < cells; ++c) m.log_odds[c] = m.L.min - occ::UNKNOWN_FLAG;
    if (seeded)
        for (size_t c = 0; c < cells; ++c) {
            int s;
            if (std::fscanf(f, "%d", &s) != 1) return 3;
            m.grid[c] = (unsigned char)s;
        }
    for (int k = 0; k < n_scans; ++k) {
        int n;
        double ox, oy;
        if (std::fscanf(f, "%d %lf %lf", &n, &ox, &oy) != 3 || n < 0) return 3;
        float* pts = new float[(size_t)n * floats];
        for (int i = 0; i < n; ++i) {
            for (int d = 0; d < floats; ++d) pts[(size_t)i * floats + d] = std::numeric_limits<float>::quiet_NaN(); // padding is never read
            if (std::fscanf(f, "%f %f", &pts[(size_t)i * floats], &pts[(size_t)i * floats + 1]) != 2) return 3;
        }
        const int status = occ::integrate_scan(m, pts, n, floats * (int)sizeof(float), ox, oy, range, perspective != 0);
        delete[] pts;
        long left = 0;
        for (size_t c = 0; c < cells; ++c) left += (m.count_all[c] != 0) + (m.count_hit[c] != 0);
        std::printf("%d %ld\n", status, left);
        for (int x = 0; x < nx; ++x) {
            for (int y = 0; y < ny; ++y) std::printf("%d ", (int)m.grid[(size_t)x * ny + y]);
            std::printf("\n");
        }
        for (int x = 0; x < nx; ++x) {
            for (int y = 0; y < ny; ++y) std::printf("%.17g ", m.log_odds[(size_t)x * ny + y]);
            std::printf("\n");
        }
    }
    std::fclose(f);
    delete[] m.grid; delete[] m.log_odds; delete[] m.count_hit; delete[] m.count_all; delete[] m.mark_x; delete[] m.mark_y; delete[] m.row;
    return 0;
}
