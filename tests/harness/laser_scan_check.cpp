// laser_scan_check.cpp -- csrc/laser_scan.h on the CPU (tests/test_laser_scan_cpu.py): runs the poses of a text file through
// laser::scan_one (the header's own loop over points, image, bin points and compaction) and prints every output, doubles with 17
// digits and floats with 9.
//   usage: laser_scan_check <scene file>
//   file:  the nine parameters in the order of laser::Params, then n_points n_poses capacity;  n_points x "x y z";  n_poses x "x y yaw"
//   out:   per pose "status count", then one line each: the image [bins] (empty in perspective mode), the laser-frame points
//          [slots][3], the world-frame points [slots][3], the index [slots], the compact points [slots][3] (empty in perspective mode)
#include <cstdio>
#include <cstdlib>

#include "laser_scan.h"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    laser::Params p;
    int n, n_poses, capacity;
    if (std::fscanf(f, "%lf %lf %d %d %lf %d %lf %d %d %d %d %d", &p.sensing_horizon, &p.pc_resolution, &p.hrz_laser_line_num, &p.vtc_laser_line_num,
                    &p.vtc_laser_range_dgr, &p.hrz_limited, &p.hrz_laser_range_dgr, &p.use_resolution_filter, &p.if_perspective, &n, &n_poses,
                    &capacity) != 12 || n < 0 || n_poses < 0 || capacity < 0)
        return 3;
    if (!laser::valid(p)) return 4;
    const laser::Derived d = laser::derive(p);
    // every array on the heap with its exact size: the address sanitizer sees an overrun
    float* cloud = new float[3 * (size_t)n];
    for (int i = 0; i < 3 * n; ++i) {
        double v;
        if (std::fscanf(f, "%lf", &v) != 1) return 3;
        cloud[i] = (float)v; // exact: the file holds float values
    }
    double* tables = new double[(size_t)laser::table_doubles(d)];
    laser::make_tables(d, tables);
    const int bins = d.hrz * d.vtc, slots = d.perspective ? capacity : bins;
    for (int k = 0; k < n_poses; ++k) {
        double x, y, yaw;
        if (std::fscanf(f, "%lf %lf %lf", &x, &y, &yaw) != 3) return 3;
        double* image = new double[d.perspective ? 0 : bins];
        float *lp = new float[3 * (size_t)slots], *wp = new float[3 * (size_t)slots], *cp = new float[d.perspective ? 0 : 3 * (size_t)slots];
        int* index = new int[slots];
        int count = -1;
        const int status = laser::scan_one(d, tables, cloud, n, x, y, yaw, capacity, image, lp, wp, index, cp, &count);
        std::printf("%d %d\n", status, count);
        if (!d.perspective)
            for (int b = 0; b < bins; ++b) std::printf("%.17g ", image[b]);
        std::printf("\n");
        const bool defined = status != laser::E_CAPACITY; // on overflow the slots are unspecified: the tail was never written
        for (int i = 0; i < 3 * slots; ++i) std::printf("%.9g ", defined ? lp[i] : 0.0f);
        std::printf("\n");
        for (int i = 0; i < 3 * slots; ++i) std::printf("%.9g ", defined ? wp[i] : 0.0f);
        std::printf("\n");
        for (int i = 0; i < slots; ++i) std::printf("%d ", defined ? index[i] : 0);
        std::printf("\n");
        if (!d.perspective)
            for (int i = 0; i < 3 * slots; ++i) std::printf("%.9g ", cp[i]);
        std::printf("\n");
        delete[] image; delete[] lp; delete[] wp; delete[] cp; delete[] index;
    }
    std::fclose(f);
    delete[] cloud; delete[] tables;
    return 0;
}
