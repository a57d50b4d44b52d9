// laser_scan_launch.h -- launch interface between backend_capi.hip and laser_scan.hip.  Apart from backend_kernels.h because it
// includes laser_scan.h, whose contraction pragma must not reach the translation units of the other kernels
#pragma once

#include <hip/hip_runtime.h>

#include "laser_scan.h"

namespace backend {

// laser scans of the resident world cloud (arithmetic and contract in laser_scan.h): one workgroup per scan; laser_range_kernel
// keeps the range image in LDS, laser_perspective_kernel compacts the points within the horizon
struct LaserArgs {
    int count, n_cloud, slots;     // slots per scan: hrz * vtc in range mode, the capacity in perspective mode
    laser::Derived d;
    const float* cloud;            // [n_cloud][3]
    const double* poses;           // x, y, yaw of scan i at (char*)poses + i * pose_stride (bytes)
    int pose_stride;
    const double* tables;          // laser::make_tables
    double* image;                 // [count][hrz * vtc] (range mode)
    float *laser_pts, *world_pts;  // [count][slots][3]
    int* index;                    // [count][slots]
    float* compact;                // [count][slots][3] (range mode)
    int *n_points, *status;        // [count]
};
// the kernels read their arguments from d_args (device memory, filled in stream order before the launch)
hipError_t laser_scan(const LaserArgs* d_args, int count, int perspective, int bins, hipStream_t s);
// registers the image's LDS size with the runtime (once per device, not in stream order: call before the first scan)
hipError_t laser_configure();

} // namespace backend
