// laser_scan.hip -- laser scans of the resident world cloud for a batch of sensor poses (alore_backend_laser_scan); arithmetic and
// contract in laser_scan.h.  One workgroup of 256 threads per scan, a brute-force pass over the whole cloud: at the launch file's
// horizon a third of the world is in range anyway (DESIGN 7b says what was measured at the short horizon).
//
// RANGE MODE (laser_range_kernel).  The range image lives in LDS, one 64-bit word per bin, initialised to the bits of 9999.0.
// Distances are non-negative doubles, so their bit patterns order as unsigned integers and the update is an LDS atomicMin on
// unsigned long long (ds_min_u64).  Threads stride over the cloud; the range cull comes first (six multiplies and adds), the square
// roots and the two atan2 run for survivors only.  After a barrier the bins are walked in chunks of 256, one bin per thread: the
// image, the laser-frame and the world-frame point go to slot x * vtc + y (NaN where the bin was not hit), and a prefix sum over
// the chunk (one ballot and one population count per wavefront, four wavefront totals through LDS) gives every hit bin its place
// in the compact list, in x-major order: the order and the count of the reference's message.
// PERSPECTIVE MODE (laser_perspective_kernel).  No image.  A wavefront compacts its survivors with one ballot and one LDS add:
// lane 0 reserves the wavefront's slots, every survivor writes at the reservation plus the number of survivors in lower lanes.
// The order of the wavefronts' reservations is not fixed, so the order within a scan is not; the source index is written beside
// every point.  A survivor beyond the capacity is counted and not written.
// Neither kernel has a thread-dependent branch round a barrier: the pose, the mode and the chunk count are the same in every thread.
#include "laser_scan_launch.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace backend {

namespace ls = laser;

constexpr int LASER_THREADS = 256, LASER_WAVES = LASER_THREADS / 64;

extern __shared__ __align__(16) unsigned long long laser_lds[];

__device__ inline void store3(float* p, const float* v) { p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; }

__device__ inline ls::Pose read_pose(const LaserArgs& a, int scan)
{
    const double* p = (const double*)((const char*)a.poses + (size_t)scan * a.pose_stride);
    return ls::make_pose(p[0], p[1], p[2]);
}

__global__ __launch_bounds__(LASER_THREADS) void laser_range_kernel(const LaserArgs* __restrict__ gp)
{
    __shared__ int wave_total[LASER_WAVES];
    const LaserArgs& a = *gp;
    const ls::Derived& d = a.d;
    const int scan = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bins = d.hrz * d.vtc; // == a.slots
    const ls::Pose o = read_pose(a, scan);
    unsigned long long* img = laser_lds;
    const unsigned long long empty = ls::bits_of(ls::EMPTY);
    for (int b = tid; b < bins; b += LASER_THREADS) img[b] = empty;
    __syncthreads();
    if (o.ok) {
        const double* cos_vtc = a.tables + 2 * d.hrz;
        for (int i = tid; i < a.n_cloud; i += LASER_THREADS) {
            const float* p = a.cloud + 3 * (size_t)i;
            const ls::Seen v = ls::see(d, o, p[0], p[1], p[2]);
            if (!v.in_range) continue;
            ls::range_point(d, o, v, cos_vtc, [&](int b, double dis) { atomicMin(&img[b], (unsigned long long)ls::bits_of(dis)); });
        }
    }
    __syncthreads();
    const size_t base = (size_t)scan * bins;
    double* image = a.image + base;
    float *lp = a.laser_pts + base * 3, *wp = a.world_pts + base * 3, *cp = a.compact + base * 3;
    int* index = a.index + base;
    int running = 0;
    for (int first = 0; first < bins; first += LASER_THREADS) {
        const int b = first + tid;
        const unsigned long long w = b < bins ? img[b] : empty;
        const bool hit = w < empty;
        const unsigned long long vote = __ballot(hit);
        if (lane == 0) wave_total[wave] = __popcll(vote);
        __syncthreads();
        int before = running, all = 0;
        for (int k = 0; k < LASER_WAVES; ++k) {
            const int t = wave_total[k];
            if (k < wave) before += t;
            all += t;
        }
        if (b < bins) {
            float l3[3], w3[3];
            image[b] = ls::double_of(w);
            if (hit) {
                const int x = b / d.vtc;
                ls::bin_point(d, a.tables, x, b - x * d.vtc, ls::double_of(w), l3);
                ls::world_point(o, l3, w3);
                const int at = before + __popcll(vote & ((1ull << lane) - 1ull));
                store3(cp + 3 * (size_t)at, l3);
                index[at] = b;
            } else {
                ls::nan_point(l3);
                ls::nan_point(w3);
            }
            store3(lp + 3 * (size_t)b, l3);
            store3(wp + 3 * (size_t)b, w3);
        }
        running += all;
        __syncthreads(); // wave_total is written again in the next chunk
    }
    for (int k = running + tid; k < bins; k += LASER_THREADS) {
        float n3[3];
        ls::nan_point(n3);
        store3(cp + 3 * (size_t)k, n3);
        index[k] = -1;
    }
    if (tid == 0) {
        a.n_points[scan] = running;
        a.status[scan] = o.ok ? ls::OK : ls::E_POSE;
    }
}

__global__ __launch_bounds__(LASER_THREADS) void laser_perspective_kernel(const LaserArgs* __restrict__ gp)
{
    __shared__ int survivors;
    const LaserArgs& a = *gp;
    const ls::Derived& d = a.d;
    const int scan = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int cap = a.slots;
    const ls::Pose o = read_pose(a, scan);
    const size_t base = (size_t)scan * cap;
    float *lp = a.laser_pts + base * 3, *wp = a.world_pts + base * 3;
    int* index = a.index + base;
    if (tid == 0) survivors = 0;
    __syncthreads();
    if (o.ok) {
        const int rounds = (a.n_cloud + LASER_THREADS - 1) / LASER_THREADS;
        for (int r = 0; r < rounds; ++r) { // whole wavefronts go round together: the ballot sees all 64 lanes
            const int i = r * LASER_THREADS + tid;
            float p3[3] = {0.f, 0.f, 0.f};
            ls::Seen v{};
            bool in = false;
            if (i < a.n_cloud) {
                const float* p = a.cloud + 3 * (size_t)i;
                p3[0] = p[0]; p3[1] = p[1]; p3[2] = p[2];
                v = ls::see(d, o, p3[0], p3[1], p3[2]);
                in = v.in_range;
            }
            const unsigned long long vote = __ballot(in);
            if (vote == 0) continue; // the same in all lanes of the wavefront
            int start = 0;
            if (lane == 0) start = atomicAdd(&survivors, __popcll(vote));
            start = __shfl(start, 0);
            const int at = start + __popcll(vote & ((1ull << lane) - 1ull));
            if (in && at < cap) {
                float l3[3];
                ls::perspective_point(o, v, l3);
                store3(lp + 3 * (size_t)at, l3);
                store3(wp + 3 * (size_t)at, p3);
                index[at] = i;
            }
        }
    }
    __syncthreads();
    const int count = survivors;
    for (int k = (count < cap ? count : cap) + tid; k < cap; k += LASER_THREADS) {
        float n3[3];
        ls::nan_point(n3);
        store3(lp + 3 * (size_t)k, n3);
        store3(wp + 3 * (size_t)k, n3);
        index[k] = -1;
    }
    if (tid == 0) {
        a.n_points[scan] = count;
        a.status[scan] = !o.ok ? ls::E_POSE : count > cap ? ls::E_CAPACITY : ls::OK;
    }
}

static size_t laser_lds_bytes(int bins) { return sizeof(unsigned long long) * (size_t)bins; }

hipError_t laser_configure()
{
    return hipFuncSetAttribute((const void*)laser_range_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)laser_lds_bytes(ls::MAX_BINS));
}

hipError_t laser_scan(const LaserArgs* d_args, int count, int perspective, int bins, hipStream_t s)
{
    void* args[] = {&d_args};
    hipError_t e = perspective ? hipLaunchKernel((const void*)laser_perspective_kernel, dim3(count), dim3(LASER_THREADS), args, 0, s)
                               : hipLaunchKernel((const void*)laser_range_kernel, dim3(count), dim3(LASER_THREADS), args, laser_lds_bytes(bins), s);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

} // namespace backend
