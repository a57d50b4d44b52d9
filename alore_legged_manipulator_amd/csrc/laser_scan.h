// laser_scan.h -- laser scans of a world cloud, the arithmetic once (internal).
// Plain C++17: __host__ __device__ under hipcc, no HIP dependency otherwise.  What the reference's laser simulator publishes at a
// sensing tick (planning_ddr_opt/utils/laser_simulator/src/laser_sim_node.cpp: pt2LaserIdx :113-142, idx2Pt :152-160,
// perspectivePoints :343-421, renderSensedPoints :423-533, the parameters :540-581), stated so that it has exactly one answer.
// The small functions are what the kernels of laser_scan.hip run per thread; scan_one() strings them together serially and is
// what tests/harness/laser_scan_check.cpp and tools/micro/laser_scan_host.cpp run on the CPU.  The oracle is
// tests/laser_scan_cases.py (loops over points, a dis_map array, idx2Pt).
//
// THE CONTRACT
//   cloud    n points, three floats each; every coordinate is widened to double before anything else.
//   pose     the sensor at (x, y, 0) with yaw only (rcvOdometryCallbck :290-318); c = cos(yaw), s = sin(yaw).  A pose that is not
//            finite: status E_POSE, count 0, an empty image and NaN slots.
//   point    dx = px - x, dy = py - y, dz = pz;  hh = dx dx + dy dy;  d2 = hh + dz dz;  in range when d2 <= horizon * horizon;
//            dis = sqrt(d2);  vtc_rad = atan2(dz, sqrt(hh));  lx = dx c + dy s;  ly = (-dx) s + dy c;  hrz_rad = atan2(ly, lx).
//            This is pt2LaserIdx for a yaw-only rotation: the intersection with the laser plane is (px, py, 0).
//   derived  vtc_range_rad = dgr / 180 * PI;  vtc_res = vtc_range_rad / (double)(vtc - 1);  half_vtc = (vtc_range_rad + vtc_res)
//            / 2;  hrz_res = 2 * PI / (double)hrz;  half_hrz = hrz_dgr / 180 * PI / 2 (:554-564).
//   range    (renderSensedPoints) every bin of dis_map[hrz][vtc] starts at 9999.0.  A point in range with a finite dis > 0 is
//            dropped when |vtc_rad| >= half_vtc, or, hrz_limited, when |hrz_rad| >= half_hrz.  Its bin:
//            iy = floor((vtc_rad + half_vtc) / vtc_res), ix = floor((hrz_rad + (PI + hrz_res / 2)) / hrz_res), an index >= its line
//            number becomes 0 (the reference's quirk).  Without the filter, dis_map[ix][iy] = min(itself, dis).  With it, with
//            z = dis * cos_vtc[iy], t1 = min(floor(pc_resolution / (z * hrz_res)), (double)hrz), t2 = min(floor(pc_resolution /
//            (z * vtc_res)), (double)vtc), every bin ((ix + a + hrz) % hrz, iy + b) with |a| <= t1, |b| <= t2 and 0 <= iy + b < vtc
//            takes the minimum.  A bin is hit when something lowered it.  The image is a minimum over doubles: it does not depend
//            on the order of the points.
//   tables   cos_hrz[x] = cos(x * hrz_res - PI), sin_hrz[x] likewise, cos_vtc[y] = cos(y * vtc_res - vtc_range_rad / 2), sin_vtc[y]
//            likewise: hrz + vtc entries each, computed ONCE on the host (make_tables) and handed to whoever runs the rest, so
//            that everything after them is products of correctly rounded operations.
//   bin pt   idx2Pt: pz = sin_vtc[y] * dis;  q = cos_vtc[y] * dis;  px = cos_hrz[x] * q;  py = sin_hrz[x] * q;  the laser-frame
//            point is (float)px, (float)py, (float)pz -- the floats of the published cloud.
//   world    of a laser-frame point (fx, fy, fz), floats widened: ((x + c fx) - s fy, (y + s fx) + c fy, fz) in double, rounded to
//            float: what tf2::doTransform makes of the published cloud for a yaw-only transform (sdf_map.cpp:12-30).
//   outputs  range mode, per scan: the image [hrz][vtc]; slot x * vtc + y holds the laser-frame and the world-frame point of bin
//            (x, y), three NaN where the bin was not hit; the hit bins in x-major order (the order of the reference's message):
//            their number, index[k] = the bin of the k-th, compact[k] = its laser-frame point; index -1 and NaN from the count on.
//   perspective  (perspectivePoints) every point with d2 <= horizon * horizon, no angular test (the reference computes
//            pt2LaserIdx there and ignores its result): the laser-frame point ((float)lx, (float)ly, (float)dz), the world-frame
//            point = the source point verbatim, the source index.  The order within a scan is unspecified (the reference's is the
//            kd-tree's); consumers sort by index.  Slots from the count on hold NaN and index -1.  More survivors than the
//            capacity: status E_CAPACITY, the count is the true count, the slots are unspecified.
// DEVIATIONS from the reference, each with a test (tests/laser_scan_cases.py):
//   in range is decided on the double sum d2 (FLANN's radiusSearch compares sums of floats);
//   a point with a non-finite coordinate is skipped in both modes; a point with dis == 0 is skipped in range mode (its angles
//   are atan2(0, 0));
//   t1 and t2 are clamped in double before the cast to int -- the same value wherever the reference's cast of the unclamped
//   quotient is defined;
//   a horizontal spread of 2 t1 + 1 >= hrz bins visits every column once (the reference goes round the ring up to three times;
//   the minimum is idempotent);
//   half_hrz is computed whether or not hrz_limited is set (the reference leaves it 0 then and never reads it);
//   parameters the reference would divide by zero on, or that make no image, are refused (valid()).
#ifndef ALORE_LASER_SCAN_H
#define ALORE_LASER_SCAN_H

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define LS_HD __host__ __device__ inline
#else
#define LS_HD inline
#endif

namespace laser {

constexpr int MAX_BINS = 8192; // hrz * vtc: one 64-bit word each, 64 KiB of LDS
constexpr int OK = 0, E_POSE = -1, E_CAPACITY = -2;
constexpr double EMPTY = 9999.0;
constexpr double PI = 3.14159265358979323846; // M_PI

struct Params {
    double sensing_horizon, pc_resolution;
    int hrz_laser_line_num, vtc_laser_line_num;
    double vtc_laser_range_dgr;
    int hrz_limited;
    double hrz_laser_range_dgr;
    int use_resolution_filter, if_perspective;
};
// planner_sim.launch (detection_range_ 27.0, gridmap_interval_ 0.1, if_perspective_ true, hrz_limited_ false, 90 degrees) and
// config/perspective_laser.yaml (360 x 16 lines over 30 degrees, no filter).  config/normal_laser.yaml, the occluding sensor:
// sensing_horizon 10.0, vtc_laser_line_num 2, vtc_laser_range_dgr 10.0, hrz_laser_line_num 360, use_resolution_filter true
inline void default_params(Params* p)
{
    p->sensing_horizon = 27.0; p->pc_resolution = 0.1;
    p->hrz_laser_line_num = 360; p->vtc_laser_line_num = 16;
    p->vtc_laser_range_dgr = 30.0;
    p->hrz_limited = 0;
    p->hrz_laser_range_dgr = 90.0;
    p->use_resolution_filter = 0; p->if_perspective = 1;
}
// vtc < 2 divides by zero in the reference; more than MAX_BINS bins do not fit the image
inline bool valid(const Params& p)
{
    if (p.vtc_laser_line_num < 2 || p.hrz_laser_line_num < 1) return false;
    if ((long long)p.hrz_laser_line_num * p.vtc_laser_line_num > MAX_BINS) return false;
    if (!(p.sensing_horizon > 0.0) || !std::isfinite(p.sensing_horizon) || !(p.pc_resolution > 0.0) || !std::isfinite(p.pc_resolution)) return false;
    if (!(p.vtc_laser_range_dgr > 0.0) || !(p.vtc_laser_range_dgr < 180.0)) return false;
    if (p.hrz_limited && (!(p.hrz_laser_range_dgr > 0.0) || !std::isfinite(p.hrz_laser_range_dgr))) return false;
    return true;
}

struct Derived {
    int hrz, vtc, hrz_limited, filter, perspective;
    double horizon2, pc_resolution, vtc_range_rad, vtc_res, half_vtc, hrz_res, half_hrz;
};
LS_HD Derived derive(const Params& p)
{
    Derived d;
    d.hrz = p.hrz_laser_line_num; d.vtc = p.vtc_laser_line_num;
    d.hrz_limited = p.hrz_limited != 0; d.filter = p.use_resolution_filter != 0; d.perspective = p.if_perspective != 0;
    d.horizon2 = p.sensing_horizon * p.sensing_horizon;
    d.pc_resolution = p.pc_resolution;
    d.vtc_range_rad = p.vtc_laser_range_dgr / 180.0 * PI;
    d.vtc_res = d.vtc_range_rad / (double)(d.vtc - 1);
    d.half_vtc = (d.vtc_range_rad + d.vtc_res) / 2.0;
    d.hrz_res = 2 * PI / (double)d.hrz;
    d.half_hrz = p.hrz_laser_range_dgr / 180.0 * PI / 2.0;
    return d;
}

// the per-line tables, hrz + vtc entries each way: t[0 .. hrz) cos_hrz, [hrz .. 2 hrz) sin_hrz, then cos_vtc [vtc], sin_vtc [vtc].
// Host only: the one place where sin and cos of a line angle are taken
inline int table_doubles(const Derived& d) { return 2 * (d.hrz + d.vtc); }
inline void make_tables(const Derived& d, double* t)
{
    for (int x = 0; x < d.hrz; ++x) {
        const double a = x * d.hrz_res - PI;
        t[x] = std::cos(a);
        t[d.hrz + x] = std::sin(a);
    }
    for (int y = 0; y < d.vtc; ++y) {
        const double a = y * d.vtc_res - d.vtc_range_rad / 2.0;
        t[2 * d.hrz + y] = std::cos(a);
        t[2 * d.hrz + d.vtc + y] = std::sin(a);
    }
}

struct Pose {
    double x, y, c, s;
    bool ok;
};
LS_HD Pose make_pose(double x, double y, double yaw)
{
    Pose p;
    p.ok = std::isfinite(x) && std::isfinite(y) && std::isfinite(yaw);
    p.x = x; p.y = y;
    p.c = p.ok ? std::cos(yaw) : 1.0;
    p.s = p.ok ? std::sin(yaw) : 0.0;
    return p;
}

// a world point seen from the pose: the offsets and the two sums (no square root, no angle yet)
struct Seen {
    double dx, dy, dz, hh, d2;
    bool in_range; // false for a non-finite coordinate too
};
LS_HD Seen see(const Derived& d, const Pose& o, float px, float py, float pz)
{
    Seen v;
    v.dx = (double)px - o.x; v.dy = (double)py - o.y; v.dz = (double)pz;
    v.hh = v.dx * v.dx + v.dy * v.dy;
    v.d2 = v.hh + v.dz * v.dz;
    v.in_range = v.d2 <= d.horizon2; // NaN compares false; an infinite coordinate gives an infinite sum
    return v;
}
LS_HD double laser_x(const Pose& o, const Seen& v) { return v.dx * o.c + v.dy * o.s; }
LS_HD double laser_y(const Pose& o, const Seen& v) { return (-v.dx) * o.s + v.dy * o.c; }

LS_HD std::uint64_t bits_of(double v)
{
    std::uint64_t u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}
LS_HD double double_of(std::uint64_t u)
{
    double v;
    std::memcpy(&v, &u, sizeof(v));
    return v;
}

// renderSensedPoints for one point in range: lower(bin, dis) takes the minimum into bin = ix * vtc + iy.  Distances are
// non-negative doubles, so a caller may keep their bit patterns and order them as unsigned integers
template <class Lower>
LS_HD void range_point(const Derived& d, const Pose& o, const Seen& v, const double* cos_vtc, Lower&& lower)
{
    const double dis = std::sqrt(v.d2);
    if (!(dis > 0.0)) return;
    double vtc_rad = std::atan2(v.dz, std::sqrt(v.hh));
    if (std::fabs(vtc_rad) >= d.half_vtc) return;
    double hrz_rad = std::atan2(laser_y(o, v), laser_x(o, v));
    if (d.hrz_limited && std::fabs(hrz_rad) >= d.half_hrz) return;
    vtc_rad += d.half_vtc;
    int iy = (int)std::floor(vtc_rad / d.vtc_res);
    if (iy >= d.vtc) iy = 0;
    hrz_rad += PI + d.hrz_res / 2.0;
    int ix = (int)std::floor(hrz_rad / d.hrz_res);
    if (ix >= d.hrz) ix = 0;
    if (!d.filter) {
        lower(ix * d.vtc + iy, dis);
        return;
    }
    const double to_z_axis = dis * cos_vtc[iy];
    const double mesh_hrz = to_z_axis * d.hrz_res, mesh_vtc = to_z_axis * d.vtc_res;
    double f1 = std::floor(d.pc_resolution / mesh_hrz), f2 = std::floor(d.pc_resolution / mesh_vtc);
    if (!(f1 < (double)d.hrz)) f1 = (double)d.hrz; // std::min in double; a quotient that is not finite takes the line number
    if (!(f2 < (double)d.vtc)) f2 = (double)d.vtc;
    const int t1 = (int)f1, t2 = (int)f2;
    const int y0 = iy - t2 < 0 ? 0 : iy - t2, y1 = iy + t2 > d.vtc - 1 ? d.vtc - 1 : iy + t2;
    const bool whole_ring = 2 * t1 + 1 >= d.hrz;
    const int first = whole_ring ? 0 : -t1, last = whole_ring ? d.hrz - 1 : t1;
    for (int a = first; a <= last; ++a) {
        const int x = whole_ring ? a : (ix + a + d.hrz) % d.hrz; // a ring in the horizontal coordinate
        for (int y = y0; y <= y1; ++y) lower(x * d.vtc + y, dis);
    }
}

// idx2Pt from the tables, as the floats of the published cloud
LS_HD void bin_point(const Derived& d, const double* tables, int x, int y, double dis, float* out)
{
    const double pz = tables[2 * d.hrz + d.vtc + y] * dis;
    const double q = tables[2 * d.hrz + y] * dis;
    out[0] = (float)(tables[x] * q);
    out[1] = (float)(tables[d.hrz + x] * q);
    out[2] = (float)pz;
}
// the published float point in the world frame
LS_HD void world_point(const Pose& o, const float* lp, float* out)
{
    const double fx = (double)lp[0], fy = (double)lp[1];
    out[0] = (float)((o.x + o.c * fx) - o.s * fy);
    out[1] = (float)((o.y + o.s * fx) + o.c * fy);
    out[2] = lp[2];
}
// perspectivePoints for one point in range: rot^T d as floats
LS_HD void perspective_point(const Pose& o, const Seen& v, float* out)
{
    out[0] = (float)laser_x(o, v);
    out[1] = (float)laser_y(o, v);
    out[2] = (float)v.dz;
}
LS_HD void nan_point(float* out) { out[0] = out[1] = out[2] = NAN; }

// ---- one scan, serially ---------------------------------------------------------------------------------------------------------
// cloud [n][3]; tables from make_tables.  Range mode: image [hrz * vtc], laser / world / compact [hrz * vtc][3], index [hrz * vtc].
// Perspective mode: laser / world [capacity][3], index [capacity]; image and compact are not touched.  Returns the status
inline int scan_one(const Derived& d, const double* tables, const float* cloud, int n, double x, double y, double yaw, int capacity,
                    double* image, float* laser_pts, float* world_pts, int* index, float* compact, int* count)
{
    const Pose o = make_pose(x, y, yaw);
    const int bins = d.hrz * d.vtc, slots = d.perspective ? capacity : bins;
    *count = 0;
    if (!d.perspective)
        for (int b = 0; b < bins; ++b) image[b] = EMPTY;
    if (!o.ok || d.perspective) {
        for (int k = 0; k < slots; ++k) {
            nan_point(laser_pts + 3 * k);
            nan_point(world_pts + 3 * k);
            index[k] = -1;
            if (!d.perspective) nan_point(compact + 3 * k);
        }
        if (!o.ok) return E_POSE;
    }
    if (d.perspective) {
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const float* p = cloud + 3 * (size_t)i;
            const Seen v = see(d, o, p[0], p[1], p[2]);
            if (!v.in_range) continue;
            if (m < capacity) {
                perspective_point(o, v, laser_pts + 3 * (size_t)m);
                for (int k = 0; k < 3; ++k) world_pts[3 * (size_t)m + k] = p[k];
                index[m] = i;
            }
            ++m;
        }
        *count = m;
        return m > capacity ? E_CAPACITY : OK;
    }
    for (int i = 0; i < n; ++i) {
        const float* p = cloud + 3 * (size_t)i;
        const Seen v = see(d, o, p[0], p[1], p[2]);
        if (!v.in_range) continue;
        range_point(d, o, v, tables + 2 * d.hrz, [&](int b, double dis) { if (dis < image[b]) image[b] = dis; });
    }
    int m = 0;
    for (int b = 0; b < bins; ++b) {
        const bool hit = image[b] < EMPTY;
        if (hit) {
            bin_point(d, tables, b / d.vtc, b % d.vtc, image[b], laser_pts + 3 * (size_t)b);
            world_point(o, laser_pts + 3 * (size_t)b, world_pts + 3 * (size_t)b);
            for (int k = 0; k < 3; ++k) compact[3 * (size_t)m + k] = laser_pts[3 * (size_t)b + k];
            index[m++] = b;
        } else {
            nan_point(laser_pts + 3 * (size_t)b);
            nan_point(world_pts + 3 * (size_t)b);
        }
    }
    for (int k = m; k < bins; ++k) {
        nan_point(compact + 3 * (size_t)k);
        index[k] = -1;
    }
    *count = m;
    return OK;
}

} // namespace laser

#endif
