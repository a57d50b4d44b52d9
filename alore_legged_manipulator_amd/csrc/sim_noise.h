// sim_noise.h -- the simulator's Gaussian noise as counter-based draws, the arithmetic once (internal).
// Plain C++17: __host__ __device__ under hipcc, no HIP dependency otherwise.  ltv_plant::step_noisy (ltv_plant.h) and
// ltv::plant_ekf_kernel (ltv_ekf_loop.hip) draw from it; tests/harness/sim_noise_check.cpp runs it on the CPU; the oracle is
// tests/sim_noise_cases.py.
//
// The reference seeds a std::mt19937 from std::random_device in every PoseSubCallback (simulator.h:222-229): no run of it can be
// repeated.  Here a draw is a pure function of (seed, robot, event, stream): what a robot sees does not depend on the size of the
// fleet, on how a run is cut into calls or on which route enqueued it.
//   generator  Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85
//   counter    (event low word, event high word, robot, stream);   key (seed low word, seed high word)
//   streams    0: the velocity noise of a PoseSub;  1, 2: the measurement noise of a pose update ((x, y) from 1, theta from 2)
//   uniforms   the output words in pairs (0, 1) and (2, 3):  u = ((w_a >> 6) 2^26 + (w_b >> 6) + 0.5) 2^-52
//              52 bits and the half: every term and the sum are exact doubles, u lies in [2^-53, 1 - 2^-53], never 0 and never 1.
//              (With 53 bits -- w_a >> 5 -- the half does not fit the significand any more and all-one words round to u = 1.)
//   normals    Box-Muller: r = sqrt(-2 ln u1), z0 = r cos(2 pi u2), z1 = r sin(2 pi u2); cos and sin evaluated ONCE (sincos on the
//              device, libm on the host: with log and sqrt the only place where the two differ).  |z| <= sqrt(106 ln 2) < 8.58.
#ifndef ALORE_SIM_NOISE_H
#define ALORE_SIM_NOISE_H

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SN_HD __host__ __device__ inline
#else
#define SN_HD inline
#endif

namespace sim_noise {

constexpr int STREAM_VEL = 0, STREAM_MEAS_XY = 1, STREAM_MEAS_TH = 2;
constexpr double TWO_PI = 6.28318530717958647692;

// Philox4x32-10: ctr[4], key[2] in, out[4]
SN_HD void philox4x32(const uint32_t* ctr, const uint32_t* key, uint32_t* out)
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four words of (seed, robot, event, stream)
SN_HD void words(uint64_t seed, uint32_t robot, uint64_t event, uint32_t stream, uint32_t* out)
{
    const uint32_t ctr[4] = {(uint32_t)event, (uint32_t)(event >> 32), robot, stream};
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    philox4x32(ctr, key, out);
}

SN_HD double uniform(uint32_t wa, uint32_t wb)
{
    return ((double)(wa >> 6) * 67108864.0 + (double)(wb >> 6) + 0.5) * 2.220446049250313e-16; // 2^26, 2^-52
}

SN_HD void box_muller(double u1, double u2, double& z0, double& z1)
{
    const double r = std::sqrt(-2.0 * std::log(u1)), a = TWO_PI * u2;
    double sn, cs;
#if defined(__HIP_DEVICE_COMPILE__)
    sincos(a, &sn, &cs);
#else
    sn = std::sin(a);
    cs = std::cos(a);
#endif
    z0 = r * cs;
    z1 = r * sn;
}

// two independent standard normals of (seed, robot, event, stream)
SN_HD void normal2(uint64_t seed, uint32_t robot, uint64_t event, uint32_t stream, double& z0, double& z1)
{
    uint32_t w[4];
    words(seed, robot, event, stream, w);
    box_muller(uniform(w[0], w[1]), uniform(w[2], w[3]), z0, z1);
}

} // namespace sim_noise
#endif
