// frp_disturbance.hpp -- frp_nmpc.h section (15): the force of ONE sample of ONE vehicle, the device function that both
// frp_disturbance.hip's eval kernel and frp_vehicle.hip's field step call (both units are built with -ffp-contract=off, so the fused and
// the stand-alone evaluation round alike).  tests/disturbance_oracle.py is the statement: every product and sum below is written in its
// order and rounded on its own.
//   * Zone rows are the same for every lane of a wave: they are read at a wave-uniform index through a pointer to the constant address
//     space (uniform_row below), so the compiler fetches them with scalar loads into SGPRs and they cost no vector register
//     (profiles/disturbance_step_identity.txt counts the loads of the field step).
//   * Event rows are the vehicle's own: vector loads, 40 bytes per slot.
//   * The generator is integer arithmetic (three mixes shared by the axes, two per axis), then one logarithm, one square root and one
//     cosine per axis: ocml's log and cos, within an ulp or so of libm's -- the one place where the device and the oracle differ.
//   * Nothing here stores to memory: the callers own gust and tick.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/frp_nmpc.h"
#include "frp_fleet.hpp"

#pragma clang fp contract(off)

namespace frp {
namespace disturbance {

using namespace fleet;

constexpr int ZONE = FRP_DISTURBANCE_ZONE_STRIDE, EVENT = FRP_DISTURBANCE_EVENT_STRIDE;

// the SplitMix64 finaliser (distributed._splitmix64's constants)
__device__ inline unsigned long long mix(unsigned long long x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

// h of (seed, id, k): shared by the three axes of a sample
__device__ inline unsigned long long stream_key(unsigned long long seed, unsigned long long id, unsigned long long k)
{
    return mix(mix(mix(seed) + id) + k);
}

__device__ inline double normal(unsigned long long h, int axis)
{
    const unsigned long long r0 = mix(h + 2ULL * (unsigned long long)axis), r1 = mix(h + 2ULL * (unsigned long long)axis + 1ULL);
    const double u1 = (double)((r0 >> 11) + 1ULL) / 9007199254740993.0; // (the double this literal denotes is 2^53: (0, 1])
    const double u2 = (double)(r1 >> 11) / 9007199254740992.0;          // [0, 1)
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// A zone row as the scalar unit reads it: the table is written by nobody while a kernel runs (the header's contract), and the constant
// address space says so -- from a plain const __restrict__ pointer the compiler issues vector loads with a scalar base, because the
// kernels that call this also store to memory; through this type a wave-uniform index gives s_load_dwordx4 / x8 into SGPRs.
typedef const double __attribute__((address_space(4))) *uniform_row;

// w_z(p, t) of one zone row
__device__ inline double zone_weight(uniform_row row, const double p[3], double t)
{
    if (!(row[10] <= t && t < row[11])) return 0.0;
    double d[6];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        d[i] = p[i] - row[i];
        d[3 + i] = row[3 + i] - p[i];
    }
    bool in = true;
#pragma unroll
    for (int i = 0; i < 6; i++) in = in && d[i] >= 0.0;
    if (!in) return 0.0;
    double m = d[0];
#pragma unroll
    for (int i = 1; i < 6; i++) m = d[i] < m ? d[i] : m;
    const double ramp = row[9];
    return m >= ramp ? 1.0 : m / ramp;
}

// The force of sample k of vehicle b at position p.  base: the constant part; g: the OU state, read and written when d.gust is set
// (the caller loads it from d.gust and stores it where it advances).  f <- the force.
__device__ inline void sample_force(const frp_nmpc_disturbance &d, const double *__restrict__ zone, const double *__restrict__ event, int b,
                                    long long k, const double p[3], const double base[3], double g[3], double f[3])
{
    const double t = d.t_epoch + (double)k * d.dt;
    double acc[3] = {base[0], base[1], base[2]};
    for (int z = 0; z < d.Z; z++) {
        const uniform_row row = (uniform_row)(zone + (size_t)z * ZONE);
        const double w = zone_weight(row, p, t);
#pragma unroll
        for (int i = 0; i < 3; i++) acc[i] = acc[i] + w * row[6 + i];
    }
    for (int e = 0; e < d.E; e++) {
        const double *row = event + ((size_t)b * d.E + e) * EVENT;
        if (row[0] <= t && t < row[1]) {
#pragma unroll
            for (int i = 0; i < 3; i++) acc[i] = acc[i] + row[2 + i];
        }
    }
    if (d.gust) {
        const unsigned long long h = stream_key((unsigned long long)d.seed, (unsigned long long)d.id0 + (unsigned long long)(long long)b, (unsigned long long)k);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            g[i] = d.gust_a[i] * g[i] + d.gust_c[i] * normal(h, i);
            acc[i] = acc[i] + g[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 3; i++) f[i] = acc[i];
}

// the argument rules of a frp_nmpc_disturbance (host)
inline int check(const frp_nmpc_disturbance *d)
{
    if (!d || d->B < 1 || d->Z < 0 || d->Z > FRP_DISTURBANCE_MAX_ZONES || d->E < 0 || d->E > FRP_DISTURBANCE_MAX_EVENTS) return FRP_ERR_ARG;
    if ((d->zone == nullptr) != (d->Z == 0) || (d->event == nullptr) != (d->E == 0) || !d->tick) return FRP_ERR_ARG;
    if (!finite_d(d->t_epoch) || !positive(d->dt)) return FRP_ERR_ARG;
    if (d->gust) {
        for (int i = 0; i < 3; i++)
            if (!(d->gust_a[i] >= 0.0 && d->gust_a[i] <= 1.0) || !non_negative(d->gust_c[i])) return FRP_ERR_ARG;
    }
    return FRP_OK;
}

} // namespace disturbance
} // namespace frp
