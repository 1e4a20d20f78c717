// frp_disturbance.hip -- frp_nmpc.h section (15): the stand-alone evaluation of the disturbance model and its reset (the fused evaluation
// is frp_vehicle.hip's field step; the model itself is frp_disturbance.hpp's sample_force, called by both).
//
//   * One thread per vehicle, 256 per workgroup, no LDS, no barrier, no atomics: a vehicle reads and writes its own rows alone.  Per
//     sample a thread reads 24 bytes of position and writes 24 bytes of force; the zone table comes through the scalar path.
//   * No contraction in this file (the build passes -ffp-contract=off as well): t = t_epoch + k * dt, acc + w * F and a * g + c * n are a
//     product and a sum each, as tests/disturbance_oracle.py writes them.
//   * Every index is b < B and s < S as the entry point checked them (B * S fits an int; offsets are formed in size_t).
//   * Every store is a plain C++ store from a vector lane; no inline assembly.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/frp_nmpc.h"
#include "frp_disturbance.hpp"

#pragma clang fp contract(off)

namespace frp {
namespace disturbance {

__global__ __launch_bounds__(THREADS) void eval_kernel(frp_nmpc_disturbance d, int S, const double *pos, const double *base, int advance, double *force)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= d.B) return;
    const long long k0 = d.tick[b];
    double g[3] = {0.0, 0.0, 0.0}, f0[3] = {0.0, 0.0, 0.0};
    if (d.gust) {
#pragma unroll
        for (int i = 0; i < 3; i++) g[i] = d.gust[(size_t)b * 3 + i];
    }
    if (base) {
#pragma unroll
        for (int i = 0; i < 3; i++) f0[i] = base[(size_t)b * 3 + i];
    }
    for (int s = 0; s < S; s++) {
        const double *ps = pos + ((size_t)b * S + s) * 3;
        const double p[3] = {ps[0], ps[1], ps[2]};
        double f[3];
        sample_force(d, d.zone, d.event, b, (long long)((unsigned long long)k0 + (unsigned long long)s), p, f0, g, f);
        double *fo = force + ((size_t)b * S + s) * 3;
        fo[0] = f[0]; fo[1] = f[1]; fo[2] = f[2];
    }
    if (advance) {
        if (d.gust) {
#pragma unroll
            for (int i = 0; i < 3; i++) d.gust[(size_t)b * 3 + i] = g[i];
        }
        d.tick[b] = (long long)((unsigned long long)k0 + (unsigned long long)S);
    }
}

__global__ __launch_bounds__(THREADS) void reset_kernel(int B, const int *mask, double *gust, long long *tick)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= B) return;
    if (mask && mask[b] == 0) return;
    tick[b] = 0;
    if (gust) {
        gust[(size_t)b * 3 + 0] = 0.0; gust[(size_t)b * 3 + 1] = 0.0; gust[(size_t)b * 3 + 2] = 0.0;
    }
}

} // namespace disturbance
} // namespace frp

extern "C" {

int frp_nmpc_disturbance_eval(const frp_nmpc_disturbance *d, int S, const double *pos, const double *base, int advance, double *force, void *stream)
{
    using namespace frp::disturbance;
    if (check(d) != FRP_OK || S < 1 || (long long)d->B * S > 0x7fffffffLL || !pos || !force) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(eval_kernel, blocks_for(d->B), stream, *d, S, pos, base, advance, force);
}

int frp_nmpc_disturbance_reset(const frp_nmpc_disturbance *d, const int *mask, void *stream)
{
    using namespace frp::disturbance;
    if (check(d) != FRP_OK) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(reset_kernel, blocks_for(d->B), stream, d->B, mask, d->gust, d->tick);
}

} // extern "C"
