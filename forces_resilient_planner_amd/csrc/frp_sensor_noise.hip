// frp_sensor_noise.hip -- frp_nmpc.h section (16): seeded measurement errors of the states, of depth images and of float64 point scans.
// tests/sensor_noise_oracle.py is the statement: every product and sum below is written in its order and rounded on its own.
//
//   * The generator is frp_disturbance.hpp's as it is (mix, stream_key, normal); a sample's key is mix(stream_key(...) + tag), so no
//     channel shares a 64-bit word with the gusts or with another channel.
//   * states_kernel: one thread per vehicle, the samples in order, twelve normals per sample; a vehicle reads and writes its own rows,
//     bias and tick alone, so it advances them itself.
//   * depth_kernel (the unit's hot path: F * rows * cols threads): grid (ceil(rows * cols / 256), F), one thread per pixel, lane l of a
//     wave takes pixel base + l -- a wave reads 128 consecutive bytes and writes 128.  No LDS, no barrier, no atomics.  Per pixel with a
//     return: three mixes for the key and the uniform, two for the normal, one FP64 division, one log, one sqrt, one cos.
//   * scan_kernel: grid (ceil(P / 256), S), one thread per point, 24 bytes in and out at a stride of 24 bytes across the lanes.
//   * The frame counters are read by every thread of a frame: tick_kernel advances them in a launch of its own, stream-ordered after the
//     first -- no kernel waits on another workgroup.
//   * Every index is checked against the sizes the entry point checked (b < B, pixel < rows * cols, point < count <= P); offsets are
//     formed in size_t.  Every store is a plain C++ store from a vector lane; no inline assembly.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/frp_nmpc.h"
#include "frp_disturbance.hpp"

#pragma clang fp contract(off)

namespace frp {
namespace sensor_noise {

using namespace fleet;
using disturbance::mix;
using disturbance::normal;
using disturbance::stream_key;

// h_sample of (seed, id0 + i, k) for a channel's tag
__device__ inline unsigned long long sample_key(const frp_nmpc_sensor_noise &n, long long i, long long k, unsigned long long tag)
{
    return mix(stream_key((unsigned long long)n.seed, (unsigned long long)n.id0 + (unsigned long long)i, (unsigned long long)k) + tag);
}

// u(h, j) in [0, 1): the quotient is exact
__device__ inline double uniform(unsigned long long h, int j) { return (double)(mix(h + (unsigned long long)j) >> 11) / 9007199254740992.0; }

// x + e, but a zero term is not added: x keeps its bits
__device__ inline double add_term(double x, double e) { return e == 0.0 ? x : x + e; }

__global__ __launch_bounds__(THREADS) void states_kernel(frp_nmpc_sensor_noise n, int S, const double *x_true, double *x_meas, double *y, int advance)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= n.B) return;
    const long long k0 = n.tick[b];
    double bias[3], m[9];
#pragma unroll
    for (int i = 0; i < 3; i++) bias[i] = n.bias[(size_t)b * 3 + i];
    for (int s = 0; s < S; s++) {
        const double *xs = x_true + ((size_t)b * S + s) * 9;
        double x[9];
#pragma unroll
        for (int j = 0; j < 9; j++) x[j] = xs[j];
        const unsigned long long h = sample_key(n, b, (long long)((unsigned long long)k0 + (unsigned long long)s), FRP_SENSOR_NOISE_TAG_STATE);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            if (finite_d(x[i])) {
                bias[i] = n.bias_a[i] * bias[i] + n.bias_c[i] * normal(h, i);
                m[i] = add_term(add_term(x[i], bias[i]), n.sigma_p[i] * normal(h, 3 + i));
            } else {
                m[i] = x[i];
            }
            m[3 + i] = finite_d(x[3 + i]) ? add_term(x[3 + i], n.sigma_v[i] * normal(h, 6 + i)) : x[3 + i];
            m[6 + i] = finite_d(x[6 + i]) ? add_term(x[6 + i], n.sigma_a[i] * normal(h, 9 + i)) : x[6 + i];
        }
        double *ms = x_meas + ((size_t)b * S + s) * 9;
#pragma unroll
        for (int j = 0; j < 9; j++) ms[j] = m[j];
    }
    if (y) {
#pragma unroll
        for (int j = 0; j < 9; j++) y[(size_t)b * 9 + j] = m[j];
    }
    if (advance) {
#pragma unroll
        for (int i = 0; i < 3; i++) n.bias[(size_t)b * 3 + i] = bias[i];
        n.tick[b] = (long long)((unsigned long long)k0 + (unsigned long long)S);
    }
}

__global__ __launch_bounds__(THREADS) void reset_kernel(int B, const int *mask, const double *x, double *y, double *bias, long long *tick)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= B) return;
    if (mask && mask[b] == 0) return;
    tick[b] = 0;
    bias[(size_t)b * 3 + 0] = 0.0; bias[(size_t)b * 3 + 1] = 0.0; bias[(size_t)b * 3 + 2] = 0.0;
    if (y) {
#pragma unroll
        for (int j = 0; j < 9; j++) y[(size_t)b * 9 + j] = x[(size_t)b * 9 + j];
    }
}

__global__ __launch_bounds__(THREADS) void depth_kernel(frp_nmpc_sensor_noise n, int npix, const unsigned short *in, unsigned short *out, const int *active,
                                                        const long long *frame_tick)
{
    const int f = blockIdx.y;
    const unsigned idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= (unsigned)npix) return;
    if (active && active[f] == 0) return;
    const size_t at = (size_t)f * (size_t)npix + idx;
    const unsigned short pix = in[at];
    unsigned short res = 0;
    if (pix != 0) {
        const unsigned long long h = mix(sample_key(n, f, frame_tick[f], FRP_SENSOR_NOISE_TAG_DEPTH) + (unsigned long long)idx);
        if (!(uniform(h, 2) < n.depth_p_drop)) {
            const double z = (double)pix / n.depth_scale;
            const double sigma = n.depth_sigma0 + (n.depth_sigma2 * z) * z;
            const double v = (double)pix + (n.depth_scale * sigma) * normal(h, 0);
            const double w = floor(v + 0.5);
            if (w >= 1.0 && w <= 65535.0) res = (unsigned short)w;
        }
    }
    out[at] = res;
}

__global__ __launch_bounds__(THREADS) void scan_kernel(frp_nmpc_sensor_noise n, int P, const double *in, double *out, const double *origin, const int *count,
                                                       const int *active, const long long *frame_tick)
{
    const int s = blockIdx.y;
    const unsigned idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= (unsigned)P) return;
    if (active && active[s] == 0) return;
    if (count && (count[s] < 0 || idx >= (unsigned)count[s])) return;
    const size_t at = ((size_t)s * (size_t)P + idx) * 3;
    const double p[3] = {in[at], in[at + 1], in[at + 2]};
    double q[3] = {p[0], p[1], p[2]};
    if (finite_d(p[0]) && finite_d(p[1]) && finite_d(p[2])) {
        const double o[3] = {origin[(size_t)s * 3], origin[(size_t)s * 3 + 1], origin[(size_t)s * 3 + 2]};
        const double d[3] = {p[0] - o[0], p[1] - o[1], p[2] - o[2]};
        const double r = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        if (positive(r)) {
            const unsigned long long h = mix(sample_key(n, s, frame_tick[s], FRP_SENSOR_NOISE_TAG_SCAN) + (unsigned long long)idx);
            if (uniform(h, 2) < n.scan_p_drop) {
                q[0] = q[1] = q[2] = __builtin_nan("");
            } else {
                const double e = (n.scan_sigma0 + n.scan_sigma1 * r) * normal(h, 0);
                if (e != 0.0) {
                    const double g = 1.0 + e / r;
#pragma unroll
                    for (int i = 0; i < 3; i++) q[i] = o[i] + d[i] * g;
                }
            }
        }
    }
    out[at] = q[0]; out[at + 1] = q[1]; out[at + 2] = q[2];
}

// frame_tick[f] += 1 for the active frames: launched after the kernel whose threads read the counters
__global__ __launch_bounds__(THREADS) void tick_kernel(int F, const int *active, long long *frame_tick)
{
    const int f = blockIdx.x * THREADS + threadIdx.x;
    if (f >= F) return;
    if (active && active[f] == 0) return;
    frame_tick[f] = (long long)((unsigned long long)frame_tick[f] + 1ULL);
}

// the argument rules of a frp_nmpc_sensor_noise (host)
inline int check(const frp_nmpc_sensor_noise *n)
{
    if (!n || n->B < 1) return FRP_ERR_ARG;
    for (int i = 0; i < 3; i++) {
        if (!non_negative(n->sigma_p[i]) || !non_negative(n->sigma_v[i]) || !non_negative(n->sigma_a[i])) return FRP_ERR_ARG;
        if (!(n->bias_a[i] >= 0.0 && n->bias_a[i] <= 1.0) || !non_negative(n->bias_c[i])) return FRP_ERR_ARG;
    }
    if (!positive(n->depth_scale) || !non_negative(n->depth_sigma0) || !non_negative(n->depth_sigma2) || !non_negative(n->scan_sigma0) || !non_negative(n->scan_sigma1))
        return FRP_ERR_ARG;
    if (!(n->depth_p_drop >= 0.0 && n->depth_p_drop <= 1.0) || !(n->scan_p_drop >= 0.0 && n->scan_p_drop <= 1.0)) return FRP_ERR_ARG;
    return FRP_OK;
}

// `kernel` on a (blocks, frames) grid of THREADS, then the counters' launch
template <typename... P, typename... A>
inline int launch_frames(void (*kernel)(P...), unsigned blocks, int frames, const int *active, long long *frame_tick, void *stream, const A &...args)
{
    hipLaunchKernelGGL(kernel, dim3(blocks, (unsigned)frames), dim3(THREADS), 0, static_cast<hipStream_t>(stream), args...);
    if (hipGetLastError() != hipSuccess) return FRP_ERR_HIP;
    return launch(tick_kernel, blocks_for(frames), stream, frames, active, frame_tick);
}

} // namespace sensor_noise
} // namespace frp

extern "C" {

int frp_nmpc_sensor_noise_states(const frp_nmpc_sensor_noise *n, int S, const double *x_true, double *x_meas, double *y, int advance, void *stream)
{
    using namespace frp::sensor_noise;
    if (check(n) != FRP_OK || !n->bias || !n->tick || S < 1 || (long long)n->B * S > 0x7fffffffLL || !x_true || !x_meas) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(states_kernel, blocks_for(n->B), stream, *n, S, x_true, x_meas, y, advance);
}

int frp_nmpc_sensor_noise_reset(const frp_nmpc_sensor_noise *n, const int *mask, const double *x, double *y, void *stream)
{
    using namespace frp::sensor_noise;
    if (check(n) != FRP_OK || !n->bias || !n->tick || (x == nullptr) != (y == nullptr)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch(reset_kernel, blocks_for(n->B), stream, n->B, mask, x, y, n->bias, n->tick);
}

int frp_nmpc_sensor_noise_depth(const frp_nmpc_sensor_noise *n, int F, int rows, int cols, const unsigned short *in, unsigned short *out, const int *active,
                                long long *frame_tick, void *stream)
{
    using namespace frp::sensor_noise;
    if (check(n) != FRP_OK || F < 1 || F > FRP_SENSOR_NOISE_MAX_FRAMES || rows < 1 || cols < 1 || (long long)rows * cols > 0x7fffffffLL || !in || !out || !frame_tick)
        return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    const int npix = rows * cols;
    return launch_frames(depth_kernel, blocks_for(npix), F, active, frame_tick, stream, *n, npix, in, out, active, (const long long *)frame_tick);
}

int frp_nmpc_sensor_noise_scan(const frp_nmpc_sensor_noise *n, int S, int P, const double *in, double *out, const double *origin, const int *count,
                               const int *active, long long *frame_tick, void *stream)
{
    using namespace frp::sensor_noise;
    if (check(n) != FRP_OK || S < 1 || S > FRP_SENSOR_NOISE_MAX_FRAMES || P < 1 || !in || !out || !origin || !frame_tick) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    return launch_frames(scan_kernel, blocks_for(P), S, active, frame_tick, stream, *n, P, in, out, origin, count, active, (const long long *)frame_tick);
}

} // extern "C"
