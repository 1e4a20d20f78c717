// frp_nmpc.h section (8), frp_nmpc_occmap_distance.h: the truncated squared distance field of the map's bit plane and the clearance
// queries on it.  No reference counterpart (occ_grid/src/occ_map.cpp keeps no distance); tests/occmap_distance_oracle.py is the
// executable statement, as brute force, and the field equals it to the bit.
//
//   * The squared Euclidean distance separates by axis: three passes, each f'(i) = min over k in [-R, R] of f(i + k) + k * k along
//     one axis, from f = 0 on occupied voxels and "none" elsewhere; with `border` an index outside the axis contributes k * k.  A true
//     nearest offset with D2 <= R * R has every component <= R, so windows of +-R lose nothing; every candidate a pass forms is the
//     squared distance to a real occupied (or outside) voxel or holds a term > R * R, so nothing below the truth is formed; values
//     above R * R survive between the passes and are cut once, at the end.  Integers throughout: "none" after the z pass is R + 1
//     (squared: > R * R), every sum stays <= (R + 1)^2 + R^2 <= 8321.
//   * z pass (dz_kernel), straight from the bit plane: one thread per voxel, z across the lanes, so a wavefront reads one or two
//     columns' words (broadcast loads) and stores 64 contiguous bytes.  The nearest set bit at or below / at or above z by count-
//     leading / count-trailing-zeros on the column's words, walking at most R / 32 + 2 words each way.  Bits at z >= gz of the last
//     word are masked (not trusted to be zero); the border is the two terms z + 1 and gz - z.  Output: uint8 min(dz, R + 1).
//   * y and x pass (axis_kernel, one template): the volume seen as [outer][axis][inner] -- [gx][gy][gz] for y, [1][gx][gy * gz] for
//     x -- with the inner index across the lanes, so that loads and stores are contiguous.  A workgroup stages TY + 2R rows of a tile
//     of TZ inner elements in LDS as uint16 (the z pass's bytes squared on the way in; rows outside the axis are 0 with `border`, none
//     without), then thread t takes the outputs e = t, t + 256, ... of the flattened [row][inner] tile: lanes read consecutive uint16
//     at e + j * width for j = 0 ... 2R -- no bank conflicts -- and add (j - R)^2.  TZ is the whole inner extent up to 128 elements,
//     else 64; TY fills 32 KB of LDS per workgroup (60 KB for R > 32, so that the 2R halo rows stay below the rows they serve), i.e.
//     two to five workgroups per CU of gfx950's 160 KB.  The x pass cuts at R * R and writes the field.
//   * Bytes per voxel: z pass 1/8 read + 1 written, y pass 1 read + 2 written, x pass 2 read + 2 written (+ 2R / TY halo re-reads, from
//     L2): about 8, what frp_nmpc_occmap_refresh streams (8 read, 1 written).
//   * Clearance: one thread per position / per vehicle, the index arithmetic of frp_occmap.hpp (floored, the tests on the double),
//     clear = res * sqrt((double)d2): a correctly rounded square root and one product; this file is compiled with -ffp-contract=off.
//   * Every index: voxel < gx * gy * gz < 2^30 (frp::occmap::valid), plane word < gx * gy * wz, LDS element < (TY + 2R) * TZ as sized by
//     the entry point; q < Q, b < B, s < S as checked there, offsets formed in size_t.  No atomics, no waiting between workgroups,
//     every store a plain C++ store from a vector lane.
#include "frp_occmap.hpp"

#include <climits>

#pragma clang fp contract(off)

namespace frp {
namespace occmap {

constexpr int DIST_THREADS = 256;
constexpr int DIST_FAR = FRP_OCCMAP_DIST_FAR;
constexpr int DIST_TZ_WHOLE = 128;        // an inner extent up to this is one tile
constexpr int DIST_TZ = 64;               // else tiles of one wavefront's width
constexpr size_t DIST_LDS = 32768;        // LDS per workgroup for R <= 32 ...
constexpr size_t DIST_LDS_WIDE = 61440;   // ... and beyond (below the 64 KB a launch gets without an attribute)

// min(dz, R + 1) per voxel from the bit plane; border: z = -1 and z = gz are occupied
__global__ __launch_bounds__(DIST_THREADS) void dz_kernel(int n, int gz, int wz, int R, int border, const uint32_t *plane, uint8_t *dz)
{
    const uint32_t last = (gz & 31) ? (1u << (gz & 31)) - 1u : 0xffffffffu; // the voxels of a column's last word
    for (size_t i = (size_t)blockIdx.x * DIST_THREADS + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * DIST_THREADS) {
        const int col = (int)((unsigned)i / (unsigned)gz), z = (int)i - col * gz; // (n < 2^30)
        const uint32_t *cw = plane + (size_t)col * wz;
        const int w = z >> 5, b = z & 31;
        int best = R + 1;
        for (int ww = w; ww >= 0 && z - (32 * ww + 31) <= R; ww--) { // the nearest set bit at or below z
            uint32_t m = cw[ww] & (ww == wz - 1 ? last : 0xffffffffu);
            if (ww == w) m &= 0xffffffffu >> (31 - b);
            if (m) {
                const int d = z - (32 * ww + 31 - __builtin_clz(m));
                best = d < best ? d : best;
                break;
            }
        }
        for (int ww = w; ww < wz && 32 * ww - z <= R; ww++) { // ... and at or above
            uint32_t m = cw[ww] & (ww == wz - 1 ? last : 0xffffffffu);
            if (ww == w) m &= 0xffffffffu << b;
            if (m) {
                const int d = 32 * ww + __builtin_ctz(m) - z;
                best = d < best ? d : best;
                break;
            }
        }
        if (border) {
            const int lo = z + 1, hi = gz - z;
            best = lo < best ? lo : best;
            best = hi < best ? hi : best;
        }
        dz[i] = (uint8_t)best;
    }
}

struct Pass {
    int O, A, I;      // the volume as [O][A][I]; the pass runs along A
    int TY, TZ;       // outputs per workgroup along A, tile width along I
    int nty, ntz;     // tiles per axis
    int R, border;
    int cut;          // the last pass: values above R * R become FAR
};

// In = uint8_t: the z pass's distances, squared on the way in; In = uint16_t: squared distances
template <typename In>
__global__ __launch_bounds__(DIST_THREADS) void axis_kernel(Pass p, const In *in, uint16_t *out)
{
    extern __shared__ uint16_t s_f[]; // [ny + 2R][nz]
    const unsigned bid = blockIdx.x;
    const int tz = (int)(bid % (unsigned)p.ntz);
    const unsigned rest = bid / (unsigned)p.ntz;
    const int ty = (int)(rest % (unsigned)p.nty), o = (int)(rest / (unsigned)p.nty);
    const int R = p.R, y0 = ty * p.TY, z0 = tz * p.TZ;
    const int ny = p.A - y0 < p.TY ? p.A - y0 : p.TY, nz = p.I - z0 < p.TZ ? p.I - z0 : p.TZ;
    const size_t base = (size_t)o * p.A * p.I + z0;
    const int loads = (ny + 2 * R) * nz;
    for (int e = threadIdx.x; e < loads; e += DIST_THREADS) {
        const int row = e / nz, zl = e - row * nz, y = y0 - R + row;
        unsigned v;
        if (y < 0 || y >= p.A) {
            v = p.border ? 0u : (unsigned)DIST_FAR;
        } else {
            v = in[base + (size_t)y * p.I + zl];
            if (sizeof(In) == 1) v *= v;
        }
        s_f[e] = (uint16_t)v;
    }
    __syncthreads();
    const int outs = ny * nz, r2 = R * R;
    for (int e = threadIdx.x; e < outs; e += DIST_THREADS) {
        int m = INT_MAX;
        for (int j = 0; j <= 2 * R; j++) {
            const int k = j - R, v = (int)s_f[e + j * nz] + k * k;
            m = v < m ? v : m;
        }
        const int row = e / nz, zl = e - row * nz;
        if (p.cut) m = m <= r2 ? m : DIST_FAR;
        out[base + (size_t)(y0 + row) * p.I + zl] = (uint16_t)m; // (k = 0 is a row of the axis: m <= (R + 1)^2 without the cut)
    }
}

// the tiling of a pass along A of [O][A][I]; returns the LDS bytes of a workgroup
static size_t plan_pass(Pass *p, int O, int A, int I, int R, int border, int cut)
{
    p->O = O; p->A = A; p->I = I; p->R = R; p->border = border ? 1 : 0; p->cut = cut;
    p->TZ = I <= DIST_TZ_WHOLE ? I : DIST_TZ;
    p->ntz = (I + p->TZ - 1) / p->TZ;
    const int rows = (int)((R <= 32 ? DIST_LDS : DIST_LDS_WIDE) / (sizeof(uint16_t) * (size_t)p->TZ)); // >= 128 (240): more than 2R
    const int ty_max = rows - 2 * R;
    p->nty = (A + ty_max - 1) / ty_max;
    p->TY = (A + p->nty - 1) / p->nty; // the tiles of an axis alike
    return (size_t)(p->TY + 2 * R) * p->TZ * sizeof(uint16_t);
}

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

static size_t voxels(const frp_nmpc_occmap *m) { return (size_t)m->grid[0] * m->grid[1] * m->grid[2]; }

static bool radius_ok(int R) { return R >= 1 && R <= FRP_OCCMAP_DIST_MAX_R; }

struct Point {
    double clear;
    int d2;
};

// the clearance rule of the header for one position
__device__ inline Point clearance_of(const Geo &g, const uint16_t *field, double px, double py, double pz)
{
    const double f[3] = {floored(px, g.origin[0], g.res_inv), floored(py, g.origin[1], g.res_inv), floored(pz, g.origin[2], g.res_inv)};
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; a++) in = in && f[a] >= 0.0 && f[a] <= (double)(g.grid[a] - 1); // isInMap on the double: a NaN and an infinity fail
    Point r;
    r.clear = 0.0; r.d2 = -1;
    if (!in) return r;
    const int x = clamp_id(f[0]), y = clamp_id(f[1]), z = clamp_id(f[2]);
    r.d2 = field[((size_t)x * g.grid[1] + y) * g.grid[2] + z];
    r.clear = r.d2 == DIST_FAR ? HUGE_VAL : g.res * sqrt((double)r.d2);
    return r;
}

__global__ __launch_bounds__(DIST_THREADS) void clearance_kernel(Geo g, const uint16_t *field, int Q, const double *pos, double *clear, int *d2)
{
    const size_t q = (size_t)blockIdx.x * DIST_THREADS + threadIdx.x;
    if (q >= (size_t)Q) return;
    const Point r = clearance_of(g, field, pos[3 * q], pos[3 * q + 1], pos[3 * q + 2]);
    clear[q] = r.clear;
    if (d2) d2[q] = r.d2;
}

__global__ __launch_bounds__(DIST_THREADS) void trace_kernel(Geo g, const uint16_t *field, int B, int S, int stride, const double *pos, const int *active,
                                                             double *min_clear, int *hits, int *samples)
{
    const size_t b = (size_t)blockIdx.x * DIST_THREADS + threadIdx.x;
    if (b >= (size_t)B) return;
    if (active && active[b] == 0) return;
    double mn = min_clear[b];
    int h = hits[b];
    const double *p = pos + b * (size_t)S * stride;
    for (int s = 0; s < S; s++, p += stride) {
        const Point r = clearance_of(g, field, p[0], p[1], p[2]); // (never a NaN: a position that is not finite is 0.0)
        if (r.clear < mn) mn = r.clear;
        if (r.clear == 0.0) h++;
    }
    min_clear[b] = mn;
    hits[b] = h;
    samples[b] += S;
}

__global__ __launch_bounds__(DIST_THREADS) void clearance_reset_kernel(int B, const int *mask, double *min_clear, int *hits, int *samples)
{
    const size_t b = (size_t)blockIdx.x * DIST_THREADS + threadIdx.x;
    if (b >= (size_t)B) return;
    if (mask && mask[b] == 0) return;
    min_clear[b] = HUGE_VAL;
    hits[b] = 0;
    samples[b] = 0;
}

} // namespace occmap
} // namespace frp

extern "C" {

size_t frp_nmpc_occmap_distance_scratch_bytes(const frp_nmpc_occmap *m, int R)
{
    using namespace frp::occmap;
    if (!valid(m) || !radius_ok(R)) return 0;
    return align256(voxels(m)) + voxels(m) * sizeof(uint16_t);
}

int frp_nmpc_occmap_distance_update(const frp_nmpc_occmap *m, int R, int border, uint16_t *field, void *scratch, size_t scratch_bytes,
                                    void *map_workspace, size_t map_workspace_bytes, void *stream)
{
    using namespace frp::occmap;
    if (!args_ok(m, map_workspace, map_workspace_bytes) || !radius_ok(R) || !field || !scratch) return FRP_ERR_ARG;
    if (scratch_bytes < frp_nmpc_occmap_distance_scratch_bytes(m, R)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = voxels(m);
    const int gx = m->grid[0], gy = m->grid[1], gz = m->grid[2];
    uint8_t *dz = static_cast<uint8_t *>(scratch);
    uint16_t *dyz = reinterpret_cast<uint16_t *>(dz + align256(n));
    hipLaunchKernelGGL(dz_kernel, dim3(blocks_for(n, 65536)), dim3(DIST_THREADS), 0, st, (int)n, gz, (gz + 31) / 32, R, border ? 1 : 0,
                       static_cast<const uint32_t *>(map_workspace), dz);
    Pass py, px;
    const size_t lds_y = plan_pass(&py, gx, gy, gz, R, border, 0);
    const size_t lds_x = plan_pass(&px, 1, gx, gy * gz, R, border, 1);
    hipLaunchKernelGGL(axis_kernel<uint8_t>, dim3((unsigned)((size_t)py.O * py.nty * py.ntz)), dim3(DIST_THREADS), lds_y, st, py, dz, dyz);
    hipLaunchKernelGGL(axis_kernel<uint16_t>, dim3((unsigned)((size_t)px.O * px.nty * px.ntz)), dim3(DIST_THREADS), lds_x, st, px, dyz, field);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

int frp_nmpc_occmap_clearance(const frp_nmpc_occmap *m, const uint16_t *field, int R, int Q, const double *pos, double *clear, int *d2, void *stream)
{
    using namespace frp::occmap;
    if (!valid(m) || !radius_ok(R) || !field || Q < 0 || (Q > 0 && (!pos || !clear))) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (Q == 0) return FRP_OK;
    hipLaunchKernelGGL(clearance_kernel, dim3(((unsigned)Q + DIST_THREADS - 1u) / DIST_THREADS), dim3(DIST_THREADS), 0, static_cast<hipStream_t>(stream), geo(m),
                       field, Q, pos, clear, d2);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

int frp_nmpc_occmap_clearance_trace(const frp_nmpc_occmap *m, const uint16_t *field, int R, int B, int S, int stride, const double *pos, const int *active,
                                    double *min_clear, int *hits, int *samples, void *stream)
{
    using namespace frp::occmap;
    if (!valid(m) || !radius_ok(R) || !field || B < 0 || S < 1 || stride < 3) return FRP_ERR_ARG;
    if ((size_t)B * (size_t)S > (size_t)INT_MAX) return FRP_ERR_ARG;
    if (B > 0 && (!pos || !min_clear || !hits || !samples)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (B == 0) return FRP_OK;
    hipLaunchKernelGGL(trace_kernel, dim3(((unsigned)B + DIST_THREADS - 1u) / DIST_THREADS), dim3(DIST_THREADS), 0, static_cast<hipStream_t>(stream), geo(m), field,
                       B, S, stride, pos, active, min_clear, hits, samples);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

int frp_nmpc_occmap_clearance_reset(int B, const int *mask, double *min_clear, int *hits, int *samples, void *stream)
{
    using namespace frp::occmap;
    if (B < 0 || (B > 0 && (!min_clear || !hits || !samples))) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (B == 0) return FRP_OK;
    hipLaunchKernelGGL(clearance_reset_kernel, dim3(((unsigned)B + DIST_THREADS - 1u) / DIST_THREADS), dim3(DIST_THREADS), 0, static_cast<hipStream_t>(stream), B,
                       mask, min_clear, hits, samples);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

} // extern "C"
