// frp_peers.hpp -- what the two units of frp_nmpc.h section (18) share (frp_peers.hip: the grid, the record, the peer cloud;
// frp_peers_boxes.hip: the peer boxes): the walk over the 27 cells around a planner and the selection of its FRP_PEERS_MAX_NEAR nearest
// peers by one wavefront.  The helpers are frp_peers.hip's text as it was, moved; select_near is the candidate loop of its cloud kernel as
// a function, which that kernel still states itself (called as a function it came out with other bytes; as it is, that unit's device code
// did not change: profiles/peers_avoid_astar_identity.txt).  Both units are built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "../../include/frp_nmpc.h"
#include "frp_fleet.hpp"

#pragma clang fp contract(off)

namespace frp {
namespace peers {

using namespace fleet;

constexpr int WAVE = 64;
constexpr int WAVES = THREADS / WAVE;
constexpr int CAND = FRP_PEERS_MAX_CAND;
constexpr int NEAR = FRP_PEERS_MAX_NEAR;
static_assert(CAND >= NEAR + WAVE && NEAR == WAVE, "a reduced list takes one more step of the wave; one lane per kept peer");

// the wavefront's own ordering of its LDS traffic (frp_device.hpp's form): no instruction on this target beyond the waits
#define FRP_PEERS_SYNC()                                          \
    do {                                                          \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    \
        __builtin_amdgcn_wave_barrier();                          \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");    \
    } while (0)

__device__ inline bool finite3(double x, double y, double z) { return finite_d(x) && finite_d(y) && finite_d(z); }
__device__ inline double sq3(double x, double y, double z) { return (x * x + y * y) + z * z; }

__device__ inline int ncell_of(const frp_nmpc_peers &p) { return p.dims[0] * p.dims[1] * p.dims[2]; }

// The 9 ranges of `items` that hold the 27 cells around cell (cx, cy, cz) of segment s: range r = (dy + 1) + 3 * (dz + 1) is
// [lo, hi), clamped to [0, nitems]; an absent row is the empty range
__device__ inline void range_of(const frp_nmpc_peers &p, int s, int ncell, int nitems, int cx, int cy, int cz, int r, int &lo, int &hi)
{
    const int yy = cy + r % 3 - 1, zz = cz + r / 3 - 1;
    lo = hi = 0;
    if (yy < 0 || yy >= p.dims[1] || zz < 0 || zz >= p.dims[2]) return;
    const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx < p.dims[0] - 1 ? cx + 1 : p.dims[0] - 1;
    const int row = s * ncell + (zz * p.dims[1] + yy) * p.dims[0];
    int a = p.start[row + x0], e = p.start[row + x1 + 1];
    a = a < 0 ? 0 : a;
    e = e > nitems ? nitems : e;
    if (e > a) { lo = a; hi = e; }
}

// is the key (d, i) before (e, j)
__device__ inline bool before(double d, int i, double e, int j) { return d < e || (d == e && i < j); }

// The wave's list (cd, cp)[0 .. n) reduced to its min(n, NEAR) smallest keys, ascending, in (kd, kp) and copied back to the front of the
// list; returns their number.  Called by the whole wave with a uniform n.
__device__ inline int keep_smallest(double *cd, int *cp, double *kd, int *kp, int n, int lane)
{
    FRP_PEERS_SYNC();
    for (int i = lane; i < n; i += WAVE) {
        const double d = cd[i];
        const int q = cp[i];
        int rank = 0;
        for (int j = 0; j < n; j++) rank += before(cd[j], cp[j], d, q) ? 1 : 0;
        if (rank < NEAR) { kd[rank] = d; kp[rank] = q; }
    }
    FRP_PEERS_SYNC();
    const int m = n < NEAR ? n : NEAR;
    if (lane < m) { cd[lane] = kd[lane]; cp[lane] = kp[lane]; }
    FRP_PEERS_SYNC();
    return m;
}

// KEEP IN STEP: cloud_kernel of frp_peers.hip states this loop itself (see the head of this file); an edit here is an edit there, and the
// two oracle comparisons (tests/test_gpu_peers.py, tests/test_gpu_peers_avoid.py) are what binds them until that kernel calls this function.
// Planner b's peers on a grid built with S = 1: the entered q != b with d2 <= R2, ascending in (d2, q), the first NEAR of them in
// kp[0 .. m); returns m, and in `seen` how many there were.  Called by the whole wave (b uniform); cd / cp hold CAND entries, kd / kp NEAR.
__device__ __forceinline__ int select_near(const frp_nmpc_peers &p, const double *pos, int stride, double R2, int b, int lane, double *cd, int *cp,
                                           double *kd, int *kp, int &seen_out)
{
    const int ncell = ncell_of(p), nitems = p.B;
    const int cid = p.key[b];
    int n = 0, seen = 0;
    if (cid >= 0 && cid < ncell) {
        const int cx = cid % p.dims[0], cy = (cid / p.dims[0]) % p.dims[1], cz = cid / (p.dims[0] * p.dims[1]);
        const double *me = pos + (size_t)b * stride;
        const double mx = me[0], my = me[1], mz = me[2];
        int rlo = 0, rhi = 0;
        if (lane < 9) range_of(p, 0, ncell, nitems, cx, cy, cz, lane, rlo, rhi);
        int lo9[9], cum[10];
        cum[0] = 0;
#pragma unroll
        for (int r = 0; r < 9; r++) {
            lo9[r] = __shfl(rlo, r, WAVE);
            cum[r + 1] = cum[r] + (__shfl(rhi, r, WAVE) - lo9[r]);
        }
        const int total = cum[9];
        for (int i0 = 0; i0 < total; i0 += WAVE) {
            if (n + WAVE > CAND) n = keep_smallest(cd, cp, kd, kp, n, lane);
            const int i = i0 + lane;
            bool in = false;
            double d2 = 0.0;
            int q = -1;
            if (i < total) {
                int at = -1;
#pragma unroll
                for (int r = 0; r < 9; r++)
                    if (i >= cum[r] && i < cum[r + 1]) at = lo9[r] + (i - cum[r]);
                if (at >= 0 && at < nitems) q = p.items[at];
                if (q >= 0 && q < p.B && q != b) {
                    const double *o = pos + (size_t)q * stride;
                    d2 = sq3(mx - o[0], my - o[1], mz - o[2]);
                    in = d2 <= R2;
                }
            }
            const unsigned long long mask = __ballot(in);
            if (in) {
                const int at = n + (int)__popcll(mask & ((1ull << lane) - 1ull));
                cd[at] = d2;
                cp[at] = q;
            }
            n += (int)__popcll(mask);
            seen += (int)__popcll(mask);
        }
    }
    seen_out = seen;
    return keep_smallest(cd, cp, kd, kp, n, lane);
}

// ---- host: the argument rules both units apply to a grid and to the positions it was built from ----

static bool grid_ok(const frp_nmpc_peers *p)
{
    if (!p || p->B < 0 || p->S < 1 || !positive(p->cell) || !positive(p->R) || !(p->R <= p->cell)) return false;
    long long cells = p->S;
    for (int i = 0; i < 3; i++) {
        if (!finite_d(p->origin[i]) || p->dims[i] < 1 || p->dims[i] > FRP_PEERS_MAX_CELLS) return false;
        cells *= p->dims[i];
        if (cells > FRP_PEERS_MAX_CELLS) return false;
    }
    if ((long long)p->B * p->S > 0x7fffffffLL) return false;
    return p->start && p->items && p->key && p->slot && p->block_sums && p->outside;
}

static bool pos_ok(const frp_nmpc_peers *p, const double *pos, int stride)
{
    return pos && stride >= 3 && (long long)p->B * p->S * stride <= 0x7fffffffLL;
}

} // namespace peers
} // namespace frp
