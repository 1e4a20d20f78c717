// frp_peers.hpp -- what the two units of frp_nmpc.h section (18) share (frp_peers.hip: the grid, the record, the peer cloud;
// frp_peers_boxes.hip: the peer boxes): the walk over the 27 cells around a planner and the selection of its FRP_PEERS_MAX_NEAR nearest
// peers by one wavefront.  The helpers are frp_peers.hip's text as it was, moved; select_near is the candidate loop of its cloud kernel as
// a function, which that kernel still states itself (called as a function it came out with other bytes; as it is, that unit's device code
// did not change: profiles/peers_avoid_astar_identity.txt).  Both units are built with -ffp-contract=off.  frp_peers_yield.hip (section
// 20, the ranked boxes) is the third: it shares the selection and, with frp_peers_boxes.hip, the box of a centre and the argument rules.
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

// ---- the box of a centre: what frp_peers_boxes.hip and frp_peers_yield.hip (the ranked boxes) both state ----

// floor((x - origin) * inv): posToIndex before its conversion
__device__ inline double voxel_f(double x, double origin, double inv) { return floor((x - origin) * inv); }

// Centre t of planner b's emission order (kept peer t / nc, centre t % nc) as the box it gives: 1 kept (lo / hi clipped, as ints), 0
// dropped, -1 dropped because it holds the planner's own voxel.  own[k]: voxel_f of the planner's position.
__device__ inline int peer_box(const frp_nmpc_peers &p, const frp_nmpc_peers_box_view &v, const double *pos, int stride, const int *kp, int nc, int t, double inv,
                               const double own[3], int lo[3], int hi[3])
{
    const int peer = kp[t / nc], c = t % nc;
    if (peer < 0 || peer >= p.B) return 0;
    const double *src;
    if (c == 0) {
        src = pos + (size_t)peer * stride;
    } else {
        if (v.have_traj[peer] == 0) return 0;
        const int st = v.stages[c - 1];
        if (st < 0 || st >= v.N) return 0;
        src = v.pre_plan + ((size_t)peer * v.N + st) * ROW + 8;
    }
    double fl[3], fh[3];
    bool finite = true, outside = false, mine = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        fl[k] = voxel_f(src[k] - v.half[k], v.origin[k], inv);
        fh[k] = voxel_f(src[k] + v.half[k], v.origin[k], inv);
        const double top = (double)(v.grid[k] - 1);
        finite = finite && finite_d(fl[k]) && finite_d(fh[k]);
        outside = outside || fh[k] < 0.0 || fl[k] > top;
        mine = mine && fl[k] <= own[k] && own[k] <= fh[k];
    }
    if (!finite || outside) return 0;
    if (mine) return -1;
#pragma unroll
    for (int k = 0; k < 3; k++) { // (both bounds are finite, fh >= 0 and fl <= grid - 1: the clipped values are voxel indices)
        const double top = (double)(v.grid[k] - 1);
        lo[k] = fl[k] < 0.0 ? 0 : (int)fl[k];
        hi[k] = fh[k] > top ? v.grid[k] - 1 : (int)fh[k];
    }
    return 1;
}

// ---- host: the argument rules the units apply to a grid and to the positions it was built from ----

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

// the map fields, Q, boxes and count of a view: what the boxes and the path walk both need
static bool map_ok(const frp_nmpc_peers_box_view *v, long long B)
{
    if (!v || v->Q < 0 || !positive(v->resolution) || !v->count || (v->Q > 0 && !v->boxes)) return false;
    for (int k = 0; k < 3; k++)
        if (!finite_d(v->origin[k]) || v->grid[k] < 1) return false;
    return B * v->Q * 6 <= 0x7fffffffLL;
}

// what frp_nmpc_peers_boxes refuses of its arguments, for the entries that take the same ones
static bool boxes_ok(const frp_nmpc_peers *p, const frp_nmpc_peers_box_view *v, const double *pos, int stride)
{
    if (!grid_ok(p) || p->S != 1 || !pos_ok(p, pos, stride) || !map_ok(v, p->B)) return false;
    if (v->N < 1 || v->K < 0 || v->K > FRP_PEERS_MAX_STAGES || !non_negative(v->half[0]) || !non_negative(v->half[1]) || !non_negative(v->half[2])) return false;
    if (!v->pre_plan || !v->have_traj || (v->K > 0 && !v->stages) || !v->overflow || !v->dropped_own) return false;
    return (long long)p->B * v->N * ROW <= 0x7fffffffLL;
}

} // namespace peers
} // namespace frp
