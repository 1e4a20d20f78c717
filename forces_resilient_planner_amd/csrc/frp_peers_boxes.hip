// frp_peers_boxes.hip -- frp_nmpc.h section (19): a planner's peers as boxes of map voxels, and the safety timer's path walk against
// them.  The third consumer of the boxes, the kinodynamic A* on the map plus a planner's boxes, is frp_astar_peers.hip.  No reference
// counterpart; tests/peers_avoid_oracle.py is the executable statement -- brute force over all pairs -- and this file agrees with it to
// the bit.
//
//   * boxes: one wavefront per planner, four per workgroup, on a grid built with S = 1 -- the cloud kernel's shape.  The peers and their
//     order are select_near of frp_peers.hpp (the cloud kernel's rule).  Then two passes over the <= 64 * 9 centres, lane = centre in
//     emission order (peer rank first, then centre): count the kept boxes and the own-voxel drops (ballots), and -- where the count
//     fits Q -- write, each lane at the prefix count of the kept before it.  LDS: the selection's 52224 bytes per workgroup.  Waves of a
//     workgroup share nothing; there is no __syncthreads in that kernel.
//   * A bound is floor(((c -+ half) - origin) * inv), posToIndex's operations, one rounding each (this unit is built with
//     -ffp-contract=off as well); it stays a double until it was compared with 0 and grid: a NaN, an infinity or a bound beyond int
//     never reaches a conversion.  A row is written only at b * Q + at with 0 <= at < Q.
//   * path walk: one thread per planner, samples 0, stride, ... in rising order, stops at the first hit.  It reads min(count, Q) rows.
//   * Every store is a plain C++ store from a vector lane; no atomics, no inline assembly.
#include "frp_peers.hpp"

namespace frp {
namespace peers {

__global__ __launch_bounds__(THREADS) void boxes_kernel(frp_nmpc_peers p, frp_nmpc_peers_box_view v, const double *pos, int stride, double R2, double inv)
{
    __shared__ double cand_d[WAVES][CAND];
    __shared__ int cand_p[WAVES][CAND];
    __shared__ double kept_d[WAVES][NEAR];
    __shared__ int kept_p[WAVES][NEAR];
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    const int b = blockIdx.x * WAVES + wave; // (uniform in the wave)
    if (b >= p.B) return;
    int *kp = kept_p[wave];
    int seen = 0;
    const int m = select_near(p, pos, stride, R2, b, lane, cand_d[wave], cand_p[wave], kept_d[wave], kp, seen);
    const int nc = 1 + v.K, slots = m * nc;
    const double *me = pos + (size_t)b * stride;
    const double own[3] = {voxel_f(me[0], v.origin[0], inv), voxel_f(me[1], v.origin[1], inv), voxel_f(me[2], v.origin[2], inv)};
    int n = 0, dropped = 0;
    for (int t0 = 0; t0 < slots; t0 += WAVE) {
        int lo[3], hi[3];
        const int r = t0 + lane < slots ? peer_box(p, v, pos, stride, kp, nc, t0 + lane, inv, own, lo, hi) : 0;
        n += (int)__popcll(__ballot(r == 1));
        dropped += (int)__popcll(__ballot(r == -1));
    }
    const bool fits = n <= v.Q;
    if (fits) {
        int at0 = 0;
        for (int t0 = 0; t0 < slots; t0 += WAVE) {
            int lo[3], hi[3];
            const bool ok = t0 + lane < slots && peer_box(p, v, pos, stride, kp, nc, t0 + lane, inv, own, lo, hi) == 1;
            const unsigned long long mask = __ballot(ok);
            const int at = at0 + (int)__popcll(mask & ((1ull << lane) - 1ull));
            if (ok && at >= 0 && at < v.Q) {
                int *dst = v.boxes + ((size_t)b * v.Q + at) * 6;
                dst[0] = lo[0]; dst[1] = lo[1]; dst[2] = lo[2]; dst[3] = hi[0]; dst[4] = hi[1]; dst[5] = hi[2];
            }
            at0 += (int)__popcll(mask);
        }
    }
    if (lane == 0) {
        v.count[b] = fits ? n : -n;
        v.overflow[b] = seen > NEAR ? 1 : 0;
        v.dropped_own[b] = dropped;
    }
}

// checkReplanCallback's path loop (nmpc_manage.cpp:329-340) for planner b against its boxes
__global__ __launch_bounds__(THREADS) void check_paths_kernel(frp_nmpc_peers_box_view v, int B, int K, int stride, double inv, const double *kino_path,
                                                              const int *kino_size, const int *have_traj, int *first_hit)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= B) return;
    int n = kino_size[b];
    if (n > K) n = K;
    if (have_traj && have_traj[b] == 0) n = 0;
    int nb = v.count[b];
    nb = nb < 1 ? 0 : (nb > v.Q ? v.Q : nb);
    const int *bx = v.boxes + (size_t)b * v.Q * 6;
    const double *path = kino_path + (size_t)b * K * 3;
    int hit = -1;
    for (long long s = 0; s < n && hit < 0 && nb > 0; s += stride) {
        const double *q = path + 3 * (size_t)s;
        int id[3];
        bool in_map = true;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double f = voxel_f(q[k], v.origin[k], inv);
            const bool ok = f >= 0.0 && f <= (double)(v.grid[k] - 1); // (a NaN fails both)
            in_map = in_map && ok;
            id[k] = ok ? (int)f : -1;
        }
        if (!in_map) continue;
        for (int j = 0; j < nb; j++) {
            const int *r = bx + 6 * j;
            if (r[0] <= id[0] && id[0] <= r[3] && r[1] <= id[1] && id[1] <= r[4] && r[2] <= id[2] && id[2] <= r[5]) { hit = (int)s; break; }
        }
    }
    first_hit[b] = hit;
}

} // namespace peers
} // namespace frp

extern "C" {

int frp_nmpc_peers_boxes(const frp_nmpc_peers *p, const frp_nmpc_peers_box_view *v, const double *pos, int stride, void *stream)
{
    using namespace frp::peers;
    if (!boxes_ok(p, v, pos, stride)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (p->B == 0) return FRP_OK;
    return launch(boxes_kernel, (unsigned)((p->B + WAVES - 1) / WAVES), stream, *p, *v, pos, stride, p->R * p->R, 1.0 / v->resolution);
}

int frp_nmpc_peers_check_paths(const frp_nmpc_peers_box_view *v, int B, int path_K, int stride, const double *kino_path, const int *kino_size,
                               const int *have_traj, int *first_hit, void *stream)
{
    using namespace frp::peers;
    if (B < 0 || !map_ok(v, B) || path_K < 1 || stride < 1 || (B > 0 && (!kino_path || !kino_size || !first_hit))) return FRP_ERR_ARG;
    if ((long long)B * path_K * 3 > 0x7fffffffLL) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (B == 0) return FRP_OK;
    return launch(check_paths_kernel, blocks_for(B), stream, *v, B, path_K, stride, 1.0 / v->resolution, kino_path, kino_size, have_traj, first_hit);
}

} // extern "C"
