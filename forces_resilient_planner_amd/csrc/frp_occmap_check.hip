// frp_nmpc.h section (8), frp_nmpc_occmap_check.h: OccMap::checkPosSurround (occ_grid/src/occ_map.cpp:625-643) and the two loops
// of its caller, NMPCManage::checkReplanCallback (plan_manage/src/nmpc_manage.cpp:285-341), on the map's bit plane.
//
//   * checkPosSurround probes the full product {-hx..hx} x {-hy..hy} x {-hz..hz} and every probe's voxel index
//     floor(((pos[a] + (double)i * resolution) - origin[a]) * resolution_inv) depends on one axis only.  A wavefront therefore
//     computes 2h + 1 <= 63 indices per axis, one per lane, with the reference's operations (this file is compiled with
//     -ffp-contract=off; floor(pos) + i is NOT the same index at voxel faces), instead of (2hx+1)(2hy+1)(2hz+1) probes.
//   * getVoxelState (:95-106) per probe: an index outside the map on ANY axis is -1, a collision; because the box is a product,
//     one such index on one axis decides the point.  Otherwise every probe is in the map, an index outside the local box on
//     any axis makes its probes 0 (free), and what is left is again a product: surviving x times surviving y times surviving z.
//   * the surviving z indices become a mask per 32-bit word of the bit plane; the lanes take the (x, y) columns, AND the column's
//     word with the mask and vote.  Rounding may map two offsets to one index or skip one: the indices are the computed ones, a
//     column read twice changes nothing.
//   * no atomics, no waiting between workgroups, log_odds and occ are not read.
#include "frp_occmap_check.hpp"

namespace frp {
namespace occmap {

// checkPosSurround for Q points: one wavefront per point
__global__ __launch_bounds__(256) void check_surround_kernel(Geo g, Half hf, int Q, const double *pos, const int *planner, const int *local_box,
                                                             const uint32_t *plane, int *free_out)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t q = (size_t)blockIdx.x * 4 + wave;
    if (q >= (size_t)Q) return;
    const int *bx = local_box ? local_box + 6 * (size_t)(planner ? planner[q] : 0) : nullptr;
    const bool ok = surround_free(g, hf, pos[3 * q], pos[3 * q + 1], pos[3 * q + 2], bx, plane, lane);
    if (lane == 0) free_out[q] = ok ? 1 : 0;
}

// checkReplanCallback's path loop (:329-340) for planner blockIdx.x: wave w takes the samples w, w + 4, ... in rising order and
// stops at its first collision; the smallest of the four is first_hit
__global__ __launch_bounds__(256) void check_paths_kernel(Geo g, Half hf, int K, int stride, const double *kino_path, const int *kino_size, const int *have_traj,
                                                          const int *local_box, const uint32_t *plane, int *first_hit)
{
    __shared__ int s_hit[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int n = kino_size[b];
    if (n > K) n = K;
    if (have_traj && have_traj[b] == 0) n = 0; // :329
    const int *bx = local_box ? local_box + 6 * (size_t)b : nullptr;
    const double *path = kino_path + (size_t)b * K * 3;
    int hit = 0x7fffffff;
    for (long long s = (long long)wave * stride; s < n; s += 4ll * stride) { // i += 5 (:331)
        const double *p = path + 3 * (size_t)s;
        if (!surround_free(g, hf, p[0], p[1], p[2], bx, plane, lane)) { hit = (int)s; break; } // :333-338
    }
    if (lane == 0) s_hit[wave] = hit;
    __syncthreads();
    if (threadIdx.x == 0) {
        int m = s_hit[0];
        for (int k = 1; k < 4; k++) m = s_hit[k] < m ? s_hit[k] : m;
        first_hit[b] = m == 0x7fffffff ? -1 : m;
    }
}

struct Goals {
    int B, n_groups, group_size;
    double *end_pt;
    const int *have_target, *local_box;
    const double *table;
    int *blocked, *hits;
};

// checkReplanCallback's goal test and search (:289-316): one wavefront per planner; the candidates are walked one after the
// other because each is taken relative to the goal the candidates before it may have moved
__global__ __launch_bounds__(256) void check_goals_kernel(Geo g, Half check, Half search, Goals a, const uint32_t *plane)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t b = (size_t)blockIdx.x * 4 + wave;
    if (b >= (size_t)a.B) return;
    if (a.have_target && a.have_target[b] == 0) { // :289
        if (lane == 0) { a.blocked[b] = 0; a.hits[b] = 0; }
        return;
    }
    const int *bx = a.local_box ? a.local_box + 6 * b : nullptr;
    double ex = a.end_pt[3 * b], ey = a.end_pt[3 * b + 1], ez = a.end_pt[3 * b + 2];
    int hits = 0;
    const bool blocked = !surround_free(g, check, ex, ey, ez, bx, plane, lane); // :291
    if (blocked) {
        for (int grp = 0; grp < a.n_groups; grp++) {          // r, theta (:299-300)
            for (int k = 0; k < a.group_size; k++) {          // nz (:301)
                const double *t = a.table + 3 * ((size_t)grp * a.group_size + k);
                const double nx = ex + t[0], ny = ey + t[1], nz = t[2]; // :303-305, r * cos(theta) and r * sin(theta) from the table
                if (surround_free(g, search, nx, ny, nz, bx, plane, lane)) { // :308
                    ex = nx; ey = ny; ez = nz; hits++;          // :309
                    break;                                      // :312 -- leaves the nz loop only
                }
            }
        }
        if (hits > 0 && lane == 0) { a.end_pt[3 * b] = ex; a.end_pt[3 * b + 1] = ey; a.end_pt[3 * b + 2] = ez; }
    }
    if (lane == 0) { a.blocked[b] = blocked ? 1 : 0; a.hits[b] = hits; }
}

} // namespace occmap
} // namespace frp

extern "C" {

int frp_nmpc_occmap_check_surround(const frp_nmpc_occmap *m, const frp_nmpc_occmap_body *body, double inflate_ratio, int Q, const double *pos,
                                   const int *planner, const int *local_box, int *free_out, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace frp::occmap;
    Half hf;
    if (!args_ok(m, workspace, workspace_bytes) || !half_extents(m, body, inflate_ratio, &hf)) return FRP_ERR_ARG;
    if (Q < 0 || (Q > 0 && (!pos || !free_out)) || (planner && !local_box)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (Q == 0) return FRP_OK;
    hipLaunchKernelGGL(check_surround_kernel, dim3(((unsigned)Q + 3u) / 4u), dim3(256), 0, static_cast<hipStream_t>(stream), geo(m), hf, Q, pos, planner,
                       local_box, static_cast<const uint32_t *>(workspace), free_out);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

int frp_nmpc_occmap_check_paths(const frp_nmpc_occmap *m, const frp_nmpc_occmap_body *body, double inflate_ratio, int B, int K, int stride,
                                const double *kino_path, const int *kino_size, const int *have_traj, const int *local_box, int *first_hit,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace frp::occmap;
    Half hf;
    if (!args_ok(m, workspace, workspace_bytes) || !half_extents(m, body, inflate_ratio, &hf)) return FRP_ERR_ARG;
    if (B < 0 || K <= 0 || stride <= 0 || (B > 0 && (!kino_path || !kino_size || !first_hit))) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (B == 0) return FRP_OK;
    hipLaunchKernelGGL(check_paths_kernel, dim3((unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), geo(m), hf, K, stride, kino_path, kino_size,
                       have_traj, local_box, static_cast<const uint32_t *>(workspace), first_hit);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

int frp_nmpc_occmap_check_goals(const frp_nmpc_occmap *m, const frp_nmpc_occmap_body *body, double inflate_check, double inflate_search, int B,
                                double *end_pt, const int *have_target, const int *local_box, int n_groups, int group_size, const double *table,
                                int *goal_blocked, int *goal_hits, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace frp::occmap;
    Half check, search;
    if (!args_ok(m, workspace, workspace_bytes) || !half_extents(m, body, inflate_check, &check) || !half_extents(m, body, inflate_search, &search))
        return FRP_ERR_ARG;
    if (B < 0 || n_groups < 0 || group_size <= 0 || (size_t)n_groups * (size_t)group_size > (size_t)1 << 24 || (n_groups > 0 && !table)) return FRP_ERR_ARG;
    if (B > 0 && (!end_pt || !goal_blocked || !goal_hits)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (B == 0) return FRP_OK;
    Goals a;
    a.B = B; a.n_groups = n_groups; a.group_size = group_size; a.end_pt = end_pt; a.have_target = have_target; a.local_box = local_box;
    a.table = table; a.blocked = goal_blocked; a.hits = goal_hits;
    hipLaunchKernelGGL(check_goals_kernel, dim3(((unsigned)B + 3u) / 4u), dim3(256), 0, static_cast<hipStream_t>(stream), geo(m), check, search, a,
                       static_cast<const uint32_t *>(workspace));
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

} // extern "C"
