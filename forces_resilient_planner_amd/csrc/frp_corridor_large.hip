// frp_corridor_large.hip -- include/frp_nmpc_corridor_large.h: the shared-cloud chain of the corridor for clouds of up to
// FRP_CORRIDOR_LARGE_MAX_POINTS points.
//
// The chain of frp_corridor.hip hands a planner from the one-wavefront kernel to the grid workgroup kernel to the plain-cloud
// workgroup kernel.  Only the last one keeps bit masks over CLOUD positions (3 x P / 8 bytes of LDS: FRP_CORRIDOR_MAX_POINTS), and it is
// reached only by a planner with more than CR_LIST points in a local box.  Here the first two launches are frp_corridor.hip's own
// (corridor_launch_listed: same kernels, dynamic LDS for the list alone), and the third is corridor_large_kernel below:
//   * the first scan of a decomposition gathers the in-box points through the grid -- scan_grid's cell rows, the shared box test
//     (load_box / in_box / box_hull), the shared cut -- into THIS WORKGROUP's list in device memory: uint32 entries, cloud index in
//     bits 0-30, "inside the seed ellipsoid" in bit 31, as the LDS list of the grid kernel;
//   * every later scan is frp_corridor_scan.inc's scan<> over list positions (its `list` pointer is generic: LDS there, HBM here);
//     the three masks cover FRP_CORRIDOR_LARGE_LIST positions: 24 KB of static LDS, the plain-cloud kernel's maximum today;
//   * the stage loop is corridor_kernel's, statement for statement, without the register tile (a box that gets here holds more than
//     CR_LIST points; the tile holds 1280).  Minima are tie-broken by the original cloud index, so the polytopes are those the
//     plain-cloud kernel computes from the same visible points, bit for bit (tests/test_gpu_corridor_large.py);
//   * S = min(B, FRP_CORRIDOR_LARGE_GROUPS) workgroups walk the planners b = wg, wg + S, ... and skip the unflagged ones: a static
//     assignment -- no queue, no flag polled across workgroups, no grid barrier -- so the workspace is S lists whatever B is;
//   * a box with more than FRP_CORRIDOR_LARGE_LIST points is refused for that planner (the marker of the header), never truncated.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/frp_nmpc.h"

// (frp_corridor.hip: every corridor kernel computes the same bits from the same inputs -- no implicit contraction in this file either)
#pragma clang fp contract(off)

#include "frp_corridor_scan.inc"

namespace frp {

constexpr int CL_LIST = FRP_CORRIDOR_LARGE_LIST, CL_WORDS = CL_LIST / 64, CL_GROUPS = FRP_CORRIDOR_LARGE_GROUPS;
static_assert(CL_LIST % 64 == 0 && 3 * CL_WORDS * sizeof(uint64_t) == 24576, "three masks over the list: 24 KB of LDS");
static_assert(FRP_CORRIDOR_LARGE_MAX_POINTS < (1ll << 31), "a list entry holds a cloud index in bits 0-30");

// scan_grid with the list in device memory and FRP_CORRIDOR_LARGE_LIST entries: the cell rows under the local box's hull, CR_GROWS rows
// in flight per wave, every in-box (and visible) point appended to `list`; returns the closest point inside the seed ellipsoid.
// u.count ends as the number of in-box points, whether or not they all fitted.
template <bool CUT>
__device__ __forceinline__ Best gather_grid(const frp_nmpc_corridor &c, const CutBox &cb, uint32_t *list, Uni &u, Best *s_red, int &phase)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const M3 Ci = ld3(u.Ci);
    const double d[3] = {u.mid[0], u.mid[1], u.mid[2]};
    const BoxFrame f = load_box(u, c);
    int lo[3], hi[3];
    box_hull(f, c, lo, hi);
    const int ny = hi[1] - lo[1] + 1, rows = ny * (hi[2] - lo[2] + 1), nx = c.grid_dims[0];
    Best best{1.7976931348623157e308, 0x7fffffff, 0.0, 0.0, 0.0};
    for (int r0 = wave; r0 < rows; r0 += CR_WAVES * CR_GROWS) {
        int beg[CR_GROWS], end[CR_GROWS], most = 0;
#pragma unroll
        for (int k = 0; k < CR_GROWS; ++k) {
            const int r = r0 + k * CR_WAVES;
            beg[k] = end[k] = 0;
            if (r < rows) {
                const size_t row = ((size_t)(lo[2] + r / ny) * c.grid_dims[1] + (lo[1] + r % ny)) * nx;
                beg[k] = c.grid_start[row + lo[0]];
                end[k] = c.grid_start[row + hi[0] + 1];
            }
            most = max(most, end[k] - beg[k]);
        }
        for (int off = 0; off < most; off += 64) {
            double x[CR_GROWS], y[CR_GROWS], z[CR_GROWS];
            int id[CR_GROWS];
#pragma unroll
            for (int k = 0; k < CR_GROWS; ++k) {
                const int p = beg[k] + off + lane;
                const bool ok = p < end[k];
                const size_t p3 = 3 * (size_t)(ok ? p : 0);
                x[k] = ok ? c.grid_points[p3] : 0.0; y[k] = ok ? c.grid_points[p3 + 1] : 0.0; z[k] = ok ? c.grid_points[p3 + 2] : 0.0;
                id[k] = ok ? c.grid_index[p] : -1;
            }
            uint64_t w0[CR_GROWS];
            bool i1[CR_GROWS];
            int total = 0;
#pragma unroll
            for (int k = 0; k < CR_GROWS; ++k) {
                bool in0 = in_box(f, x[k], y[k], z[k], id[k]);
                i1[k] = false;
                if (CUT) in0 = in0 && cut_sees<CUT>(cb, x[k], y[k], z[k]);
                if (in0) {
                    const double dist = ell_dist2(Ci, d, x[k], y[k], z[k]);
                    i1[k] = dist <= 1;
                    if (i1[k] && before(dist, id[k], best.dist, best.idx)) best = Best{dist, id[k], x[k], y[k], z[k]};
                }
                w0[k] = __ballot(in0);
                total += (int)__popcll(w0[k]);
            }
            if (total) {
                int at = 0;
                if (lane == 0) at = atomicAdd(&u.count, total);
                at = __builtin_amdgcn_readfirstlane(at);
#pragma unroll
                for (int k = 0; k < CR_GROWS; ++k) {
                    const int mine = at + (int)__popcll(w0[k] & ((1ull << lane) - 1));
                    if (((w0[k] >> lane) & 1) && mine < CL_LIST) list[mine] = (uint32_t)id[k] | (i1[k] ? 0x80000000u : 0u); // (bounded: never past this workgroup's list)
                    at += (int)__popcll(w0[k]);
                }
            }
        }
    }
    return block_min(best, s_red, phase); // (its barrier also orders the list's stores before the loads of the scans behind)
}

// Three workgroups per CU like corridor_kernel (a decomposition is a chain of latency-bound scans); 27 KB of LDS per workgroup leaves
// room for five, so the register budget decides, as there.
template <bool CUT>
__global__ __launch_bounds__(CR_THREADS) __attribute__((amdgpu_waves_per_eu(FRP_CR_WPE, FRP_CR_WPE))) void corridor_large_kernel(CorridorArgs<CUT> args, uint32_t *workspace, int *overflow)
{
    const frp_nmpc_corridor &c = corridor_of(args);
    __shared__ uint64_t s_mask[3 * CL_WORDS];
    __shared__ double s_A[FRP_CORRIDOR_MAX_F * 3], s_b[FRP_CORRIDOR_MAX_F];
    __shared__ Best s_red[2 * CR_WAVES];
    __shared__ Uni u;
    int phase = 0;
    const int tid = threadIdx.x;
    uint64_t *m0 = s_mask, *m1 = s_mask + CL_WORDS, *m2 = s_mask + 2 * CL_WORDS; // obs_, obs, working list -- over LIST positions
    uint32_t *list = workspace + (size_t)blockIdx.x * CL_LIST;
    int P_live = c.cloud_count ? c.cloud_count[0] : c.P;
    P_live = P_live < c.P ? P_live : c.P;
    const int max_rounds = P_live + 8; // (corridor_kernel: a list is exhausted after at most that many rounds; only non-finite input needs the bound)
    Scan sc;
    sc.pts = c.cloud;
    sc.list = list;

    for (int b = (int)blockIdx.x; b < c.B; b += (int)gridDim.x) {
        // (every thread reads the flag before the first barrier below; thread 0 overwrites it only behind several of them)
        if (c.poly_index[(size_t)b * c.N] != -1) {
            if (tid == 0 && overflow) overflow[b] = 0;
            continue;
        }
        const double *ref = c.ref_pos + (size_t)b * c.N * 3, *yaw = c.ref_yaw + (size_t)b * c.N, *Eb = c.ellipsoid + (size_t)b * c.N * 9;
        CutBox cb = {};
        if (CUT) cb = load_cut(cut_of(args), b);
        int npoly = 0, rows = 0;
        bool refused = false;
        if (tid == 0) u.overflow = 0;

        for (int i = 0; i < c.N; ++i) {
            // ---- does the stage's inflated tube ellipsoid fit the last polytope? (nmpc_solver.cpp:291-313) ----------
            if (npoly > 0) {
                int viol = 0;
                if (tid < rows) {
                    const double a0 = s_A[3 * tid], a1 = s_A[3 * tid + 1], a2 = s_A[3 * tid + 2];
                    const double *E = Eb + 9 * i;
                    const double e0 = E[0] * a0 + E[1] * a1 + E[2] * a2, e1 = E[3] * a0 + E[4] * a1 + E[5] * a2, e2 = E[6] * a0 + E[7] * a1 + E[8] * a2;
                    const double add = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
                    viol = (a0 * ref[3 * i] + a1 * ref[3 * i + 1] + a2 * ref[3 * i + 2] - (s_b[tid] - c.inflation * add)) > 0;
                }
                if (!__syncthreads_or(viol)) {
                    if (tid == 0) c.poly_index[(size_t)b * c.N + i] = npoly - 1;
                    continue;
                }
            }
            // ---- new decomposition around the seed segment (nmpc_solver.cpp:315-329) -------------------------------
            if (tid == 0) {
                double sy, cy;
                sincos(yaw[i], &sy, &cy);
                const double p1[3] = {ref[3 * i], ref[3 * i + 1], ref[3 * i + 2]};
                const double p2[3] = {p1[0] + c.seed_len * cy, p1[1] + c.seed_len * sy, p1[2]};
                const double dv[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
                const double len = sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) u.mid[k] = (p1[k] + p2[k]) / 2;
                u.len = len;
                { // local box planes (line_segment.h:47-85); the large route always has a box
                    const double dir[3] = {dv[0] / len, dv[1] / len, dv[2] / len};
                    double dh[3] = {dir[1], -dir[0], 0.0};
                    double hn = sqrt(dh[0] * dh[0] + dh[1] * dh[1]);
                    if (hn == 0.0) { dh[0] = -1.0; dh[1] = 0.0; hn = 1.0; }
                    dh[0] /= hn; dh[1] /= hn;
                    const double dvv[3] = {dir[1] * dh[2] - dir[2] * dh[1], dir[2] * dh[0] - dir[0] * dh[2], dir[0] * dh[1] - dir[1] * dh[0]};
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        u.frame[0][k] = dh[k]; u.frame[1][k] = dir[k]; u.frame[2][k] = dvv[k]; u.p1[k] = p1[k];
                        u.box[0][k] = p1[k] + dh[k] * c.bbox[1];  u.box[6][k] = dh[k];
                        u.box[1][k] = p1[k] - dh[k] * c.bbox[1];  u.box[7][k] = -dh[k];
                        u.box[2][k] = p2[k] + dir[k] * c.bbox[0]; u.box[8][k] = dir[k];
                        u.box[3][k] = p1[k] - dir[k] * c.bbox[0]; u.box[9][k] = -dir[k];
                        u.box[4][k] = p1[k] + dvv[k] * c.bbox[2]; u.box[10][k] = dvv[k];
                        u.box[5][k] = p1[k] - dvv[k] * c.bbox[2]; u.box[11][k] = -dvv[k];
                    }
                }
                // seed ellipsoid (line_segment.h:139-154)
                const double f = len / 2;
                double ax0 = f + c.offset_x, ax1 = f, ax2 = f, c00 = f + c.offset_x, cdd = f;
                if (ax0 > 0) { const double ratio = ax1 / ax0; ax0 *= ratio; ax1 *= ratio; ax2 *= ratio; c00 *= ratio; cdd *= ratio; }
                u.ax[0] = ax0; u.ax[1] = ax1; u.ax[2] = ax2;
                const double pitch = atan2(-dv[2], sqrt(dv[0] * dv[0] + dv[1] * dv[1])), yw = atan2(dv[1], dv[0]);
                const M3 Ri = mul(quat_to_rot(cos(yw / 2), 0, 0, sin(yw / 2)), quat_to_rot(cos(pitch / 2), 0, sin(pitch / 2), 0));
                u.count = 0;
                st3(u.Ri, Ri); st3(u.Rf, Ri);
                st3(u.Ci, inverse(rot_diag_rot(Ri, c00, cdd, cdd)));
            }
            __syncthreads();
            Best cp = gather_grid<CUT>(c, cb, list, u, s_red, phase);
            if (u.count > CL_LIST) { // (uniform: read behind the barrier of gather_grid's reduction) more points than the list holds: refuse
                refused = true;
                break;
            }
            sc.Pn = u.count; sc.W = (u.count + 63) / 64;
            for (int g = tid >> 6; g < sc.W; g += CR_WAVES) { // the masks over list positions: obs_ = all, obs = inside the seed ellipsoid
                const int pos = g * 64 + (tid & 63);
                const bool valid = pos < sc.Pn;
                const uint64_t w0 = __ballot(valid), w1 = __ballot(valid && (list[valid ? pos : 0] >> 31));
                if ((tid & 63) == 0) { m0[g] = w0; m1[g] = w1; m2[g] = w1; }
            }
            // shrink the second axis until no obstacle is inside (line_segment.h:156-181)
            for (int guard = 0; cp.idx != 0x7fffffff && guard < max_rounds; ++guard) {
                if (tid == 0) {
                    const double pw[3] = {cp.x - u.mid[0], cp.y - u.mid[1], cp.z - u.mid[2]};
                    const M3 Ri = ld3(u.Ri);
                    double p[3];
                    tmul(Ri, pw, p);
                    const double roll = atan2(p[2], p[1]);
                    const M3 Rf = mul(Ri, quat_to_rot(cos(roll / 2), sin(roll / 2), 0, 0));
                    tmul(Rf, pw, p);
                    if (p[0] < u.ax[0]) u.ax[1] = fabs(p[1]) / sqrt(1 - (p[0] / u.ax[0]) * (p[0] / u.ax[0]));
                    st3(u.Rf, Rf);
                    st3(u.Ci, inverse(rot_diag_rot(Rf, u.ax[0], u.ax[1], u.ax[1])));
                }
                __syncthreads();
                cp = scan<KEEP_OUTSIDE>(sc, m2, m2, u, s_red, phase);
            }
            // third axis (line_segment.h:183-208)
            if (tid == 0) st3(u.Ci, inverse(rot_diag_rot(ld3(u.Rf), u.ax[0], u.ax[1], u.ax[2])));
            __syncthreads();
            cp = scan<KEEP_INSIDE>(sc, m1, m2, u, s_red, phase);
            for (int guard = 0; cp.idx != 0x7fffffff && guard < max_rounds; ++guard) {
                if (tid == 0) {
                    const double pw[3] = {cp.x - u.mid[0], cp.y - u.mid[1], cp.z - u.mid[2]};
                    const M3 Rf = ld3(u.Rf);
                    double p[3];
                    tmul(Rf, pw, p);
                    const double dd = 1 - (p[0] / u.ax[0]) * (p[0] / u.ax[0]) - (p[1] / u.ax[1]) * (p[1] / u.ax[1]);
                    if (dd > CR_EPS) u.ax[2] = fabs(p[2]) / sqrt(dd);
                    st3(u.Ci, inverse(rot_diag_rot(Rf, u.ax[0], u.ax[1], u.ax[2])));
                }
                __syncthreads();
                cp = scan<KEEP_OUTSIDE>(sc, m2, m2, u, s_red, phase);
            }
            // hyperplanes (decomp_base.h:63-83) + LinearConstraint rows (polyhedron.h:98-118)
            double *gA = c.poly_A + (((size_t)b * c.N + npoly) * c.F) * 3, *gb = c.poly_b + ((size_t)b * c.N + npoly) * c.F;
            if (tid == 0) {
                const M3 Ci = ld3(u.Ci);
                st3(u.CC, mul(Ci, transpose(Ci))); // C^-1 C^-T (ellipsoid.h:53-58)
                u.rows = 0;
            }
            cp = scan<KEEP_ALL>(sc, m0, m2, u, s_red, phase); // Ci is unchanged since the last barrier
            for (int guard = 0; cp.idx != 0x7fffffff && guard < max_rounds; ++guard) {
                const double q[3] = {cp.x, cp.y, cp.z};
                const double w[3] = {q[0] - u.mid[0], q[1] - u.mid[1], q[2] - u.mid[2]};
                double n[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) n[k] = u.CC[3 * k] * w[0] + u.CC[3 * k + 1] * w[1] + u.CC[3 * k + 2] * w[2];
                const double nl = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) n[k] /= nl;
                if (tid == 0) emit_row(u, q, n, c.F, s_A, s_b, gA, gb);
                cp = scan<KEEP_BEHIND_PLANE>(sc, m2, m2, u, s_red, phase, q, n);
            }
            if (tid == 0) {
                for (int k = 0; k < 6; ++k) emit_row(u, u.box[k], u.box[6 + k], c.F, s_A, s_b, gA, gb);
                c.poly_nfaces[(size_t)b * c.N + npoly] = u.rows;
                c.poly_index[(size_t)b * c.N + i] = npoly;
            }
            __syncthreads(); // rows of the new polytope visible to the containment check of the next stage
            rows = u.rows < c.F ? u.rows : c.F;
            ++npoly;
        }
        if (tid == 0) {
            if (refused) { // the documented marker: nothing of this planner's result is to be used
                for (int k = 0; k < c.N; ++k) { c.poly_nfaces[(size_t)b * c.N + k] = 0; c.poly_index[(size_t)b * c.N + k] = 0; }
                if (c.poly_count) c.poly_count[b] = INT_MIN;
            } else {
                for (int k = npoly; k < c.N; ++k) c.poly_nfaces[(size_t)b * c.N + k] = 0;
                if (c.poly_count) c.poly_count[b] = u.overflow ? -npoly : npoly;
            }
            if (overflow) overflow[b] = refused ? 1 : 0;
        }
        __syncthreads(); // thread 0 is done with u before the next planner's first stage resets it
    }
}

} // namespace frp

extern "C" size_t frp_nmpc_corridor_large_workspace_bytes(int B)
{
    if (B < 1) return 0;
    return (size_t)(B < frp::CL_GROUPS ? B : frp::CL_GROUPS) * frp::CL_LIST * sizeof(uint32_t);
}

extern "C" int frp_nmpc_corridor_batch_large(const frp_nmpc_corridor *p, const frp_nmpc_corridor_cut *cut, const frp_nmpc_corridor_large *w, void *stream)
{
    if (!frp::corridor_args_ok(p, cut, FRP_CORRIDOR_LARGE_MAX_POINTS) || p->cloud_per_planner) return FRP_ERR_ARG;
    if (!p->grid_start || !(p->bbox[0] != 0.0 || p->bbox[1] != 0.0 || p->bbox[2] != 0.0)) return FRP_ERR_ARG; // (corridor_args_ok has checked the rest of a given grid)
    if (!w || !w->workspace || w->workspace_bytes < frp_nmpc_corridor_large_workspace_bytes(p->B)) return FRP_ERR_ARG;
    int devices = 0; // (as the occupancy map's calls: valid arguments without a device are FRP_ERR_NO_DEVICE, not a failed launch)
    if (hipGetDeviceCount(&devices) != hipSuccess || devices < 1) return FRP_ERR_NO_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    frp::corridor_launch_listed(p, cut, st); // launches 1 and 2: frp_corridor.hip's kernels, LDS for the list alone
    const unsigned groups = (unsigned)(p->B < frp::CL_GROUPS ? p->B : frp::CL_GROUPS);
    uint32_t *lists = static_cast<uint32_t *>(w->workspace);
    if (cut) {
        const frp::CorridorCutArgs a = {*p, *cut};
        hipLaunchKernelGGL(frp::corridor_large_kernel<true>, dim3(groups), dim3(frp::CR_THREADS), 0, st, a, lists, w->overflow);
    } else
        hipLaunchKernelGGL(frp::corridor_large_kernel<false>, dim3(groups), dim3(frp::CR_THREADS), 0, st, *p, lists, w->overflow);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}
