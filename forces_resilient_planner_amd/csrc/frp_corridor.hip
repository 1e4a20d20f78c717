// frp_corridor.hip -- SURVEY 8f row f-3: corridor generation and selection (NMPCSolver::getSikangConst over the
// horizon, nmpc_solver.cpp:288-332, on top of DecompROS' EllipsoidDecomp3D::dilate) batched on the device.  Inputs
// are the stage references (row f-4 / the caller), the tube matrices of frp_nmpc_tube_batch (f-2) and the obstacle
// cloud; outputs are exactly the polytope inputs of frp_nmpc_pack_batch (f-1): poly_A, poly_b, poly_nfaces,
// poly_index.
//
// Reference (src/ThirdParty/DecompROS/decomp_ros_utils/include/ unless noted):
//   getSikangConst                   plan_manage/src/nmpc_solver.cpp:288-332
//   EllipsoidDecomp3D::dilate / get_constraints   decomp_util/ellipsoid_decomp.h:47-90
//   DecompBase::set_obs / find_polyhedron         decomp_util/decomp_base.h:33-38, 63-83
//   LineSegment::dilate / add_local_bbox / find_ellipsoid (3D)   decomp_util/line_segment.h:31-35, 47-85, 136-211
//   Ellipsoid::dist / closest_point / closest_hyperplane         decomp_geometry/ellipsoid.h:19-58
//   Polyhedron::inside, LinearConstraint(p0, planes)             decomp_geometry/polyhedron.h:51-58, 98-118
//   vec3_to_rotation                 decomp_geometry/geometric_utils.h:27-35;  epsilon_  decomp_basis/data_type.h:129
//
// Mapping.  One 256-thread workgroup per planner walks the stages in order (a stage reuses the polytope made for an
// earlier stage while its inflated tube ellipsoid fits, so the stage loop is sequential by definition).  A
// decomposition is a sequence of scans -- "keep the points that ..., and find the one closest to the ellipsoid
// centre in the ellipsoid's metric" -- where the reference rebuilds std::vectors:
//   * the first scan reads the whole cloud once (CR_UNROLL 64-point words in flight per wave) -- or, when the caller
//     supplies the uniform grid of frp_nmpc_cloud_grid_build, only the cell rows under the box's axis-aligned hull
//     (scan_grid, a separate kernel instantiation) --, tests the local box in the box's own frame, and appends the indices of the in-box points to a dense list in LDS (one LDS atomic
//     per CR_UNROLL words; the order of the list is irrelevant because minima are tie-broken by cloud index, which
//     is the reference's first-minimum rule on its order-preserving lists);
//   * every later scan runs over that list (typically 10 % of the cloud) with all lanes busy; point lists are bit
//     masks over list positions, one 64-bit word per 64 positions, produced by wave ballots; word g is always read
//     and written by the same wave, empty words are skipped 64 at a time with a ballot.  Boxes holding more than
//     CR_LIST points fall back to masks over the cloud itself;
//   * "filter with the new ellipsoid, then take the closest of what is left" uses the same distances, so both happen
//     in ONE scan; the workgroup minimum carries the winner's coordinates (one barrier, double-buffered);
//   * the 3x3 algebra of an ellipsoid update is wave-uniform: thread 0 does it and publishes the result through LDS
//     (struct Uni), so it costs the scanning waves no registers; the hyperplane of a cut is a dozen operations and
//     is computed by every lane from the winner the reduction hands out (no publish, no extra barrier).
// Memory-side work: 24 bytes per cloud point per decomposition, then 24-byte gathers of in-box points from L2 (the
// cloud is shared by the planners of a fleet); lists of up to CR_TILE * 256 points live in registers (scan_tile).
// Measured (profiles/r01_corridor_bench.json): first scan + list + register-tile fill 32 us on the plain cloud, 16 us
// through the uniform grid of frp_nmpc_cloud_grid_build (scan_grid), then ~20-30 scans of ~1.9 us per decomposition.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/frp_nmpc.h"

// Which point a round picks is decided by comparisons of nearly equal distances (after find_ellipsoid the obstacle points that shaped the
// ellipsoid sit at distance 1 +- 1 ulp), so every kernel of this file must compute the SAME bits from the same inputs.  Left to the
// compiler, a * b + c is fused or not depending on the code around it (round 5: the shell kernel visited two touching points in the other
// order -- same rows, swapped); hence no implicit contraction anywhere in this file, and the per-point expressions (metric distance,
// box frame projection, side of a cut) written once, with their fused multiply-adds spelled out.
#pragma clang fp contract(off)

#include "frp_corridor_scan.inc" // dot3 ... emit_row, BoxFrame / load_box / in_box / box_hull: shared with frp_corridor_large.hip

namespace frp {

// GRID = true: the first scan of every decomposition goes through the uniform grid; a planner that meets a box with more
// than CR_LIST points marks itself (poly_index[b][0] = -1) and leaves, and the GRID = false kernel launched right behind
// with only_flagged = 1 redoes just those planners from the plain cloud.  Two kernels instead of one with both first
// scans inlined: the combined one needs 256 VGPRs + 100 spilled SGPRs and loses the second resident workgroup per CU.
// CUT = true: the visibility cut of frp_nmpc_corridor_batch_cut in the first scan.  The cut travels behind the corridor in ONE kernel
// argument (CorridorArgs<true>); the uncut instantiations take the plain frp_nmpc_corridor as before and compile to the code they were.
template <bool GRID, bool CUT = false>
__global__ __launch_bounds__(CR_THREADS) __attribute__((amdgpu_waves_per_eu(FRP_CR_WPE, FRP_CR_WPE))) void corridor_kernel(CorridorArgs<CUT> args, int only_flagged)
{
    const frp_nmpc_corridor &c = corridor_of(args);
#ifdef FRP_CORRIDOR_PROFILE
    long long tp_check = 0, tp_init = 0, tp_cloud = 0, tp_lead = 0, tp_scan = 0, tp_emit = 0, tp_begin = wall_clock64();
    int np_scan = 0;
#endif
    extern __shared__ uint64_t s_mask[];
    __shared__ double s_A[FRP_CORRIDOR_MAX_F * 3], s_b[FRP_CORRIDOR_MAX_F];
    __shared__ Best s_red[2 * CR_WAVES];
    int phase = 0;
    __shared__ Uni u;
    const int b = blockIdx.x, tid = threadIdx.x;
    Scan sc;
    sc.Pn = c.cloud_count ? c.cloud_count[c.cloud_per_planner ? b : 0] : c.P;
    sc.Pn = sc.Pn < c.P ? sc.Pn : c.P;
    sc.W = (c.P + 63) / 64;
    sc.pts = c.cloud + (c.cloud_per_planner ? (size_t)b * c.P * 3 : 0);
    const int W_cloud = sc.W, P_cloud = sc.Pn;
    uint64_t *m0 = s_mask, *m1 = s_mask + sc.W, *m2 = s_mask + 2 * sc.W; // obs_, obs, working list
    uint32_t *list = reinterpret_cast<uint32_t *>(s_mask + 3 * sc.W);
    const double *ref = c.ref_pos + (size_t)b * c.N * 3, *yaw = c.ref_yaw + (size_t)b * c.N, *Eb = c.ellipsoid + (size_t)b * c.N * 9;
    const bool has_box = c.bbox[0] != 0.0 || c.bbox[1] != 0.0 || c.bbox[2] != 0.0;
    if (only_flagged && c.poly_index[(size_t)b * c.N] != -1) return; // (behind another kernel: only the planners it left flagged)
    CutBox cb = {};
    if (CUT) cb = load_cut(cut_of(args), b);
    int npoly = 0, rows = 0; // rows = stored rows of the last polytope (s_A / s_b)
    // Every round of the reference's while-loops removes at least the closest point, so a list is exhausted after at
    // most Pn rounds; the bound only matters for non-finite input, where the reference would spin forever.
    const int max_rounds = sc.Pn + 8;
    if (tid == 0) u.overflow = 0;

    for (int i = 0; i < c.N; ++i) {
        CR_T0
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
                CR_ACC(tp_check)
                continue;
            }
        }
        CR_ACC(tp_check)
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
            if (has_box) { // local box planes (line_segment.h:47-85)
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
        CR_ACC(tp_init)
        sc.list = nullptr; sc.W = W_cloud; sc.Pn = P_cloud;
        Best cp;
        if (GRID) {
            cp = scan_grid<CUT>(c, cb, list, u, s_red, phase);
            if (u.count > CR_LIST) { // more points in the box than the list holds: leave this planner to the plain-cloud kernel
                if (tid == 0) c.poly_index[(size_t)b * c.N] = -1;
                return;
            }
        } else
            cp = scan_cloud<CUT>(sc, m0, m1, m2, list, u, has_box, c.bbox, cb, s_red, phase);
        if (u.count <= CR_LIST) { // the usual case: from here on a position is an entry of the dense list
            sc.list = list; sc.Pn = u.count; sc.W = (u.count + 63) / 64;
            for (int g = tid >> 6; g < sc.W; g += CR_WAVES) {
                const int pos = g * 64 + (tid & 63);
                const bool valid = pos < sc.Pn;
                const uint64_t w0 = __ballot(valid), w1 = __ballot(valid && (list[valid ? pos : 0] >> 31));
                if ((tid & 63) == 0) { m0[g] = w0; m1[g] = w1; m2[g] = w1; }
            }
        }
        const bool tiled = u.count <= CR_TILE * CR_THREADS;
        Tile tile;
#pragma unroll
        for (int j = 0; j < CR_TILE; ++j) {
            const int pos = ((tid >> 6) + j * CR_WAVES) * 64 + (tid & 63);
            const bool valid = tiled && pos < sc.Pn;
            tile.id[j] = valid ? (int)(list[pos] & 0x7fffffffu) : 0;
            tile.x[j] = valid ? sc.pts[3 * (size_t)tile.id[j]] : 0.0;
            tile.y[j] = valid ? sc.pts[3 * (size_t)tile.id[j] + 1] : 0.0;
            tile.z[j] = valid ? sc.pts[3 * (size_t)tile.id[j] + 2] : 0.0;
            tile.d2[j] = 0.0;
        }
        CR_ACC(tp_cloud)
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
            CR_ACC(tp_lead)
            cp = tiled ? scan_tile<KEEP_OUTSIDE>(tile, sc.W, m2, m2, u, s_red, phase) : scan<KEEP_OUTSIDE>(sc, m2, m2, u, s_red, phase);
            CR_ACC(tp_scan) CR_CNT(np_scan)
        }
        // third axis (line_segment.h:183-208)
        if (tid == 0) st3(u.Ci, inverse(rot_diag_rot(ld3(u.Rf), u.ax[0], u.ax[1], u.ax[2])));
        __syncthreads();
        CR_ACC(tp_lead)
        cp = tiled ? scan_tile<KEEP_INSIDE>(tile, sc.W, m1, m2, u, s_red, phase) : scan<KEEP_INSIDE>(sc, m1, m2, u, s_red, phase);
        CR_ACC(tp_scan) CR_CNT(np_scan)
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
            CR_ACC(tp_lead)
            cp = tiled ? scan_tile<KEEP_OUTSIDE>(tile, sc.W, m2, m2, u, s_red, phase) : scan<KEEP_OUTSIDE>(sc, m2, m2, u, s_red, phase);
            CR_ACC(tp_scan) CR_CNT(np_scan)
        }
        // hyperplanes (decomp_base.h:63-83) + LinearConstraint rows (polyhedron.h:98-118)
        double *gA = c.poly_A + (((size_t)b * c.N + npoly) * c.F) * 3, *gb = c.poly_b + ((size_t)b * c.N + npoly) * c.F;
        if (tid == 0) {
            const M3 Ci = ld3(u.Ci);
            st3(u.CC, mul(Ci, transpose(Ci))); // C^-1 C^-T (ellipsoid.h:53-58)
            u.rows = 0;
        }
        CR_ACC(tp_lead)
        cp = tiled ? scan_tile<KEEP_ALL>(tile, sc.W, m0, m2, u, s_red, phase) : scan<KEEP_ALL>(sc, m0, m2, u, s_red, phase); // Ci is unchanged since the last barrier
        CR_ACC(tp_scan) CR_CNT(np_scan)
        for (int guard = 0; cp.idx != 0x7fffffff && guard < max_rounds; ++guard) {
            // closest_hyperplane (ellipsoid.h:53-58) by every lane from the winner the reduction handed out: no
            // publish-through-LDS, hence no barrier between "pick" and "cut"
            const double q[3] = {cp.x, cp.y, cp.z};
            const double w[3] = {q[0] - u.mid[0], q[1] - u.mid[1], q[2] - u.mid[2]};
            double n[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) n[k] = u.CC[3 * k] * w[0] + u.CC[3 * k + 1] * w[1] + u.CC[3 * k + 2] * w[2];
            const double nl = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) n[k] /= nl;
            if (tid == 0) emit_row(u, q, n, c.F, s_A, s_b, gA, gb);
            CR_ACC(tp_lead)
            cp = tiled ? scan_tile<KEEP_BEHIND_PLANE>(tile, sc.W, m2, m2, u, s_red, phase, q, n) : scan<KEEP_BEHIND_PLANE>(sc, m2, m2, u, s_red, phase, q, n);
            CR_ACC(tp_scan) CR_CNT(np_scan)
        }
        if (tid == 0) {
            if (has_box)
                for (int k = 0; k < 6; ++k) emit_row(u, u.box[k], u.box[6 + k], c.F, s_A, s_b, gA, gb);
            c.poly_nfaces[(size_t)b * c.N + npoly] = u.rows;
            c.poly_index[(size_t)b * c.N + i] = npoly;
        }
        __syncthreads(); // rows of the new polytope visible to the containment check of the next stage
        CR_ACC(tp_emit)
        rows = u.rows < c.F ? u.rows : c.F;
        ++npoly;
    }
#ifdef FRP_CORRIDOR_PROFILE
    if (tid == 0 && (b == 0 || b == 1000)) {
        printf("scan body %lld reduce %lld (all WGs thread 0)\n", g_prof[0], g_prof[1]);
        printf("corridor wg %d: total %lld check %lld init %lld cloud %lld lead %lld scan %lld (%d scans) emit %lld [100 MHz ticks], %d polytopes\n", b,
               wall_clock64() - tp_begin, tp_check, tp_init, tp_cloud, tp_lead, tp_scan, np_scan, tp_emit, npoly);
    }
#endif
    if (tid == 0) {
        for (int k = npoly; k < c.N; ++k) c.poly_nfaces[(size_t)b * c.N + k] = 0;
        if (c.poly_count) c.poly_count[b] = u.overflow ? -npoly : npoly; // (overflow = a polytope was truncated, so npoly >= 1 and the sign is never lost)
    }
}


// ================================================================== one wavefront per planner (round 4), boxes of any size (round 5)
// A decomposition is a chain of ~20 dependent rounds (pick the closest point, cut, filter), each a few hundred instructions: with four
// wavefronts per planner a round pays a workgroup barrier, an LDS exchange of the per-wave minima and the latency of everything in
// between, and the CU holds 3 planners (12 waves at the 168-register budget).  Measured on the full-tick workload (4096 planners,
// 18 k points, ~1000 of them in a local box): per planner and tick 58 us in 42 scans, 33 us in the two first scans, 25 us between
// scans, 15 us in 20 containment checks -- all latency; two waves per planner (6 per CU) already ran 0.90 -> 0.76 ms.  This kernel
// gives a planner ONE wavefront, so nothing in a round crosses a wave:
//   * the points a round looks at live in the wave's registers, CW_TILE points per lane; the point sets (obs_, obs, the working set) are
//     one bit per point in three 32-bit registers PER LANE -- no LDS masks, no ballots to store them, empty tile rows are skipped;
//   * the closest point of a round is a DPP minimum and six v_readlane: no barrier, no LDS;
//   * the hyperplane loop (decomp_base.h:63-83) compares distances in a FIXED ellipsoid: they are computed once by its opening scan;
//   * the containment checks of the stages behind a new polytope (nmpc_solver.cpp:291-313) are evaluated together, lane = stage, the
//     rows read from LDS: one global round trip per polytope instead of one per stage.
// The wave-uniform 3x3 algebra stays on lane 0 behind LDS (struct Uni) exactly as in the four-wave kernel -- same instructions, same
// results: the kernels produce bit-identical polytopes (tests/test_gpu_parity.py::_check_corridor compares every grid launch -- this
// kernel -- with the plain-cloud launch of the workgroup kernel, array for array).
// Round 4 held the WHOLE box in the tile (20 rows = 1280 points at 256 registers, 2 waves per SIMD = 8 planners per CU: 0.90 -> 0.40 ms
// for the tick's corridor; boxes beyond the tile went back to the workgroup kernels: 4.13 / 11.6 ms on the 19 k / 62 k-point clouds of
// tests/tools/corridor_bench.py).  Round 5: a decomposition never needs its box all at once --
//   * find_ellipsoid (line_segment.h:136-211) only looks at the points inside the SEED ellipsoid: pass A streams the grid rows under the
//     box's hull, counts the in-box points and lists just those (more than the tile holds: the planner is flagged, poly_index[b][0] =
//     -1, for the workgroup kernels launched behind) -- and, betting that there are none, the first shell of the next step too;
//   * find_polyhedron (decomp_base.h:63-83) visits the in-box points in order of their distance in the final ellipsoid, and every cut
//     removes what lies behind it.  So the points are taken in SHELLS of that distance: pass B streams the hull again and lists the
//     points with T_lo <= d2 < T_hi that are in front of every plane cut so far (the planes sit in LDS; the test is the scan's own
//     expression, and a point is alive iff it is in front of ALL planes, whatever the order they are tried in); the tile runs the
//     reference's loop on them until none is left, and since every point outside the shell is farther than every point inside, the
//     closest alive point of the shell IS the closest alive point.  The first shell is sized for 3/8 of a tile (from the count the previous decomposition's shell
//     held; the cloud's mean density for a planner's first box); behind it nearly everything is already cut, so the next shell is tried unbounded and narrowed only if it overflows.
//   Same picks, same cuts, same rows (tests/test_gpu_parity.py::test_corridor_dense_clouds_boxes_beyond_the_register_tile).
// -- and with the box out of the registers the tile can be SMALL: a wavefront's rounds are a dependent chain (one wave per SIMD instead
// of two: the same 87 us per planner and tick), so what counts is wavefronts in flight.  Measured, every planner through this form
// (19 k cloud / 62 k cloud / the tick's corridor, ms; tools/dbg/corridor_allshell.sh): 20 rows at 2 waves per SIMD 1.84 / 3.16 / 0.447,
// 16 rows 1.74 / 2.99 / 0.427, 12 rows at 3 waves (108 spilled registers) 1.76 / 3.01 / 0.459, 8 rows at 4 waves 1.48 / 2.69 / 0.369 --
// with 9 KB of LDS per planner (64 cuts kept, a one-row packing buffer) so that sixteen planners fit a CU 1.43 / 2.61 / 0.339, and with
// the stream two words deep instead of eight (fewer registers in the passes) 1.23 / 2.16 / 0.293 (6 rows at 5 waves: 1.63 / 4.11 /
// 0.395); the rows of the cuts made after the loop, lane = cut, instead of by lane 0 inside every round 1.20 / 2.11 / 0.284; 7 rows and
// shells sized for 5/8 of a tile 1.18 / 2.08 / 0.280; pass A reading only the cells under its first shell (whose bound follows the previous
// decomposition's count) 1.05 / 1.40 / 0.270, and with that a first shell of 3/8 of a tile **0.97 / 1.46 / 0.254**
// (profiles/r05_corridor_knobs.txt).  That is the shipped configuration; the round-4 form (whole box, 20 rows) is gone: 1.89 / 3.22 /
// 0.385 with it in front.
// Needs the uniform grid and the local box (the production configuration).  What this kernel gives up on -- more than a tile of points
// inside the seed ellipsoid, more than CS_PLANES cuts, a shell it cannot narrow -- it flags for the workgroup kernels.
#ifndef FRP_CW_TILE
#define FRP_CW_TILE 7
#endif
#ifndef FRP_CW_WPE
#define FRP_CW_WPE 4
#endif
#ifndef FRP_CW_PACK   // experiment knob: 0 = the survivors of the cuts stay in the tile rows they were listed in
#define FRP_CW_PACK 1
#endif
#ifndef FRP_CW_D2   // experiment knob: 0 = recompute the hyperplane loop's distances every round (one register pair per tile row fewer)
#define FRP_CW_D2 1
#endif
constexpr int CW_TILE = FRP_CW_TILE, CW_CAP = 64 * CW_TILE;
static_assert(CW_TILE <= 32, "one bit per tile row in a 32-bit lane mask");
struct TileW { double x[CW_TILE], y[CW_TILE], z[CW_TILE], d2[FRP_CW_D2 ? CW_TILE : 1]; int id[CW_TILE]; };

#define CW_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

__device__ __forceinline__ double readlane_f64(double v, int l)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l) << 32) |
                                            (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l)));
}
// the wave's minimum in (distance, cloud index) order, uniform in every lane; idx = INT_MAX when no lane had a point
__device__ __forceinline__ Best wave_best(const Best &mine)
{
    const double d = wave_min_f64(mine.dist);
    uint64_t own = __ballot(mine.dist == d && mine.idx != 0x7fffffff);
    if (own == 0) return Best{1.7976931348623157e308, 0x7fffffff, 0.0, 0.0, 0.0};
    if (own & (own - 1)) { // equal distances: the smaller cloud index (the reference's first minimum on its order-preserving lists)
        const int i = wave_min_i32(mine.dist == d ? mine.idx : 0x7fffffff);
        own = __ballot(mine.dist == d && mine.idx == i);
    }
    const int l = __builtin_ctzll(own);
    Best r;
    r.dist = d; r.idx = __builtin_amdgcn_readlane(mine.idx, l);
    r.x = readlane_f64(mine.x, l); r.y = readlane_f64(mine.y, l); r.z = readlane_f64(mine.z, l);
    return r;
}

template <int MODE>
__device__ __forceinline__ Best scan_wave(TileW &t, int W, unsigned in, unsigned &out, const Uni &u, const double *pq = nullptr, const double *pn = nullptr,
                                          int *kept = nullptr)
{
    const M3 Ci = ld3(u.Ci);
    const double d[3] = {u.mid[0], u.mid[1], u.mid[2]};
    double q[3] = {0, 0, 0}, n[3] = {0, 0, 0};
    if (MODE == KEEP_BEHIND_PLANE) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { q[k] = pq[k]; n[k] = pn[k]; }
    }
    Best best{1.7976931348623157e308, 0x7fffffff, 0.0, 0.0, 0.0};
    unsigned o = 0;
    int nk = 0;
#pragma unroll
    for (int j = 0; j < CW_TILE; ++j) {
        if (j < W) {
            bool alive = (in >> j) & 1u;
            if (__ballot(alive) != 0) { // (wave-uniform: a tile row with no member is skipped)
                if (alive) {
                    const double dist = (MODE == KEEP_BEHIND_PLANE && FRP_CW_D2) ? t.d2[FRP_CW_D2 ? j : 0] : ell_dist2(Ci, d, t.x[j], t.y[j], t.z[j]);
                    if (MODE == KEEP_ALL && FRP_CW_D2) t.d2[FRP_CW_D2 ? j : 0] = dist;
                    if (MODE == KEEP_OUTSIDE) alive = 1 - sqrt(dist) > CR_EPS;
                    if (MODE == KEEP_INSIDE) alive = dist <= 1;
                    if (MODE == KEEP_BEHIND_PLANE) alive = cut_side(n, q, t.x[j], t.y[j], t.z[j]) < 0;
                    if (alive && before(dist, t.id[j], best.dist, best.idx)) best = Best{dist, t.id[j], t.x[j], t.y[j], t.z[j]};
                }
                o |= (alive ? 1u : 0u) << j;
                if (kept) nk += (int)__popcll(__ballot(alive));
            }
        }
    }
    out = o;
    if (kept) *kept = nk;
    return wave_best(best);
}

#ifndef FRP_CS_FILL // eighths of a tile a shell is sized for (3: since pass A reads only the cells under its shell a smaller one pays -- profiles/r05_corridor_knobs.txt)
#define FRP_CS_FILL 3
#endif
#ifndef FRP_CS_FMAX // the most a first shell's bound grows from one decomposition to the next
#define FRP_CS_FMAX 1.6
#endif
#ifndef FRP_CS_PLANES
#define FRP_CS_PLANES 64
#endif
constexpr int CS_PLANES = FRP_CS_PLANES; // cuts of one decomposition kept for the later shells (more: the planner is left to the workgroup kernels)
constexpr int CS_RETRIES = 48;

// (BoxFrame, load_box, in_box, box_hull: the local box as the first scans test it, and its hull in grid cells -- frp_corridor_scan.inc)

// every point of the cell-sorted cloud under the hull [lo, hi] of a local box.  The grid rows under the hull (cells lo[0]..hi[0] of one
// (iy, iz): one contiguous run of the sorted points each) are laid end to end -- lane = row fetches its run, a wave scan gives the run
// offsets, a lane finds the run of its flat position by a 6-step search in LDS -- so every wavefront-wide load is full whatever the
// runs' lengths, CS_U of them are in flight, and the next batch is fetched before the current one is looked at (a pass is a chain of
// L2 round trips: 2500 .. 8000 candidates per pass, ~1.5x the in-box points).  f(batch, chunks) is called in uniform control flow with
// the first `chunks` 64-point words of the batch live (id < 0: no point in this lane) and returns false (uniformly) to stop the pass.
// s_row: 128 ints of LDS.
#ifndef FRP_CS_U
#define FRP_CS_U 2
#endif
constexpr int CS_U = FRP_CS_U;
struct HullBatch { double x[CS_U], y[CS_U], z[CS_U]; int id[CS_U]; };

// Before a row is read it is clipped: its cells form a box [x range] x [one cell in y] x [one cell in z] (border cells, which also hold
// the points outside the grid, count as unbounded on their outer side), and a point can only matter if it is on the keep side of every
// plane in s_cuts[0 .. ncuts) -- the six faces of the local box pushed out by a micrometre, then the cuts made so far -- so per plane the
// row keeps just the x range in which SOME point of its y-z cross-section is on the keep side (bounds rounded outward; the exact tests
// are still made per point).  The hull of a rotated box loses a third of its cells this way, the pass behind a finished shell four
// fifths: what is alive by then lies inside the polytope under construction.
template <class Fn>
__device__ __forceinline__ void stream_hull(const frp_nmpc_corridor &c, const int (&lo)[3], const int (&hi)[3], int *s_row, const double *s_cuts, int ncuts, Fn &&f)
{
    const int lane = threadIdx.x;
    const int ny = hi[1] - lo[1] + 1, rows = ny * (hi[2] - lo[2] + 1), nx = c.grid_dims[0];
    const double inf = __builtin_huge_val();
    for (int rb = 0; rb < rows; rb += 64) {
        int mbeg = 0, run = 0;
        if (rb + lane < rows) {
            const int r = rb + lane;
            const int iy = lo[1] + r % ny, iz = lo[2] + r / ny;
            const double ylo = iy == 0 ? -inf : c.grid_origin[1] + iy * c.grid_cell, yhi = iy == c.grid_dims[1] - 1 ? inf : c.grid_origin[1] + (iy + 1) * c.grid_cell;
            const double zlo = iz == 0 ? -inf : c.grid_origin[2] + iz * c.grid_cell, zhi = iz == c.grid_dims[2] - 1 ? inf : c.grid_origin[2] + (iz + 1) * c.grid_cell;
            double xlo = -inf, xhi = inf;
            for (int p = 0; p < ncuts; ++p) {
                const double *pl = s_cuts + 6 * p;
                const double n0 = pl[3], n1 = pl[4], n2 = pl[5];
                // the least n1 (y - q1) + n2 (z - q2) over the cross-section: a point (x, y, z) is kept only if n0 (x - q0) + that < 0
                const double ry = n1 > 0 ? n1 * (ylo - pl[1]) : (n1 < 0 ? n1 * (yhi - pl[1]) : 0.0), rz = n2 > 0 ? n2 * (zlo - pl[2]) : (n2 < 0 ? n2 * (zhi - pl[2]) : 0.0);
                const double rmin = ry + rz;
                if (n0 != 0.0) {
                    const double off = -rmin * __builtin_amdgcn_rcp(n0), bnd = pl[0] + off, mg = 1e-6 + 1e-6 * fabs(off);
                    if (n0 > 0) { if (bnd + mg < xhi) xhi = bnd + mg; } else { if (bnd - mg > xlo) xlo = bnd - mg; }
                } else if (rmin > 1e-6)
                    xlo = inf;
            }
            if (xlo <= xhi) {
                // the cells of [xlo, xhi] the way the grid bins a coordinate: clamped to the grid -- a bound outside the grid still meets the
                // border cell, which holds the points out there (tests: test_corridor_grid_smaller_than_the_cloud_and_other_edges) -- then to the hull
                const double a = floor((xlo - c.grid_origin[0]) / c.grid_cell), bb = floor((xhi - c.grid_origin[0]) / c.grid_cell);
                int ia = a < 0 ? 0 : (a > nx - 1 ? nx - 1 : (int)a), ib = bb < 0 ? 0 : (bb > nx - 1 ? nx - 1 : (int)bb);
                ia = ia > lo[0] ? ia : lo[0]; ib = ib < hi[0] ? ib : hi[0];
                if (ia <= ib) {
                    const size_t row = ((size_t)iz * c.grid_dims[1] + iy) * nx;
                    mbeg = c.grid_start[row + ia];
                    run = c.grid_start[row + ib + 1] - mbeg;
                }
            }
        }
        int inc = run;
#pragma unroll
        for (int dl = 1; dl < 64; dl <<= 1) { const int v = __shfl_up(inc, dl); if (lane >= dl) inc += v; }
        const int total = __builtin_amdgcn_readlane(inc, 63);
        CW_SYNC(); // (the previous block's searches are done)
        s_row[lane] = inc - run; s_row[64 + lane] = mbeg; // rows past the last one have an empty run: their offset is `total`, beyond every position
        CW_SYNC();
        if (total == 0) continue;
        // (no branch in here: positions past the end are clamped to the last point, so the CS_U searches advance in lock step -- one LDS
        // round trip per step, not per step and load -- and the loads of a batch are issued back to back)
        auto fetch = [&](int t0, HullBatch &B) {
            int t[CS_U], r[CS_U];
#pragma unroll
            for (int k = 0; k < CS_U; ++k) { const int tt = t0 + 64 * k + lane; t[k] = tt < total ? tt : total - 1; r[k] = 0; }
#pragma unroll
            for (int step = 32; step; step >>= 1) { // the last run that starts at or before t (never an empty one)
                int v[CS_U];
#pragma unroll
                for (int k = 0; k < CS_U; ++k) v[k] = s_row[r[k] + step];
#pragma unroll
                for (int k = 0; k < CS_U; ++k) r[k] += v[k] <= t[k] ? step : 0;
            }
            int p[CS_U];
#pragma unroll
            for (int k = 0; k < CS_U; ++k) p[k] = s_row[64 + r[k]] + (t[k] - s_row[r[k]]);
#pragma unroll
            for (int k = 0; k < CS_U; ++k) {
                const size_t p3 = 3 * (size_t)p[k];
                B.x[k] = c.grid_points[p3]; B.y[k] = c.grid_points[p3 + 1]; B.z[k] = c.grid_points[p3 + 2];
                B.id[k] = c.grid_index[p[k]];
            }
#pragma unroll
            for (int k = 0; k < CS_U; ++k) B.id[k] = t0 + 64 * k + lane < total ? B.id[k] : -1;
        };
        HullBatch cur, nxt;
        fetch(0, cur);
        for (int t0 = 0; t0 < total; t0 += 64 * CS_U) {
            const bool has_next = t0 + 64 * CS_U < total;
            if (has_next) fetch(t0 + 64 * CS_U, nxt);
            const int left = (total - t0 + 63) / 64;
            if (!f(cur, left < CS_U ? left : CS_U)) return;
            if (has_next) cur = nxt;
        }
    }
}

// The points a cut leaves alive are scattered over all the tile rows they were listed in (a thousand points: after five cuts a hundred
// are left, in seven rows of sixteen on average -- and a round costs its live ROWS).  Once no more than CW_PACK are alive they are moved
// to the first rows, through LDS (the list's space: it has been read by then), and the rounds behind visit two rows.  Which lane holds a
// point does not matter to any result: minima are taken in (distance, cloud index) order.
#ifndef FRP_CW_PACKN
#define FRP_CW_PACKN 64
#endif
constexpr int CW_PACK = FRP_CW_PACKN;
constexpr int CW_LIST = CW_CAP > CW_PACK * 9 ? CW_CAP : CW_PACK * 9; // entries of the in-box list; also the packing buffer (36 bytes per packed point)
static_assert(CW_PACK % 64 == 0, "whole tile rows");
__device__ __forceinline__ void pack_tile(TileW &t, unsigned &m, int &W, int alive, uint32_t *buf)
{
    const int lane = threadIdx.x;
    double *bx = reinterpret_cast<double *>(buf), *by = bx + CW_PACK, *bz = by + CW_PACK, *bd = bz + CW_PACK;
    int *bi = reinterpret_cast<int *>(bd + CW_PACK);
    const int c = __popc(m);
    int inc = c;
#pragma unroll
    for (int dl = 1; dl < 64; dl <<= 1) { const int v = __shfl_up(inc, dl); if (lane >= dl) inc += v; }
    int slot = inc - c;
#pragma unroll
    for (int j = 0; j < CW_TILE; ++j) {
        if (j < W && ((m >> j) & 1u)) {
            bx[slot] = t.x[j]; by[slot] = t.y[j]; bz[slot] = t.z[j]; bd[slot] = t.d2[FRP_CW_D2 ? j : 0]; bi[slot] = t.id[j];
            ++slot;
        }
    }
    CW_SYNC();
    unsigned o = 0;
#pragma unroll
    for (int j = 0; j < CW_PACK / 64; ++j) {
        const int pos = j * 64 + lane;
        const bool valid = pos < alive;
        t.x[j] = valid ? bx[pos] : 0.0; t.y[j] = valid ? by[pos] : 0.0; t.z[j] = valid ? bz[pos] : 0.0;
        t.d2[FRP_CW_D2 ? j : 0] = valid ? bd[pos] : 0.0; t.id[j] = valid ? bi[pos] : 0;
        o |= (valid ? 1u : 0u) << j;
    }
    CW_SYNC();
    m = o; W = CW_PACK / 64;
}

// The kernel's text is frp_corridor_wave.inc (see there why it is included and not a template): once as it always was, once with the
// visibility cut of frp_nmpc_corridor_batch_cut in both passes' "in the local box" test.
#define CW_KERNEL corridor_wave_kernel(frp_nmpc_corridor c)
#define CW_PROLOGUE
#define CW_AND_SEEN(x, y, z)
#include "frp_corridor_wave.inc"
#undef CW_KERNEL
#undef CW_PROLOGUE
#undef CW_AND_SEEN
#define CW_KERNEL corridor_wave_cut_kernel(CorridorCutArgs args)
#define CW_PROLOGUE const frp_nmpc_corridor &c = args.c; const CutBox cb = load_cut(args.cut, blockIdx.x);
#define CW_AND_SEEN(x, y, z) && cut_sees<true>(cb, x, y, z)
#include "frp_corridor_wave.inc"
#undef CW_KERNEL
#undef CW_PROLOGUE
#undef CW_AND_SEEN

} // namespace frp

namespace frp {

__device__ __forceinline__ int grid_cell_of(const double *pt, const double *origin, double cell, const int *dims)
{
    int ix[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a = floor((pt[k] - origin[k]) / cell);
        ix[k] = !(a > 0) ? 0 : (a > dims[k] - 1 ? dims[k] - 1 : (int)a); // NaN and points beyond the grid go to border cells
    }
    return (ix[2] * dims[1] + ix[1]) * dims[0] + ix[0];
}

struct GridArgs { const double *cloud; int P; double origin[3]; double cell; int dims[3]; double *points; int *index; int *start; int *cursor; };

__global__ void grid_zero_kernel(GridArgs g, int cells)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= cells; i += gridDim.x * blockDim.x) { g.start[i] = 0; if (i < cells) g.cursor[i] = 0; }
}
__global__ void grid_count_kernel(GridArgs g)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < g.P; i += gridDim.x * blockDim.x)
        atomicAdd(&g.start[grid_cell_of(g.cloud + 3 * (size_t)i, g.origin, g.cell, g.dims) + 1], 1);
}
// inclusive prefix sum of start[1..cells] in place, one workgroup walking the array in 1024-element chunks
__global__ __launch_bounds__(1024) void grid_scan_kernel(GridArgs g, int cells)
{
    __shared__ int s_part[16], s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int base = 1; base <= cells; base += 1024) {
        const int i = base + tid;
        int v = i <= cells ? g.start[i] : 0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(v, off); if (lane >= off) v += t; }
        if (lane == 63) s_part[wave] = v;
        __syncthreads();
        int add = s_carry;
        for (int w = 0; w < wave; ++w) add += s_part[w];
        if (i <= cells) g.start[i] = v + add;
        __syncthreads();
        if (tid == 1023) s_carry = v + add;
        __syncthreads();
    }
}
__global__ void grid_scatter_kernel(GridArgs g)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < g.P; i += gridDim.x * blockDim.x) {
        const double *pt = g.cloud + 3 * (size_t)i;
        const int cell = grid_cell_of(pt, g.origin, g.cell, g.dims);
        const int at = g.start[cell] + atomicAdd(&g.cursor[cell], 1); // order inside a cell is irrelevant (ties go by cloud index)
        g.points[3 * (size_t)at] = pt[0]; g.points[3 * (size_t)at + 1] = pt[1]; g.points[3 * (size_t)at + 2] = pt[2];
        g.index[at] = i;
    }
}

} // namespace frp

extern "C" int frp_nmpc_cloud_grid_build(const double *cloud, int P, const double origin[3], double cell, const int dims[3],
                                         double *grid_points, int *grid_index, int *grid_start, int *scratch, void *stream)
{
    if (P < 0 || (P > 0 && !cloud) || !origin || !dims || !(cell > 0.0) || !grid_points || !grid_index || !grid_start || !scratch) return FRP_ERR_ARG;
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || (long long)dims[0] * dims[1] * dims[2] > FRP_CORRIDOR_MAX_CELLS) return FRP_ERR_ARG;
    const int cells = dims[0] * dims[1] * dims[2];
    frp::GridArgs g = {cloud, P, {origin[0], origin[1], origin[2]}, cell, {dims[0], dims[1], dims[2]}, grid_points, grid_index, grid_start, scratch};
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(frp::grid_zero_kernel, dim3(256), dim3(256), 0, st, g, cells);
    if (P > 0) hipLaunchKernelGGL(frp::grid_count_kernel, dim3(256), dim3(256), 0, st, g);
    hipLaunchKernelGGL(frp::grid_scan_kernel, dim3(1), dim3(1024), 0, st, g, cells);
    if (P > 0) hipLaunchKernelGGL(frp::grid_scatter_kernel, dim3(256), dim3(256), 0, st, g);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

// FRP_CORRIDOR_WAVE=0 (experiments): workgroup kernels only
static bool corridor_wave_off()
{
    static const bool off = [] { const char *e = getenv("FRP_CORRIDOR_WAVE"); return e && e[0] == '0'; }();
    return off;
}

bool frp::corridor_args_ok(const frp_nmpc_corridor *p, const frp_nmpc_corridor_cut *cut, int max_points)
{
    if (!p || p->B <= 0 || p->N < 1 || p->N > 64 || p->F < 6 || p->F > FRP_CORRIDOR_MAX_F || p->P < 0 || p->P > max_points ||
        (p->P > 0 && !p->cloud) || !p->ref_pos || !p->ref_yaw || !p->ellipsoid || !p->poly_A || !p->poly_b || !p->poly_nfaces || !p->poly_index)
        return false;
    if (!(p->seed_len > 0.0) || !(p->inflation >= 0.0)) return false;
    if (!(p->offset_x > -0.5 * p->seed_len)) return false; // at or below, the seed ellipsoid's matrix is singular or negative and find_ellipsoid's loops do not end
    if (p->grid_start && (!p->grid_points || !p->grid_index || !(p->grid_cell > 0.0) || p->grid_dims[0] < 1 || p->grid_dims[1] < 1 || p->grid_dims[2] < 1 ||
                          p->cloud_per_planner))
        return false;
    if (cut && (!cut->box || !(cut->resolution > 0.0) || !__builtin_isfinite(cut->resolution) || !__builtin_isfinite(cut->origin[0]) ||
                !__builtin_isfinite(cut->origin[1]) || !__builtin_isfinite(cut->origin[2]) || p->cloud_per_planner))
        return false;
    return true;
}

// frp_corridor_large.hip.  The grid kernel lays its three masks and the list out from P (m1 = s_mask + ceil(P / 64), ...), but behind its
// first scan it either leaves (more than CR_LIST points in the box: the planner stays flagged) or works on LIST positions only: sc.Pn =
// u.count <= CR_LIST, sc.W = ceil(u.count / 64), and scan<> / scan_tile / the mask fill index m0 / m1 / m2 by g < sc.W alone; the cloud
// is reached through list entries (sc.pts[3 * id], a size_t offset).  P itself enters only that layout and max_rounds = min(count, P) + 8.
// So the kernel is handed the same corridor with P = min(P, CR_LIST): masks over CR_LIST positions (3 KB) + the list (32 KB) whatever
// the cloud holds, and max_rounds >= u.count + 8 still (u.count <= CR_LIST and u.count <= the live count), which is all a finite input
// needs.  The one-wavefront kernel takes P as it is (its first density guess and its own round bound; it has no masks).
void frp::corridor_launch_listed(const frp_nmpc_corridor *p, const frp_nmpc_corridor_cut *cut, hipStream_t st)
{
    const bool wave = !corridor_wave_off();
    frp_nmpc_corridor listed = *p;
    listed.P = p->P < frp::CR_LIST ? p->P : frp::CR_LIST;
    const size_t lds = (size_t)3 * ((listed.P + 63) / 64) * sizeof(uint64_t) + frp::CR_LIST * sizeof(uint32_t);
    if (cut) {
        const frp::CorridorCutArgs a = {*p, *cut}, al = {listed, *cut};
        if (wave) hipLaunchKernelGGL(frp::corridor_wave_cut_kernel, dim3((unsigned)p->B), dim3(64), 0, st, a);
        hipLaunchKernelGGL((frp::corridor_kernel<true, true>), dim3((unsigned)p->B), dim3(frp::CR_THREADS), lds, st, al, wave ? 1 : 0);
        return;
    }
    if (wave) hipLaunchKernelGGL(frp::corridor_wave_kernel, dim3((unsigned)p->B), dim3(64), 0, st, *p);
    hipLaunchKernelGGL(frp::corridor_kernel<true>, dim3((unsigned)p->B), dim3(frp::CR_THREADS), lds, st, listed, wave ? 1 : 0);
}

// counted_grid (frp_nmpc_corridor_batch_view): the caller asserts that the grid was built for exactly cloud_count[0] points, so a count
// does not turn it off; P is then the capacity of the buffers (the kernels clamp the point count to the count, the one-wavefront
// kernel reads points through the grid alone)
static int corridor_launch(const frp_nmpc_corridor *p, const frp_nmpc_corridor_cut *cut, void *stream, bool counted_grid = false)
{
    if (!frp::corridor_args_ok(p, cut, FRP_CORRIDOR_MAX_POINTS)) return FRP_ERR_ARG;
    const size_t lds = (size_t)3 * ((p->P + 63) / 64) * sizeof(uint64_t) + frp::CR_LIST * sizeof(uint32_t);
    const bool has_box = p->bbox[0] != 0.0 || p->bbox[1] != 0.0 || p->bbox[2] != 0.0;
    const bool grid = p->grid_start && has_box && (counted_grid || !p->cloud_count);
    // production configuration (shared cloud with a grid, local box, N <= 64 = one lane per stage): one wavefront per planner;
    // planners it flags (more than a tile of points inside a seed ellipsoid, more than CS_PLANES cuts) go to the workgroup kernel
    // through the grid, and what THAT one flags (more in-box points than its LDS list) to the plain-cloud kernel.
    const bool wave = grid && !corridor_wave_off();
    if (cut) { // the same chain, the cut carried through all three launches
        hipStream_t st = static_cast<hipStream_t>(stream);
        const frp::CorridorCutArgs a = {*p, *cut};
        if (wave) hipLaunchKernelGGL(frp::corridor_wave_cut_kernel, dim3((unsigned)p->B), dim3(64), 0, st, a);
        if (grid) hipLaunchKernelGGL((frp::corridor_kernel<true, true>), dim3((unsigned)p->B), dim3(frp::CR_THREADS), lds, st, a, wave ? 1 : 0);
        hipLaunchKernelGGL((frp::corridor_kernel<false, true>), dim3((unsigned)p->B), dim3(frp::CR_THREADS), lds, st, a, grid ? 1 : 0);
        return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
    }
    if (wave) hipLaunchKernelGGL(frp::corridor_wave_kernel, dim3((unsigned)p->B), dim3(64), 0, static_cast<hipStream_t>(stream), *p);
    if (grid) hipLaunchKernelGGL(frp::corridor_kernel<true>, dim3((unsigned)p->B), dim3(frp::CR_THREADS), lds, static_cast<hipStream_t>(stream), *p, wave ? 1 : 0);
    hipLaunchKernelGGL(frp::corridor_kernel<false>, dim3((unsigned)p->B), dim3(frp::CR_THREADS), lds, static_cast<hipStream_t>(stream), *p, grid ? 1 : 0);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

extern "C" int frp_nmpc_corridor_batch(const frp_nmpc_corridor *p, void *stream) { return corridor_launch(p, nullptr, stream); }

extern "C" int frp_nmpc_corridor_batch_cut(const frp_nmpc_corridor *p, const frp_nmpc_corridor_cut *cut, void *stream)
{
    return corridor_launch(p, cut, stream);
}

// include/frp_nmpc_occmap_view.h: the same chain for the device-built shared view -- a device-side count AND the grid
extern "C" int frp_nmpc_corridor_batch_view(const frp_nmpc_corridor *p, const frp_nmpc_corridor_cut *cut, void *stream)
{
    if (!p || !p->cloud_count || p->cloud_per_planner) return FRP_ERR_ARG;
    return corridor_launch(p, cut, stream, true);
}
