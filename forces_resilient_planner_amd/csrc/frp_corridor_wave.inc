// frp_corridor_wave.inc -- the body of the one-wavefront corridor kernel, included by frp_corridor.hip once per variant:
//   CW_KERNEL(name and parameters)  CW_PROLOGUE (declares `c`, and the cut's bounds `cb` in the cut variant)  CW_AND_SEEN(x, y, z)
// The kernel sits at its 128-register cap with 60 spilled, and its code is sensitive to everything around it: as a template over
// the cut (or as a shared inlined body) the UNCUT kernel came out with another schedule and another spill count.  Textual inclusion
// keeps the uncut kernel's tokens what they were -- it compiles to the same instructions as before the cut existed.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(FRP_CW_WPE, FRP_CW_WPE))) void CW_KERNEL
{
    CW_PROLOGUE
    __shared__ double s_A[FRP_CORRIDOR_MAX_F * 3], s_b[FRP_CORRIDOR_MAX_F];
    __shared__ uint32_t list[CW_LIST];
    __shared__ Uni u;
    __shared__ double s_pl[(6 + CS_PLANES) * 6]; // the local box's faces (pushed out, for the row clipping only), then the cuts of the running decomposition, (q, n) as the scans use them
    __shared__ int s_row[128];                         // stream_hull's run offsets
    __shared__ double s_seedCi[9];                     // C^-1 of the seed ellipsoid, to tell whether find_ellipsoid changed it
    __shared__ int s_same;
    double rho_prev = 0.0, T1_prev = 0.0; // the planner's previous decomposition (the next box is a little further along the path): cloud points per unit of
    int cnt_prev = -1;                    // volume around its seed, the bound of its first shell and the points that shell held (-1: no decomposition yet)
    const int b = blockIdx.x, lane = threadIdx.x;
#ifdef FRP_CORRIDOR_PROFILE
    long long tp_a = 0, tp_b = 0, tp_tile = 0, tp_shrink = 0, tp_rest = 0, tp_begin = wall_clock64();
    int np_b = 0, np_retry = 0, np_shell = 0, np_dec = 0, np_round = 0, np_listed = 0, np_box = 0;
    CR_T0
#endif
    const double *ref = c.ref_pos + (size_t)b * c.N * 3, *yaw = c.ref_yaw + (size_t)b * c.N, *Eb = c.ellipsoid + (size_t)b * c.N * 9;
    const int P_cloud = c.P;
    const int max_rounds = P_cloud + 8; // (see corridor_kernel: only non-finite input needs the bound)
    if (lane == 0) u.overflow = 0;
    int npoly = 0;
    int i = 0;
    while (i < c.N) {
        // ---- new decomposition around the seed segment of stage i (nmpc_solver.cpp:315-329): lane 0, as in corridor_kernel ----
        if (lane == 0) {
            double sy, cy;
            sincos(yaw[i], &sy, &cy);
            const double p1[3] = {ref[3 * i], ref[3 * i + 1], ref[3 * i + 2]};
            const double p2[3] = {p1[0] + c.seed_len * cy, p1[1] + c.seed_len * sy, p1[2]};
            const double dv[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
            const double len = sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) u.mid[k] = (p1[k] + p2[k]) / 2;
            u.len = len;
            { // local box planes (line_segment.h:47-85)
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
            const double f = len / 2;
            double ax0 = f + c.offset_x, ax1 = f, ax2 = f, c00 = f + c.offset_x, cdd = f;
            if (ax0 > 0) { const double ratio = ax1 / ax0; ax0 *= ratio; ax1 *= ratio; ax2 *= ratio; c00 *= ratio; cdd *= ratio; }
            u.ax[0] = ax0; u.ax[1] = ax1; u.ax[2] = ax2;
            const double pitch = atan2(-dv[2], sqrt(dv[0] * dv[0] + dv[1] * dv[1])), yw = atan2(dv[1], dv[0]);
            const M3 Ri = mul(quat_to_rot(cos(yw / 2), 0, 0, sin(yw / 2)), quat_to_rot(cos(pitch / 2), 0, sin(pitch / 2), 0));
            st3(u.Ri, Ri); st3(u.Rf, Ri);
            st3(u.Ci, inverse(rot_diag_rot(Ri, c00, cdd, cdd)));
            st3(s_seedCi, ld3(u.Ci));
            for (int k = 0; k < 6; ++k)
                for (int j = 0; j < 3; ++j) { s_pl[6 * k + j] = u.box[k][j] + 1e-6 * u.box[6 + k][j]; s_pl[6 * k + 3 + j] = u.box[6 + k][j]; }
        }
        CW_SYNC();
        // ---- first scan through the grid: the in-box points -> list (cloud index | inside-the-seed-ellipsoid flag), the closest inside one
        int count = 0;
        Best cp;
        int hlo[3] = {0, 0, 0}, hhi[3] = {0, 0, 0}, nbox = 0; // the hull of the box in grid cells, the in-box points
#ifdef FRP_CORRIDOR_PROFILE
        CR_ACC(tp_rest)
#endif
        double T1 = -1.0; // bound of the shell pass A lists beside the points inside the seed ellipsoid (< 0: none)
        int rest1 = 0;    //        in-box points beyond it
        // pass A: count the in-box points, list those inside the seed ellipsoid (flag bit), find the closest of them -- and, betting that
        // none is inside (then find_ellipsoid leaves the seed ellipsoid as it is), list the first shell of the seed ellipsoid's metric too
        const M3 Ci = ld3(u.Ci);
        const double d[3] = {u.mid[0], u.mid[1], u.mid[2]};
        const BoxFrame bf = load_box(u, c);
        box_hull(bf, c, hlo, hhi);
        // FRP_CS_FILL eighths of a tile at the density the previous decomposition met -- the cloud's mean, for the planner's first box (any
        // value is correct; this one avoids retries)
        const double box_vol = 8.0 * c.bbox[1] * c.bbox[2] * (0.5 * u.len + c.bbox[0]), unit_seed = 4.1887902047863905 * u.ax[0] * u.ax[1] * u.ax[2];
        {
            const double target = (double)(CW_CAP * FRP_CS_FILL / 8);
            if (cnt_prev >= 0 && T1_prev > 1.0 && T1_prev < __builtin_huge_val()) {
                // the previous shell held cnt_prev points: scale its bound for the target as if the count grew with the shell's volume, by at
                // most 1.6 either way (a density from the shell's own volume would be fooled by the free space around the path)
                double f = cnt_prev > 0 ? cbrt(target / (double)cnt_prev) : 1.26;
                f = f * f; f = f < 0.6 ? 0.6 : (f > FRP_CS_FMAX ? FRP_CS_FMAX : f);
                T1 = T1_prev * f > 1.0 ? T1_prev * f : T1_prev;
            } else {
                const double rho = rho_prev > 0.0 ? rho_prev : (double)c.P / (c.grid_cell * c.grid_cell * c.grid_cell * c.grid_dims[0] * c.grid_dims[1] * c.grid_dims[2]);
                if (rho * box_vol > 0.9 * CW_CAP) {
                    const double r = cbrt(target / (rho * unit_seed)); // (rho unit_seed: points per unit of d2^(3/2))
                    if (r * r > 1.0 && r * r < __builtin_huge_val()) T1 = r * r;
                } else
                    T1 = __builtin_huge_val();
            }
        }
        // A bounded first shell is an ellipsoid around the seed, a fraction of the box: its axis-aligned bounds join the box faces in the row
        // clipping (cut slots 0..5, free until the first cut is made), so this pass reads the cells under the SHELL, not under the box
        // (the points inside the seed ellipsoid lie inside it too).  The in-box count is then the shell's neighbourhood's, and whether
        // anything lies beyond is not known: the pass behind the shell always runs.
        bool clipped = T1 > 1.0 && T1 < __builtin_huge_val();
        if (clipped) {
            if (lane == 0) {
                const M3 R = ld3(u.Ri);
                for (int k = 0; k < 3; ++k) {
                    double e2 = 0.0;
                    for (int j = 0; j < 3; ++j) e2 += (R.m[3 * k + j] * u.ax[j]) * (R.m[3 * k + j] * u.ax[j]);
                    const double ext = sqrt(T1 * e2) * (1.0 + 1e-9) + 1e-9;
                    for (int sgn = 0; sgn < 2; ++sgn) {
                        double *pl = s_pl + 36 + 6 * (2 * k + sgn);
                        for (int j = 0; j < 3; ++j) { pl[j] = u.mid[j] + (j == k ? (sgn ? -ext : ext) : 0.0); pl[3 + j] = j == k ? (sgn ? -1.0 : 1.0) : 0.0; }
                    }
                }
            }
            CW_SYNC();
        }
        for (;;) {
            Best best{1.7976931348623157e308, 0x7fffffff, 0.0, 0.0, 0.0};
            int n_in = 0;
            count = 0; nbox = 0; rest1 = 0;
            stream_hull(c, hlo, hhi, s_row, s_pl, clipped ? 12 : 6, [&](const HullBatch &B, int chunks) {
#pragma unroll
                for (int k = 0; k < CS_U; ++k) {
                    if (k >= chunks) break;
                    const double x = B.x[k], y = B.y[k], z = B.z[k];
                    const int id = B.id[k];
                    const bool in0 = in_box(bf, x, y, z, id) CW_AND_SEEN(x, y, z);
                    bool i1 = false, s1 = false;
                    if (in0) {
                        const double dist = ell_dist2(Ci, d, x, y, z);
                        i1 = dist <= 1;
                        s1 = !i1 && dist < T1;
                        if (i1 && before(dist, id, best.dist, best.idx)) best = Best{dist, id, x, y, z};
                    }
                    nbox += (int)__popcll(__ballot(in0));
                    n_in += (int)__popcll(__ballot(i1));
                    rest1 += (int)__popcll(__ballot(in0 && !i1 && !s1));
                    const uint64_t w1 = __ballot(i1 || s1);
                    if (w1) {
                        const int mine = count + (int)__popcll(w1 & ((1ull << lane) - 1));
                        if ((i1 || s1) && mine < CW_CAP) list[mine] = (uint32_t)id | (i1 ? 0x80000000u : 0u);
                        count += (int)__popcll(w1);
                    }
                }
                return count <= CW_CAP;
            });
            if (count > CW_CAP && T1 > 0.0) { // the bet's shell overflowed the tile: the inside points alone, the whole box; the next box starts from half the bound
                T1_prev = T1 < __builtin_huge_val() ? 0.5 * T1 : 0.0; cnt_prev = T1_prev > 1.0 ? (int)(CW_CAP * FRP_CS_FILL / 8) : -1;
                T1 = -1.0; clipped = false; CW_SYNC();
                continue;
            }
            if (T1 > 0.0) { T1_prev = T1; cnt_prev = count - n_in; }
            // the density met (for a first shell in another metric, below): the shell's points over its volume, or the box's over the box's
            rho_prev = clipped ? (double)(count > 0 ? count : 1) / (T1 * sqrt(T1) * unit_seed) : (double)nbox / box_vol;
            if (clipped) rest1 = 1;
            if (n_in > 0) T1 = -1.0; // find_ellipsoid has work to do: the listed shell is not one of the final ellipsoid (its points stay out of m1)
            cp = wave_best(best);
            break;
        }
#ifdef FRP_CORRIDOR_PROFILE
        CR_ACC(tp_a) ++np_dec; np_box += nbox;
#endif
        if (count > CW_CAP) { // more points in the box than the register tile holds: the workgroup kernels behind take this planner
            if (lane == 0) c.poly_index[(size_t)b * c.N] = -1;
            return;
        }
        CW_SYNC();
        // ---- the register tile and the three point sets (one bit per tile row and lane)
        const int W = (count + 63) / 64;
        TileW tile;
        unsigned m0 = 0, m1 = 0, m2 = 0;
#pragma unroll
        for (int j = 0; j < CW_TILE; ++j) {
            const int pos = j * 64 + lane;
            const bool valid = pos < count;
            const uint32_t e = valid ? list[pos] : 0u;
            const int idj = (int)(e & 0x7fffffffu);
            tile.id[j] = idj;
            tile.x[j] = valid ? c.cloud[3 * (size_t)idj] : 0.0;
            tile.y[j] = valid ? c.cloud[3 * (size_t)idj + 1] : 0.0;
            tile.z[j] = valid ? c.cloud[3 * (size_t)idj + 2] : 0.0;
            if (FRP_CW_D2) tile.d2[FRP_CW_D2 ? j : 0] = 0.0;
            m0 |= (valid ? 1u : 0u) << j;
            m1 |= ((valid && (e >> 31)) ? 1u : 0u) << j;
        }
        m2 = m1;
        // shrink the second axis until no obstacle is inside (line_segment.h:156-181)
        for (int guard = 0; cp.idx != 0x7fffffff && guard < max_rounds; ++guard) {
            if (lane == 0) {
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
            CW_SYNC();
            cp = scan_wave<KEEP_OUTSIDE>(tile, W, m2, m2, u);
        }
        // third axis (line_segment.h:183-208)
        if (lane == 0) st3(u.Ci, inverse(rot_diag_rot(ld3(u.Rf), u.ax[0], u.ax[1], u.ax[2])));
        CW_SYNC();
        cp = scan_wave<KEEP_INSIDE>(tile, W, m1, m2, u);
        for (int guard = 0; cp.idx != 0x7fffffff && guard < max_rounds; ++guard) {
            if (lane == 0) {
                const double pw[3] = {cp.x - u.mid[0], cp.y - u.mid[1], cp.z - u.mid[2]};
                const M3 Rf = ld3(u.Rf);
                double p[3];
                tmul(Rf, pw, p);
                const double dd = 1 - (p[0] / u.ax[0]) * (p[0] / u.ax[0]) - (p[1] / u.ax[1]) * (p[1] / u.ax[1]);
                if (dd > CR_EPS) u.ax[2] = fabs(p[2]) / sqrt(dd);
                st3(u.Ci, inverse(rot_diag_rot(Rf, u.ax[0], u.ax[1], u.ax[2])));
            }
            CW_SYNC();
            cp = scan_wave<KEEP_OUTSIDE>(tile, W, m2, m2, u);
        }
        // hyperplanes (decomp_base.h:63-83) + LinearConstraint rows (polyhedron.h:98-118)
        double *gA = c.poly_A + (((size_t)b * c.N + npoly) * c.F) * 3, *gb = c.poly_b + ((size_t)b * c.N + npoly) * c.F;
        if (lane == 0) {
            const M3 Ci = ld3(u.Ci);
            st3(u.CC, mul(Ci, transpose(Ci)));
            u.rows = 0;
        }
        CW_SYNC();
        { // the in-box points in shells of their distance in the final ellipsoid
#ifdef FRP_CORRIDOR_PROFILE
            CR_ACC(tp_shrink)
#endif
            const double inf = __builtin_huge_val();
            int npl = 0, tries = 0;
            double T_lo = -1.0, T_hi = inf;
            bool have_tile = false;
            if (T1 > 0.0) { // pass A's bet: is the final ellipsoid the seed ellipsoid, bit for bit?  Then its shell is the first one, already in the tile
                if (lane == 0) {
                    int same = 1;
                    for (int k = 0; k < 9; ++k) same &= u.Ci[k] == s_seedCi[k] ? 1 : 0;
                    s_same = same;
                }
                CW_SYNC();
                have_tile = s_same != 0;
            }
            if (!have_tile && rho_prev * box_vol > 0.9 * CW_CAP) { // first shell: the same fraction of a tile at the density pass A met, in the FINAL ellipsoid's metric
                const double per_unit = rho_prev * 4.1887902047863905 * u.ax[0] * u.ax[1] * u.ax[2]; // points per unit of d2^(3/2)
                const double r = cbrt((double)(CW_CAP * FRP_CS_FILL / 8) / per_unit);
                if (r * r > 1.0 && r * r < inf) T_hi = r * r;
            }
            // find_polyhedron's loop on the points of the tile (decomp_base.h:63-83); every cut is kept for the shells behind.  false: too many cuts
            auto cut_tile = [&](int Ws, unsigned s0) -> bool {
                unsigned s2 = 0;
                cp = scan_wave<KEEP_ALL>(tile, Ws, s0, s2, u);
                const double *hm = u.mid, *hC = u.CC; // (measured: the twelve values in scalar registers across the rounds instead -- no gain)
                for (int guard = 0; cp.idx != 0x7fffffff && guard < max_rounds; ++guard) {
                    const double q[3] = {cp.x, cp.y, cp.z};
                    const double w[3] = {q[0] - hm[0], q[1] - hm[1], q[2] - hm[2]};
                    double n[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) n[k] = hC[3 * k] * w[0] + hC[3 * k + 1] * w[1] + hC[3 * k + 2] * w[2];
                    const double nl = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
                    for (int k = 0; k < 3; ++k) n[k] /= nl;
                    if (npl >= CS_PLANES) return false;
                    if (lane == 0) { // (the cut is kept; its ROW is made after the loop, off this chain)
#pragma unroll
                        for (int k = 0; k < 3; ++k) { s_pl[36 + 6 * npl + k] = q[k]; s_pl[36 + 6 * npl + 3 + k] = n[k]; }
                    }
                    ++npl;
                    if (FRP_CW_PACK && Ws > CW_PACK / 64) {
                        int kept;
                        cp = scan_wave<KEEP_BEHIND_PLANE>(tile, Ws, s2, s2, u, q, n, &kept);
                        if (kept <= CW_PACK) pack_tile(tile, s2, Ws, kept, list);
                    } else
                        cp = scan_wave<KEEP_BEHIND_PLANE>(tile, Ws, s2, s2, u, q, n);
                }
                CW_SYNC(); // the new cuts are visible to every lane; the list may be overwritten
                return true;
            };
            bool more = true;
            if (have_tile) { // (its own copy of the loop: inside the shell loop below the tile is dead while a pass streams)
                if (!cut_tile(W, m0)) { if (lane == 0) c.poly_index[(size_t)b * c.N] = -1; return; }
#ifdef FRP_CORRIDOR_PROFILE
                CR_ACC(tp_tile) np_round += npl; ++np_shell; np_listed += count;
#endif
                more = rest1 > 0 && T1 < inf;
                T_lo = T1; T_hi = inf;
            }
            while (more) {
                int cnt = 0, rest = 0;
                {
                    const M3 Ci = ld3(u.Ci);
                    const double d[3] = {u.mid[0], u.mid[1], u.mid[2]};
                    const BoxFrame bf = load_box(u, c);
                    stream_hull(c, hlo, hhi, s_row, s_pl, 6 + npl, [&](const HullBatch &B, int chunks) {
                        bool al[CS_U];
                        double dist[CS_U];
                        uint64_t any = 0;
#pragma unroll
                        for (int k = 0; k < CS_U; ++k) {
                            al[k] = k < chunks && in_box(bf, B.x[k], B.y[k], B.z[k], B.id[k]) CW_AND_SEEN(B.x[k], B.y[k], B.z[k]);
                            dist[k] = 0.0;
                            if (al[k]) { dist[k] = ell_dist2(Ci, d, B.x[k], B.y[k], B.z[k]); al[k] = dist[k] >= T_lo; }
                            any |= __ballot(al[k]);
                        }
                        // a point is alive iff it is in front of every cut so far (most are behind one of the first): a cut is fetched from
                        // LDS once for the whole batch
                        for (int p = 0; p < npl && any; ++p) {
                            double q[3], n[3];
#pragma unroll
                            for (int j = 0; j < 3; ++j) { q[j] = s_pl[36 + 6 * p + j]; n[j] = s_pl[36 + 6 * p + 3 + j]; }
                            any = 0;
#pragma unroll
                            for (int k = 0; k < CS_U; ++k) {
                                al[k] = al[k] && cut_side(n, q, B.x[k], B.y[k], B.z[k]) < 0;
                                any |= __ballot(al[k]);
                            }
                        }
#pragma unroll
                        for (int k = 0; k < CS_U; ++k) {
                            const bool sh = al[k] && dist[k] < T_hi;
                            rest += (int)__popcll(__ballot(al[k] && !sh));
                            const uint64_t w = __ballot(sh);
                            if (w) {
                                const int mine = cnt + (int)__popcll(w & ((1ull << lane) - 1));
                                if (sh && mine < CW_CAP) list[mine] = (uint32_t)B.id[k];
                                cnt += (int)__popcll(w);
                            }
                        }
                        return cnt <= CW_CAP;
                    });
                }
#ifdef FRP_CORRIDOR_PROFILE
                CR_ACC(tp_b) ++np_b; if (cnt > CW_CAP) ++np_retry; else { ++np_shell; np_listed += cnt; }
#endif
                if (cnt > CW_CAP) { // more than a tile: narrow the shell and stream again
                    if (++tries > CS_RETRIES) { if (lane == 0) c.poly_index[(size_t)b * c.N] = -1; return; }
                    const double base = T_lo > 0.0 ? T_lo : 0.0;
                    T_hi = T_hi == inf ? (base > 1.0 ? base : 1.0) * 2.5 : base + (T_hi - base) * 0.4;
                    CW_SYNC();
                    continue;
                }
                CW_SYNC();
                unsigned s0 = 0;
#pragma unroll
                for (int j = 0; j < CW_TILE; ++j) {
                    const int pos = j * 64 + lane;
                    const bool valid = pos < cnt;
                    const int idj = valid ? (int)list[pos] : 0;
                    tile.id[j] = idj;
                    tile.x[j] = valid ? c.cloud[3 * (size_t)idj] : 0.0;
                    tile.y[j] = valid ? c.cloud[3 * (size_t)idj + 1] : 0.0;
                    tile.z[j] = valid ? c.cloud[3 * (size_t)idj + 2] : 0.0;
                    if (FRP_CW_D2) tile.d2[FRP_CW_D2 ? j : 0] = 0.0;
                    s0 |= (valid ? 1u : 0u) << j;
                }
                if (!cut_tile((cnt + 63) / 64, s0)) { if (lane == 0) c.poly_index[(size_t)b * c.N] = -1; return; }
#ifdef FRP_CORRIDOR_PROFILE
                CR_ACC(tp_tile) np_round += npl;
#endif
                more = rest > 0 && T_hi < inf;
                T_lo = T_hi; T_hi = inf;
            }
            // the LinearConstraint rows of the cuts (polyhedron.h:98-118), lane = cut, all at once: emit_row's own arithmetic, but not one
            // lane-0 detour (LDS counter, three dot products, eight stores) in every round of the loop above
            static_assert(CS_PLANES <= 64, "one lane per cut");
            if (lane < npl) {
                const double *pl = s_pl + 36 + 6 * lane;
                double n[3] = {pl[3], pl[4], pl[5]};
                double cc = pl[0] * n[0] + pl[1] * n[1] + pl[2] * n[2];
                if (n[0] * u.mid[0] + n[1] * u.mid[1] + n[2] * u.mid[2] - cc > 0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; cc = -cc; }
                if (lane < c.F) {
                    s_A[3 * lane] = n[0]; s_A[3 * lane + 1] = n[1]; s_A[3 * lane + 2] = n[2]; s_b[lane] = cc;
                    gA[3 * lane] = n[0]; gA[3 * lane + 1] = n[1]; gA[3 * lane + 2] = n[2]; gb[lane] = cc;
                }
            }
            if (lane == 0) { u.rows = npl; if (npl > c.F) u.overflow = 1; }
            CW_SYNC();
        }
        if (lane == 0) {
            for (int k = 0; k < 6; ++k) emit_row(u, u.box[k], u.box[6 + k], c.F, s_A, s_b, gA, gb);
            c.poly_nfaces[(size_t)b * c.N + npoly] = u.rows;
            c.poly_index[(size_t)b * c.N + i] = npoly;
        }
        CW_SYNC();
        const int rows = u.rows < c.F ? u.rows : c.F;
        // ---- which of the stages behind still fit this polytope (nmpc_solver.cpp:291-313)?  All of them at once: lane = (row group, stage) --
        // 64 / N lanes share a stage's rows (three at N = 20: a row costs a square root, thirty of them on twenty lanes were 6 us of every
        // decomposition) and a ballot puts the groups' verdicts together
        const int cgrp = 64 / c.N, cst = lane % c.N, csub = lane / c.N;
        bool viol = false;
        if (csub < cgrp && cst > i) {
            const double *E = Eb + 9 * cst;
            const double E0 = E[0], E1 = E[1], E2 = E[2], E3 = E[3], E4 = E[4], E5 = E[5], E6 = E[6], E7 = E[7], E8 = E[8];
            const double r0 = ref[3 * cst], r1 = ref[3 * cst + 1], r2 = ref[3 * cst + 2];
            for (int r = csub; r < rows; r += cgrp) {
                const double a0 = s_A[3 * r], a1 = s_A[3 * r + 1], a2 = s_A[3 * r + 2];
                const double e0 = E0 * a0 + E1 * a1 + E2 * a2, e1 = E3 * a0 + E4 * a1 + E5 * a2, e2 = E6 * a0 + E7 * a1 + E8 * a2;
                const double add = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
                viol = viol || (a0 * r0 + a1 * r1 + a2 * r2 - (s_b[r] - c.inflation * add)) > 0;
            }
        }
        uint64_t vm = __ballot(viol);
        for (int g = 1; g < cgrp; ++g) vm |= vm >> (g * c.N); // (bits 0 .. N-1: the stage's verdict over all its row groups; garbage above)
        if (c.N < 64) vm &= (1ull << c.N) - 1ull;
        const int next = vm ? (int)__builtin_ctzll(vm) : c.N; // the first stage whose inflated tube ellipsoid leaves the polytope
        if (lane > i && lane < next) c.poly_index[(size_t)b * c.N + lane] = npoly;
        ++npoly;
        i = next;
    }
#ifdef FRP_CORRIDOR_PROFILE
    if (lane == 0 && (b == 0 || b == 1000) && np_dec > 0)
        printf("wave %d: total %lld passA %lld passB %lld (%d passes, %d retries, %d shells) tile+rounds %lld shrink %lld rest %lld [100 MHz ticks]; %d decompositions, "
               "%d in-box points, %d listed, %d cuts (cumulative per shell)\n", b, wall_clock64() - tp_begin, tp_a, tp_b, np_b, np_retry, np_shell, tp_tile, tp_shrink, tp_rest,
               np_dec, np_box, np_listed, np_round);
#endif
    if (lane == 0) {
        for (int k = npoly; k < c.N; ++k) c.poly_nfaces[(size_t)b * c.N + k] = 0;
        if (c.poly_count) c.poly_count[b] = u.overflow ? -npoly : npoly;
    }
}
