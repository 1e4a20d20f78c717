// frp_corridor_scan.inc -- the device code that every corridor translation unit shares (frp_corridor.hip, frp_corridor_large.hip):
// the per-point expressions, the workgroup minimum, the wave-uniform state of a decomposition (struct Uni), the visibility cut, the
// scans over masks of list positions, the first scans, emit_row, and the local box as a frame with its hull in grid cells.  Moved here
// from frp_corridor.hip word for word; the kernels that use it stay in their files.  The includer sets
//     #pragma clang fp contract(off)
// BEFORE including this file and includes <hip/hip_runtime.h>, <math.h>, <stdint.h> and frp_nmpc.h (see frp_corridor.hip for why: every
// kernel must compute the same bits from the same inputs).
namespace frp {

// a0 * x + a1 * y + a2 * z with the rounding every kernel uses
__device__ __forceinline__ double dot3(double a0, double a1, double a2, double x, double y, double z)
{
    return __builtin_fma(a2, z, __builtin_fma(a1, y, a0 * x));
}
// on which side of the cut (q, n) the point lies (decomp_base.h:74-78: kept while negative)
__device__ __forceinline__ double cut_side(const double n[3], const double q[3], double x, double y, double z)
{
    return dot3(n[0], n[1], n[2], x - q[0], y - q[1], z - q[2]);
}

#ifndef FRP_CR_WAVES
#define FRP_CR_WAVES 4
#endif
constexpr int CR_WAVES = FRP_CR_WAVES, CR_THREADS = 64 * CR_WAVES, CR_UNROLL = 4, CR_BATCH = 2;
constexpr double CR_EPS = 1e-10; // epsilon_, data_type.h:129

struct M3 { double m[9]; };

__device__ __forceinline__ M3 mul(const M3 &a, const M3 &b)
{
    M3 r;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r.m[3 * i + j] = a.m[3 * i] * b.m[j] + a.m[3 * i + 1] * b.m[3 + j] + a.m[3 * i + 2] * b.m[6 + j];
    return r;
}
__device__ __forceinline__ M3 transpose(const M3 &a)
{
    M3 r;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r.m[3 * i + j] = a.m[3 * j + i];
    return r;
}
__device__ __forceinline__ M3 inverse(const M3 &a) // cofactors / determinant
{
    const double *m = a.m;
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double inv = 1.0 / (m[0] * c00 + m[1] * c01 + m[2] * c02);
    M3 r;
    r.m[0] = c00 * inv; r.m[1] = (m[2] * m[7] - m[1] * m[8]) * inv; r.m[2] = (m[1] * m[5] - m[2] * m[4]) * inv;
    r.m[3] = c01 * inv; r.m[4] = (m[0] * m[8] - m[2] * m[6]) * inv; r.m[5] = (m[2] * m[3] - m[0] * m[5]) * inv;
    r.m[6] = c02 * inv; r.m[7] = (m[1] * m[6] - m[0] * m[7]) * inv; r.m[8] = (m[0] * m[4] - m[1] * m[3]) * inv;
    return r;
}
__device__ __forceinline__ M3 quat_to_rot(double w, double x, double y, double z)
{
    M3 r;
    r.m[0] = 1 - 2 * (y * y + z * z); r.m[1] = 2 * (x * y - w * z);     r.m[2] = 2 * (x * z + w * y);
    r.m[3] = 2 * (x * y + w * z);     r.m[4] = 1 - 2 * (x * x + z * z); r.m[5] = 2 * (y * z - w * x);
    r.m[6] = 2 * (x * z - w * y);     r.m[7] = 2 * (y * z + w * x);     r.m[8] = 1 - 2 * (x * x + y * y);
    return r;
}
__device__ __forceinline__ M3 rot_diag_rot(const M3 &R, double a0, double a1, double a2) // R diag(a) R'
{
    M3 r;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            r.m[3 * i + j] = R.m[3 * i] * a0 * R.m[3 * j] + R.m[3 * i + 1] * a1 * R.m[3 * j + 1] + R.m[3 * i + 2] * a2 * R.m[3 * j + 2];
    return r;
}
__device__ __forceinline__ void tmul(const M3 &R, const double v[3], double o[3]) // o = R' v
{
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = R.m[j] * v[0] + R.m[3 + j] * v[1] + R.m[6 + j] * v[2];
}
// Ellipsoid::dist (ellipsoid.h:19-21), squared, with C^-1 precomputed.  The scans are FP64-VALU-bound and a square
// root is half of their arithmetic, so it is taken only where the reference's threshold needs it (1 - dist >
// epsilon_); "dist <= 1" and the ordering of distances are the same on the squares.
__device__ __forceinline__ double ell_dist2(const M3 &Ci, const double d[3], double x, double y, double z)
{
    const double u = x - d[0], v = y - d[1], w = z - d[2];
    const double a = dot3(Ci.m[0], Ci.m[1], Ci.m[2], u, v, w), b = dot3(Ci.m[3], Ci.m[4], Ci.m[5], u, v, w), c = dot3(Ci.m[6], Ci.m[7], Ci.m[8], u, v, w);
    return dot3(a, b, c, a, b, c);
}

struct Best { double dist; int idx; double x, y, z; }; // candidate closest point: SQUARED metric distance, cloud index, coordinates

__device__ __forceinline__ bool before(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

// Wave minima on the DPP network (quad_perm, row_half_mirror, row_mirror, then v_readlane across the four rows):
// a ds_bpermute butterfly costs an LDS round trip per step, and this reduction runs once per scan.
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true); }
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const int lo = dpp_i32<CTRL>((int)(unsigned)b), hi = dpp_i32<CTRL>((int)(unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
__device__ __forceinline__ double wave_min_f64(double v)
{
    v = fmin(v, dpp_f64<0xB1>(v)); v = fmin(v, dpp_f64<0x4E>(v)); v = fmin(v, dpp_f64<0x141>(v)); v = fmin(v, dpp_f64<0x140>(v));
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    double r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        r[k] = __longlong_as_double((long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), 16 * k) << 32) |
                                                (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, 16 * k)));
    return fmin(fmin(r[0], r[1]), fmin(r[2], r[3]));
}
__device__ __forceinline__ int wave_min_i32(int v)
{
    v = min(v, dpp_i32<0xB1>(v)); v = min(v, dpp_i32<0x4E>(v)); v = min(v, dpp_i32<0x141>(v)); v = min(v, dpp_i32<0x140>(v));
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// minimum over the workgroup in (distance, index) order; idx = INT_MAX when no point was alive.  The winner's
// coordinates travel with it, so nobody has to fetch the point again.  s_red is double-buffered by `phase`: one barrier.
__device__ Best block_min(const Best &mine, Best *s_red, int &phase)
{
    const double d = wave_min_f64(mine.dist);
    const int i = wave_min_i32(mine.dist == d ? mine.idx : 0x7fffffff);
    Best *buf = s_red + phase * CR_WAVES;
    phase ^= 1;
    const int lane = threadIdx.x & 63;
    if (i == 0x7fffffff ? lane == 0 : mine.idx == i) buf[threadIdx.x >> 6] = mine; // the lane that owns the wave's minimum
    __syncthreads();
    Best r = buf[0];
#pragma unroll
    for (int w = 1; w < CR_WAVES; ++w)
        if (before(buf[w].dist, buf[w].idx, r.dist, r.idx)) r = buf[w];
    return r;
}

struct Scan {             // what a scan iterates over
    const double *pts;    // the planner's cloud [.][3]
    const uint32_t *list; // nullptr: positions are cloud indices; else positions index this list of cloud indices
    int Pn, W;            // positions, 64-position words
};

#ifndef FRP_CR_TILE
#define FRP_CR_TILE 5
#endif
#ifndef FRP_CR_WPE
#define FRP_CR_WPE 3
#endif
// Register tile of 5 words per wave (1280 points per planner) at three workgroups per CU: a decomposition is a chain of
// ~20 latency-bound scans (reduction, barrier, thread-0 algebra), so a third resident workgroup per CU is worth more than the
// 8-word tile that needs 256 VGPRs (full tick, 4096 planners: 1.32 -> 1.09 ms; 4 per CU spills too much: 1.28; two-wave
// workgroups: 1.27-1.52).
constexpr int CR_TILE = FRP_CR_TILE; // 64-position words per wave held in registers (CR_TILE * CR_THREADS points per planner)
#ifndef FRP_CR_LIST
#define FRP_CR_LIST 8192
#endif
constexpr int CR_LIST = FRP_CR_LIST; // capacity of the in-box index list (LDS); larger boxes fall back to cloud positions

// Wave-uniform state of the running decomposition.  It lives in LDS and is advanced by thread 0 only, so the 3x3
// algebra costs no registers in the scanning waves: a scan loads just the 9 + 3 (+ 6) doubles it needs.
struct Uni {
    double Ri[9], Rf[9], Ci[9], CC[9]; // initial / final ellipsoid frame, C^-1, C^-1 C^-T
    double mid[3], ax[3];              // ellipsoid centre (p1 + p2) / 2, semi-axes
    double box[12][3];                 // local box: points 0..5, outward normals 6..11
    double frame[3][3], p1[3], len;    // the same box as a frame at p1: axes dir_h, dir, dir_v; segment length
    int rows, overflow, count;         // rows emitted, > F rows seen, in-box points appended to the list
};

__device__ __forceinline__ M3 ld3(const double *p) { M3 r; for (int k = 0; k < 9; ++k) r.m[k] = p[k]; return r; }
__device__ __forceinline__ void st3(double *p, const M3 &a) { for (int k = 0; k < 9; ++k) p[k] = a.m[k]; }

#ifdef FRP_CORRIDOR_PROFILE
__device__ long long g_prof[2];
#endif

// The visibility cut of frp_nmpc_corridor_batch_cut: planner b sees a point of the SHARED cloud iff lo[k] <= q[k] < hi[k] on every axis,
// lo / hi = origin + box[b][k] * resolution (one multiply, one add: this file is fp contract(off)) -- the loops of localOccVisCallback
// (occ_map.cpp:192-194) in position form.  One more conjunct on "in the local box" in every FIRST scan (scan_cloud, scan_grid, the
// passes of the one-wavefront kernel); the later scans run over what the first one listed.  The six bounds are uniform per planner:
// computed once at kernel entry and pinned to scalar registers, so a point costs six compares against SGPR operands and no VGPR.
// A NaN coordinate fails every compare (invisible); a row with min > max has lo > hi (nothing visible).  CUT = false: no code at all --
// the uncut kernels are the instantiations they were.
struct CutBox { double lo[3], hi[3]; };
__device__ __forceinline__ double uniform_f64(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32)) << 32) |
                                            (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b)));
}
__device__ __forceinline__ CutBox load_cut(const frp_nmpc_corridor_cut &cut, int b)
{
    CutBox cb;
    const int *row = cut.box + 6 * (size_t)b;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        cb.lo[k] = uniform_f64(cut.origin[k] + (double)row[k] * cut.resolution);
        cb.hi[k] = uniform_f64(cut.origin[k] + (double)row[3 + k] * cut.resolution);
    }
    return cb;
}
struct CorridorCutArgs { frp_nmpc_corridor c; frp_nmpc_corridor_cut cut; };
template <bool CUT> struct CorridorArgsOf { typedef frp_nmpc_corridor type; };
template <> struct CorridorArgsOf<true> { typedef CorridorCutArgs type; };
template <bool CUT> using CorridorArgs = typename CorridorArgsOf<CUT>::type;
__device__ __forceinline__ const frp_nmpc_corridor &corridor_of(const frp_nmpc_corridor &a) { return a; }
__device__ __forceinline__ const frp_nmpc_corridor &corridor_of(const CorridorCutArgs &a) { return a.c; }
__device__ __forceinline__ const frp_nmpc_corridor_cut &cut_of(const CorridorCutArgs &a) { return a.cut; }
__device__ __forceinline__ frp_nmpc_corridor_cut cut_of(const frp_nmpc_corridor &) { return frp_nmpc_corridor_cut{}; } // (never evaluated: CUT = false)
template <bool CUT>
__device__ __forceinline__ bool cut_sees(const CutBox &cb, double x, double y, double z)
{
    if (!CUT) return true;
    return cb.lo[0] <= x && x < cb.hi[0] && cb.lo[1] <= y && y < cb.hi[1] && cb.lo[2] <= z && z < cb.hi[2];
}

enum { KEEP_OUTSIDE = 0, KEEP_INSIDE = 1, KEEP_ALL = 2, KEEP_BEHIND_PLANE = 3 };

// One pass: out = { points of `in` that satisfy MODE }, returns the kept point closest to the centre in the metric
// of u.Ci (first minimum in list order).  Word g of a mask is always handled by wave g % CR_WAVES.
template <int MODE>
__device__ __forceinline__ Best scan(const Scan &s, const uint64_t *in, uint64_t *out, const Uni &u, Best *s_red, int &phase,
                                     const double *pq = nullptr, const double *pn = nullptr)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#ifdef FRP_CORRIDOR_PROFILE
    long long ts0 = wall_clock64();
#endif
    const M3 Ci = ld3(u.Ci);
    const double d[3] = {u.mid[0], u.mid[1], u.mid[2]};
    double q[3] = {0, 0, 0}, n[3] = {0, 0, 0};
    if (MODE == KEEP_BEHIND_PLANE) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { q[k] = pq[k]; n[k] = pn[k]; } // the hyperplane, computed by every lane from the reduction's winner
    }
    Best best{1.7976931348623157e308, 0x7fffffff, 0.0, 0.0, 0.0};
    // Most words of a list are empty.  Each lane fetches one of the wave's next 64 words, a ballot tells which are
    // not, and only those are visited -- one LDS round trip per 4096 points instead of one per 64.
    for (int base = wave; base < s.W; base += CR_WAVES * 64) {
        const int gm = base + lane * CR_WAVES;
        const uint64_t wm = gm < s.W ? in[gm] : 0;
        if (out != in && gm < s.W && wm == 0) out[gm] = 0;
        uint64_t nz = __ballot(wm != 0);
        while (nz) { // up to CR_BATCH non-empty words at a time, their loads issued together
            int gs[CR_BATCH], id[CR_BATCH];
            bool al[CR_BATCH];
            double x[CR_BATCH], y[CR_BATCH], z[CR_BATCH];
#pragma unroll
            for (int k = 0; k < CR_BATCH; ++k) {
                gs[k] = -1; id[k] = 0; al[k] = false; x[k] = y[k] = z[k] = 0.0;
                if (nz) {
                    const int l = __builtin_ctzll(nz);
                    nz &= nz - 1;
                    gs[k] = base + l * CR_WAVES;
                    const uint64_t word = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(wm >> 32), l) << 32) |
                                          (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)wm, l);
                    const int pos = gs[k] * 64 + lane;
                    al[k] = ((word >> lane) & 1) && pos < s.Pn;
                    if (al[k]) {
                        id[k] = s.list ? (int)(s.list[pos] & 0x7fffffffu) : pos;
                        x[k] = s.pts[3 * (size_t)id[k]]; y[k] = s.pts[3 * (size_t)id[k] + 1]; z[k] = s.pts[3 * (size_t)id[k] + 2];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < CR_BATCH; ++k) {
                if (gs[k] < 0) break;
                bool alive = al[k];
                if (alive) {
                    const double dist = ell_dist2(Ci, d, x[k], y[k], z[k]); // squared: same order, same "<= 1"
                    if (MODE == KEEP_OUTSIDE) alive = 1 - sqrt(dist) > CR_EPS;
                    if (MODE == KEEP_INSIDE) alive = dist <= 1;
                    if (MODE == KEEP_BEHIND_PLANE) alive = cut_side(n, q, x[k], y[k], z[k]) < 0;
                    if (alive && before(dist, id[k], best.dist, best.idx)) best = Best{dist, id[k], x[k], y[k], z[k]};
                }
                const uint64_t o = __ballot(alive);
                if (lane == 0) out[gs[k]] = o;
            }
        }
    }
#ifdef FRP_CORRIDOR_PROFILE
    long long ts1 = wall_clock64();
    Best r_ = block_min(best, s_red, phase);
    if (threadIdx.x == 0) { g_prof[0] += ts1 - ts0; g_prof[1] += wall_clock64() - ts1; }
    return r_;
#else
    return block_min(best, s_red, phase);
#endif
}

// The same pass when the whole list fits the wave's REGISTER TILE: up to CR_TILE words per wave (CR_TILE * 256 points
// per workgroup), whose coordinates and cloud indices were loaded once after the first scan and stay in VGPRs for
// the 20-30 scans of the decomposition -- no memory traffic at all besides the mask words.
// d2 = the squared metric distance of the point in the FINAL ellipsoid: the hyperplane loop (decomp_base.h:63-83) cuts with a fixed
// ellipsoid, so the distances its rounds compare are computed once, by the KEEP_ALL scan that opens it
struct Tile { double x[CR_TILE], y[CR_TILE], z[CR_TILE], d2[CR_TILE]; int id[CR_TILE]; };

template <int MODE>
__device__ __forceinline__ Best scan_tile(Tile &t, int W, const uint64_t *in, uint64_t *out, const Uni &u, Best *s_red, int &phase,
                                          const double *pq = nullptr, const double *pn = nullptr)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const M3 Ci = ld3(u.Ci);
    const double d[3] = {u.mid[0], u.mid[1], u.mid[2]};
    double q[3] = {0, 0, 0}, n[3] = {0, 0, 0};
    if (MODE == KEEP_BEHIND_PLANE) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { q[k] = pq[k]; n[k] = pn[k]; } // the hyperplane, computed by every lane from the reduction's winner
    }
    uint64_t w[CR_TILE];
#pragma unroll
    for (int j = 0; j < CR_TILE; ++j) { const int g = wave + j * CR_WAVES; w[j] = g < W ? in[g] : 0; }
    Best best{1.7976931348623157e308, 0x7fffffff, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < CR_TILE; ++j) {
        const int g = wave + j * CR_WAVES;
        if (g >= W) break;
        if (w[j] == 0) { if (out != in && lane == 0) out[g] = 0; continue; }
        bool alive = (w[j] >> lane) & 1;
        if (alive) {
            // (the rounds of the hyperplane loop compare the distances its opening KEEP_ALL scan stored: same values, no recomputation)
            const double dist = MODE == KEEP_BEHIND_PLANE ? t.d2[j] : ell_dist2(Ci, d, t.x[j], t.y[j], t.z[j]);
            if (MODE == KEEP_ALL) t.d2[j] = dist;
            if (MODE == KEEP_OUTSIDE) alive = 1 - sqrt(dist) > CR_EPS;
            if (MODE == KEEP_INSIDE) alive = dist <= 1;
            if (MODE == KEEP_BEHIND_PLANE) alive = cut_side(n, q, t.x[j], t.y[j], t.z[j]) < 0;
            if (alive && before(dist, t.id[j], best.dist, best.idx)) best = Best{dist, t.id[j], t.x[j], t.y[j], t.z[j]};
        }
        const uint64_t o = __ballot(alive);
        if (lane == 0) out[g] = o;
    }
    return block_min(best, s_red, phase);
}

// first scan of a decomposition: obs_ = cloud points inside the local box (decomp_base.h:33-38) -> m0, obs = those
// inside the seed ellipsoid -> m1 and m2.  Every point is read here, so the loads of CR_UNROLL word groups are
// issued before any of them is used.
template <bool CUT>
__device__ __forceinline__ Best scan_cloud(const Scan &s, uint64_t *m0, uint64_t *m1, uint64_t *m2, uint32_t *list, Uni &u, bool has_box, const double *bbox, const CutBox &cb, Best *s_red, int &phase)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const M3 Ci = ld3(u.Ci);
    const double d[3] = {u.mid[0], u.mid[1], u.mid[2]};
    // The six planes of add_local_bbox have unit normals +-dir_h, +-dir, +-dir_v, so signed_dist(x) > epsilon_ for
    // any of them is a bound on the coordinates of x - p1 in that frame (12 + 4 registers instead of 36).
    double fr[3][3], o[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[k] = u.p1[k];
#pragma unroll
        for (int j = 0; j < 3; ++j) fr[k][j] = u.frame[k][j];
    }
    const double bh = bbox[1] + CR_EPS, bd_lo = -bbox[0] - CR_EPS, bd_hi = u.len + bbox[0] + CR_EPS, bv = bbox[2] + CR_EPS;
    Best best{1.7976931348623157e308, 0x7fffffff, 0.0, 0.0, 0.0};
    for (int g0 = wave; g0 < s.W; g0 += CR_WAVES * CR_UNROLL) {
        double x[CR_UNROLL], y[CR_UNROLL], z[CR_UNROLL];
#pragma unroll
        for (int k = 0; k < CR_UNROLL; ++k) {
            const int idx = (g0 + k * CR_WAVES) * 64 + lane;
            const size_t o3 = 3 * (size_t)(idx < s.Pn ? idx : 0);
            x[k] = s.Pn ? s.pts[o3] : 0.0; y[k] = s.Pn ? s.pts[o3 + 1] : 0.0; z[k] = s.Pn ? s.pts[o3 + 2] : 0.0;
        }
        uint64_t w0[CR_UNROLL];
        bool i1[CR_UNROLL];
        int total = 0;
#pragma unroll
        for (int k = 0; k < CR_UNROLL; ++k) {
            const int g = g0 + k * CR_WAVES, idx = g * 64 + lane;
            bool in0 = g < s.W && idx < s.Pn;
            if (CUT) in0 = in0 && cut_sees<CUT>(cb, x[k], y[k], z[k]); // (without a local box the cut is the only filter)
            i1[k] = false;
            if (has_box) { // Polyhedron::inside: rejected if signed_dist > epsilon_ (polyhedron.h:51-58)
                const double ex = x[k] - o[0], ey = y[k] - o[1], ez = z[k] - o[2];
                const double h = dot3(fr[0][0], fr[0][1], fr[0][2], ex, ey, ez), t = dot3(fr[1][0], fr[1][1], fr[1][2], ex, ey, ez),
                             v = dot3(fr[2][0], fr[2][1], fr[2][2], ex, ey, ez);
                in0 = in0 && !(h > bh) && !(-h > bh) && !(t > bd_hi) && !(t < bd_lo) && !(v > bv) && !(-v > bv);
            }
            if (in0) {
                const double dist = ell_dist2(Ci, d, x[k], y[k], z[k]);
                i1[k] = dist <= 1;
                if (i1[k] && dist < best.dist) best = Best{dist, idx, x[k], y[k], z[k]};
            }
            w0[k] = __ballot(in0);
            const uint64_t w1 = __ballot(i1[k]);
            if (lane == 0 && g < s.W) { m0[g] = w0[k]; m1[g] = w1; m2[g] = w1; }
            total += (int)__popcll(w0[k]);
        }
        if (total) { // append the in-box points to the dense list (any order: minima are tie-broken by cloud index);
                     // one LDS atomic per CR_UNROLL words
            int at = 0;
            if (lane == 0) at = atomicAdd(&u.count, total);
            at = __builtin_amdgcn_readfirstlane(at);
#pragma unroll
            for (int k = 0; k < CR_UNROLL; ++k) {
                const int mine = at + (int)__popcll(w0[k] & ((1ull << lane) - 1));
                if (((w0[k] >> lane) & 1) && mine < CR_LIST)
                    list[mine] = (uint32_t)((g0 + k * CR_WAVES) * 64 + lane) | (i1[k] ? 0x80000000u : 0u);
                at += (int)__popcll(w0[k]);
            }
        }
    }
    return block_min(best, s_red, phase);
}

// first scan of a decomposition when the cloud comes with a uniform grid (frp_nmpc_cloud_grid_build): only the cell
// rows that meet the axis-aligned hull of the local box are read -- each row (cells ix0..ix1 of one (iy, iz)) is one
// contiguous run of the cell-sorted points, CR_GROWS rows in flight per wave.  Produces the dense list only (no cloud
// masks); minima are tie-broken by the ORIGINAL cloud index, so the result is the same as scanning the whole cloud.
constexpr int CR_GROWS = 2;
template <bool CUT>
__device__ __forceinline__ Best scan_grid(const frp_nmpc_corridor &c, const CutBox &cb, uint32_t *list, Uni &u, Best *s_red, int &phase)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const M3 Ci = ld3(u.Ci);
    const double d[3] = {u.mid[0], u.mid[1], u.mid[2]};
    double fr[3][3], o[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[k] = u.p1[k];
#pragma unroll
        for (int j = 0; j < 3; ++j) fr[k][j] = u.frame[k][j];
    }
    const double bh = c.bbox[1] + CR_EPS, bd_lo = -c.bbox[0] - CR_EPS, bd_hi = u.len + c.bbox[0] + CR_EPS, bv = c.bbox[2] + CR_EPS;
    // axis-aligned hull of the box { o + h fr0 + t fr1 + v fr2 : |h| <= bh, bd_lo <= t <= bd_hi, |v| <= bv } in cells
    int lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double ctr = o[k] + 0.5 * (bd_lo + bd_hi) * fr[1][k];
        const double half = bh * fabs(fr[0][k]) + 0.5 * (bd_hi - bd_lo) * fabs(fr[1][k]) + bv * fabs(fr[2][k]);
        const double a = floor((ctr - half - c.grid_origin[k]) / c.grid_cell), b = floor((ctr + half - c.grid_origin[k]) / c.grid_cell);
        const int n = c.grid_dims[k];
        lo[k] = a < 0 ? 0 : (a > n - 1 ? n - 1 : (int)a);   // points beyond the grid were binned into its border cells
        hi[k] = b < 0 ? 0 : (b > n - 1 ? n - 1 : (int)b);
    }
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
        for (int off = 0; off < most; off += 64) { // usually one trip: a row of cells holds a few dozen points
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
                bool in0 = id[k] >= 0;
                i1[k] = false;
                const double ex = x[k] - o[0], ey = y[k] - o[1], ez = z[k] - o[2];
                const double h = dot3(fr[0][0], fr[0][1], fr[0][2], ex, ey, ez), t = dot3(fr[1][0], fr[1][1], fr[1][2], ex, ey, ez),
                             v = dot3(fr[2][0], fr[2][1], fr[2][2], ex, ey, ez);
                in0 = in0 && !(h > bh) && !(-h > bh) && !(t > bd_hi) && !(t < bd_lo) && !(v > bv) && !(-v > bv);
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
                    if (((w0[k] >> lane) & 1) && mine < CR_LIST) list[mine] = (uint32_t)id[k] | (i1[k] ? 0x80000000u : 0u);
                    at += (int)__popcll(w0[k]);
                }
            }
        }
    }
    return block_min(best, s_red, phase);
}

// LinearConstraint row of hyperplane (q, n) seen from the seed centre (polyhedron.h:98-118); thread 0 only
__device__ void emit_row(Uni &u, const double q[3], const double n_[3], int F, double *s_A, double *s_b, double *gA, double *gb)
{
    double n[3] = {n_[0], n_[1], n_[2]};
    double cc = q[0] * n[0] + q[1] * n[1] + q[2] * n[2];
    if (n[0] * u.mid[0] + n[1] * u.mid[1] + n[2] * u.mid[2] - cc > 0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; cc = -cc; }
    const int r = u.rows;
    if (r < F) {
        s_A[3 * r] = n[0]; s_A[3 * r + 1] = n[1]; s_A[3 * r + 2] = n[2]; s_b[r] = cc;
        gA[3 * r] = n[0]; gA[3 * r + 1] = n[1]; gA[3 * r + 2] = n[2]; gb[r] = cc;
    } else
        u.overflow = 1;
    u.rows = r + 1;
}

#ifdef FRP_CORRIDOR_PROFILE
#define CR_T0 long long t0_ = wall_clock64();
#define CR_ACC(v) { long long t1_ = wall_clock64(); v += t1_ - t0_; t0_ = t1_; }
#define CR_CNT(v) ++v;
#else
#define CR_CNT(v)
#define CR_T0
#define CR_ACC(v)
#endif

// the local box as the first scans test it (frame at p1, half widths with epsilon_), and its axis-aligned hull in grid cells
struct BoxFrame { double fr[3][3], o[3], bh, bd_lo, bd_hi, bv; };
__device__ __forceinline__ BoxFrame load_box(const Uni &u, const frp_nmpc_corridor &c)
{
    BoxFrame f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        f.o[k] = u.p1[k];
#pragma unroll
        for (int j = 0; j < 3; ++j) f.fr[k][j] = u.frame[k][j];
    }
    f.bh = c.bbox[1] + CR_EPS; f.bd_lo = -c.bbox[0] - CR_EPS; f.bd_hi = u.len + c.bbox[0] + CR_EPS; f.bv = c.bbox[2] + CR_EPS;
    return f;
}
__device__ __forceinline__ bool in_box(const BoxFrame &f, double x, double y, double z, int id)
{
    const double ex = x - f.o[0], ey = y - f.o[1], ez = z - f.o[2];
    const double h = dot3(f.fr[0][0], f.fr[0][1], f.fr[0][2], ex, ey, ez), tt = dot3(f.fr[1][0], f.fr[1][1], f.fr[1][2], ex, ey, ez),
                 v = dot3(f.fr[2][0], f.fr[2][1], f.fr[2][2], ex, ey, ez);
    return id >= 0 && !(h > f.bh) && !(-h > f.bh) && !(tt > f.bd_hi) && !(tt < f.bd_lo) && !(v > f.bv) && !(-v > f.bv);
}
__device__ __forceinline__ void box_hull(const BoxFrame &f, const frp_nmpc_corridor &c, int (&lo)[3], int (&hi)[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double ctr = f.o[k] + 0.5 * (f.bd_lo + f.bd_hi) * f.fr[1][k];
        const double half = f.bh * fabs(f.fr[0][k]) + 0.5 * (f.bd_hi - f.bd_lo) * fabs(f.fr[1][k]) + f.bv * fabs(f.fr[2][k]);
        const double a = floor((ctr - half - c.grid_origin[k]) / c.grid_cell), bb = floor((ctr + half - c.grid_origin[k]) / c.grid_cell);
        const int n = c.grid_dims[k];
        lo[k] = a < 0 ? 0 : (a > n - 1 ? n - 1 : (int)a);
        hi[k] = bb < 0 ? 0 : (bb > n - 1 ? n - 1 : (int)bb);
    }
}

// ---- host side, defined in frp_corridor.hip, for frp_corridor_large.hip
// what frp_nmpc_corridor_batch_cut refuses, with the point limit a parameter (the existing entries pass FRP_CORRIDOR_MAX_POINTS)
bool corridor_args_ok(const frp_nmpc_corridor *p, const frp_nmpc_corridor_cut *cut, int max_points);
// launches 1 and 2 of the chain for a shared cloud with its grid and a local box (the caller has checked both): the one-wavefront kernel
// and the grid workgroup kernel, with or without the cut, dynamic LDS sized for the in-box list (CR_LIST) and not for P
void corridor_launch_listed(const frp_nmpc_corridor *p, const frp_nmpc_corridor_cut *cut, hipStream_t st);

} // namespace frp
