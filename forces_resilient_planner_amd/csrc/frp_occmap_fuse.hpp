// What the translation units of ray-cast fusion share (frp_occmap_fuse.hip: one depth frame per call; frp_occmap_fuse_batch.hip: F depth
// frames per call; frp_occmap_fuse_points.hip: S point scans per call): the frame description and workspace layout, the reference's
// index arithmetic and ray caster, the bodies of the per-pixel / per-ray stages, the batch's descriptors, ordered update and shared
// launch sequence, and the host checks of a description.  All of them are compiled with -ffp-contract=off; everything here that computes a double does it in
// the order tests/occmap_fusion_oracle.py writes down, on the host and on the device alike.
#pragma once
#include <cfloat>
#include <climits>

#include "frp_occmap_raywalk.hpp"

namespace frp {
namespace occmap {
namespace fuse {

constexpr int MAX_ROUNDS = 255;           // the round lives in the top byte of a mark
constexpr int MAX_PIXELS = 1 << 24;       // the sequence number in the other three
constexpr int HDR_INTS = 264;             // [1 .. 255] changed flag of round r, then:
constexpr int H_NRAYS = 256, H_NLIST = 257, H_CONVERGED = 258;
constexpr int NO_RAY = -2, OUTSIDE = -1;  // end voxel of a point: dropped before the ray / outside the map (INVALID_IDX)
constexpr unsigned NO_MARK = 0xFFFFFFFFu;

struct Frame {
    int rows, cols, margin, skip, nu, N;
    const unsigned short *depth, *last;
    double fx, cx, fy, cy;
    double R[9], t[3], Ri[9], lt[3]; // T_wc; last_R^-1 and last_t (shift filter)
    double depth_scale, mindist, tol, hit_log, miss_log, min_len, max_len, cmin, cmax;
    int box[6], bd[3], nbox; // ray box [lo, hi) in voxels, its dimensions and size
    int nb, max_rounds;
    int *status;
};

struct Ws {
    int *hdr;
    double *pts; // [N][3] ray start = the (clipped) point
    int *endv;   // [N] end voxel in the box, OUTSIDE or NO_RAY
    int *cnt;    // [N] cells processed
    int *list;   // cast rays, any order: each entry is a sequence number
    int *all, *hit, *owner;
    unsigned *mark;
};

// the nine arrays of a workspace (slice) that starts at b, at the offsets of Plan.off
__host__ __device__ inline Ws ws_at(char *b, const size_t *off)
{
    Ws w;
    w.hdr = reinterpret_cast<int *>(b + off[0]); w.pts = reinterpret_cast<double *>(b + off[1]);
    w.endv = reinterpret_cast<int *>(b + off[2]); w.cnt = reinterpret_cast<int *>(b + off[3]); w.list = reinterpret_cast<int *>(b + off[4]);
    w.all = reinterpret_cast<int *>(b + off[5]); w.hit = reinterpret_cast<int *>(b + off[6]); w.owner = reinterpret_cast<int *>(b + off[7]);
    w.mark = reinterpret_cast<unsigned *>(b + off[8]);
    return w;
}

// posToIndex + isInMap (:66-75) + the ray box: the voxel's index in the box, or OUTSIDE
__device__ inline int box_voxel(const Geo &g, const Frame &f, double px, double py, double pz)
{
    const double p[3] = {px, py, pz};
    int id[3];
    for (int k = 0; k < 3; k++) {
        const double fl = floored(p[k], g.origin[k], g.res_inv);
        if (!(fl >= 0.0 && fl <= (double)(g.grid[k] - 1))) return OUTSIDE;
        id[k] = (int)fl;
        if (id[k] < f.box[k] || id[k] >= f.box[3 + k]) return OUTSIDE;
    }
    return ((id[0] - f.box[0]) * f.bd[1] + (id[1] - f.box[1])) * f.bd[2] + (id[2] - f.box[2]);
}

__device__ inline double rc_mod(double value, double modulus) { return fmod(fmod(value, modulus) + modulus, modulus); } // raycast.cpp:11-14

__device__ inline double intbound(double s, double ds) // raycast.cpp:16-29
{
    if (ds < 0) { s = -s; ds = -ds; }
    s = rc_mod(s, 1.0);
    return (1 - s) / ds;
}

struct Caster { // RayCaster's members (raycast.h)
    int x, y, z, ex, ey, ez, sx, sy, sz;
    double tmx, tmy, tmz, tdx, tdy, tdz;
};

__device__ inline int sgn(double d) { return d == 0.0 ? 0 : d < 0.0 ? -1 : 1; } // signum((int)dx), :286-288

__device__ inline bool rc_set_input(Caster &c, const double *start, const double *end) // :263-310
{
    c.x = clamp_id(floor(start[0])); c.y = clamp_id(floor(start[1])); c.z = clamp_id(floor(start[2]));
    c.ex = clamp_id(floor(end[0])); c.ey = clamp_id(floor(end[1])); c.ez = clamp_id(floor(end[2]));
    const double dx = (double)c.ex - (double)c.x, dy = (double)c.ey - (double)c.y, dz = (double)c.ez - (double)c.z;
    c.sx = sgn(dx); c.sy = sgn(dy); c.sz = sgn(dz);
    c.tmx = intbound(start[0], dx); c.tmy = intbound(start[1], dy); c.tmz = intbound(start[2], dz);
    c.tdx = (double)c.sx / dx; c.tdy = (double)c.sy / dy; c.tdz = (double)c.sz / dz;
    return !(c.sx == 0 && c.sy == 0 && c.sz == 0);
}

__device__ inline bool rc_at_end(const Caster &c) { return c.x == c.ex && c.y == c.ey && c.z == c.ez; } // :321

__device__ inline void rc_advance(Caster &c) // :336-363
{
    if (c.tmx < c.tmy) {
        if (c.tmx < c.tmz) { c.x += c.sx; c.tmx += c.tdx; }
        else { c.z += c.sz; c.tmz += c.tdz; }
    } else {
        if (c.tmy < c.tmz) { c.y += c.sy; c.tmy += c.tdy; }
        else { c.z += c.sz; c.tmz += c.tdz; }
    }
}

// The while loop of :488-502 over at most `limit` cells: fn(voxel in the box or OUTSIDE) per cell, true = break.  Returns the cells
// processed, -1 when no ray is cast (need_ray, :484).
template <class F>
__device__ inline int walk(const Geo &g, const Frame &f, const double *pt, int limit, F fn)
{
    const double start[3] = {pt[0] / g.res, pt[1] / g.res, pt[2] / g.res}, end[3] = {f.t[0] / g.res, f.t[1] / g.res, f.t[2] / g.res}; // :483
    Caster c;
    if (!rc_set_input(c, start, end)) return -1;
    if (rc_at_end(c)) return -1; // :488 (cannot happen after need_ray)
    rc_advance(c);               // the ray start is skipped
    if (limit > f.nb) limit = f.nb;
    int k = 0;
    while (k < limit) {
        if (rc_at_end(c)) break;
        const double px = ((double)c.x + 0.5) * g.res, py = ((double)c.y + 0.5) * g.res, pz = ((double)c.z + 0.5) * g.res; // :492
        rc_advance(c);
        k++;
        if (fn(box_voxel(g, f, px, py, pz))) break;
    }
    return k;
}

// ---- the stages' bodies: lane i / n / s of one frame.  The kernels of both translation units are these, behind their own indexing ----

__device__ inline void init_lane(const Frame &f, const Ws &w, int i)
{
    if (i < HDR_INTS) w.hdr[i] = 0;
    if (i < f.nbox) { w.all[i] = 0; w.hit[i] = 0; w.owner[i] = INT_MAX; w.mark[i] = NO_MARK; }
}

// The head of raycastProcess's loop (:456-467) for point n = p of a frame whose sensor stands at f.t: the length test, the clip,
// setCacheOccupancy on the end voxel and the owner of cache_rayend_'s dedup.  The caller has set endv[n] = NO_RAY.
__device__ inline void end_lane(const Geo &g, const Frame &f, const Ws &w, int n, double *p)
{
    const double d[3] = {p[0] - f.t[0], p[1] - f.t[1], p[2] - f.t[2]};
    const double length = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]); // :457
    if (length < f.min_len) return;                                         // :459
    int occ = 1;
    if (length > f.max_len) {                                               // :461-464
        for (int i = 0; i < 3; i++) p[i] = d[i] / length * f.max_len + f.t[i];
        occ = 0;
    }
    const int e = box_voxel(g, f, p[0], p[1], p[2]);
    if (e >= 0) { // setCacheOccupancy (:552-560) and the dedup's owner
        atomicAdd(&w.all[e], 1);
        if (occ) atomicAdd(&w.hit[e], 1);
        atomicMin(&w.owner[e], n);
    }
    for (int i = 0; i < 3; i++) w.pts[3 * (size_t)n + i] = p[i];
    w.endv[n] = e;
}

// projectDepthImage (:314-439) and the head of raycastProcess's loop (:456-467) for scanned pixel n
__device__ inline void project_lane(const Geo &g, const Frame &f, const Ws &w, int n)
{
    if (n >= f.N) return;
    const int v = f.margin + (n / f.nu) * f.skip, u = f.margin + (n % f.nu) * f.skip; // :327-329
    w.endv[n] = NO_RAY;
    const double depth = (double)f.depth[(size_t)v * f.cols + u] / f.depth_scale; // :331
    if (depth < f.mindist) return;                                                 // :334
    const double x = ((double)u - f.cx) * depth / f.fx, y = ((double)v - f.cy) * depth / f.fy, z = depth; // :337-339
    double p[3];
    for (int i = 0; i < 3; i++) p[i] = ((f.R[3 * i] * x + f.R[3 * i + 1] * y) + f.R[3 * i + 2] * z) + f.t[i]; // :340
    if (f.last) { // :382-419
        const double q[3] = {p[0] - f.lt[0], p[1] - f.lt[1], p[2] - f.lt[2]};
        double r[3];
        for (int i = 0; i < 3; i++) r[i] = (f.Ri[3 * i] * q[0] + f.Ri[3 * i + 1] * q[1]) + f.Ri[3 * i + 2] * q[2];
        const double uu = r[0] * f.fx / r[2] + f.cx, vv = r[1] * f.fy / r[2] + f.cy; // :383-384
        if (uu >= 0 && uu < f.cols && vv >= 0 && vv < f.rows) {                      // :385; outside: a new point, kept
            const double drift = fabs((double)f.last[(size_t)(int)vv * f.cols + (int)uu] / f.depth_scale - r[2]); // :387
            if (!(drift < f.tol)) return;                                            // :389
        }
    }
    end_lane(g, f, w, n, p);
}

__device__ inline void setup_lane(const Geo &g, const Frame &f, const Ws &w, int n)
{
    if (n >= f.N) return;
    const int e = w.endv[n];
    if (e == NO_RAY || (e >= 0 && w.owner[e] != n)) return; // :470-478
    atomicAdd(&w.hdr[H_NRAYS], 1);
    const int full = walk(g, f, w.pts + 3 * (size_t)n, f.nb, [](int) { return false; });
    if (full < 0) return; // :484-489
    w.cnt[n] = full;
    w.list[atomicAdd(&w.hdr[H_NLIST], 1)] = n;
}

__device__ inline void mark_lane(const Geo &g, const Frame &f, const Ws &w, int round, int s)
{
    if (s >= w.hdr[H_NLIST]) return;
    const int n = w.list[s];
    const unsigned key = ((unsigned)(MAX_ROUNDS - round) << 24) | (unsigned)n;
    unsigned *mark = w.mark;
    walk(g, f, w.pts + 3 * (size_t)n, w.cnt[n], [=](int v) {
        if (v >= 0) atomicMin(&mark[v], key);
        return false;
    });
}

__device__ inline void stop_lane(const Geo &g, const Frame &f, const Ws &w, int round, int s)
{
    if (s >= w.hdr[H_NLIST]) return;
    const int n = w.list[s];
    const unsigned tag = (unsigned)(MAX_ROUNDS - round);
    const unsigned *mark = w.mark;
    int prev = OUTSIDE;
    const int c = walk(g, f, w.pts + 3 * (size_t)n, f.nb, [&](int v) {
        if (v < 0) return false;
        const unsigned m = mark[v];
        if (((m >> 24) == tag && (int)(m & 0xFFFFFFu) < n) || v == prev) return true; // :497-498, after the cell was counted
        prev = v;
        return false;
    });
    if (c != w.cnt[n]) {
        w.cnt[n] = c;
        w.hdr[round] = 1;
    }
}

// rounds used / minus the cap and rays cast into status[0 .. 1]; whether the frame converged
__device__ inline void status_lane(const Frame &f, const Ws &w)
{
    int rounds = -f.max_rounds;
    for (int r = 1; r <= f.max_rounds; r++)
        if (w.hdr[r] == 0) { rounds = r; break; }
    w.hdr[H_CONVERGED] = rounds > 0 ? 1 : 0;
    f.status[0] = rounds;
    f.status[1] = w.hdr[H_NRAYS];
}

__device__ inline void count_lane(const Geo &g, const Frame &f, const Ws &w, int s)
{
    if (s >= w.hdr[H_NLIST]) return;
    const int n = w.list[s];
    int *all = w.all;
    walk(g, f, w.pts + 3 * (size_t)n, w.cnt[n], [=](int v) {
        if (v >= 0) atomicAdd(&all[v], 1); // setCacheOccupancy(tmp, 0), :493
        return false;
    });
}

// The batch update (:512-531) of a voxel that a frame counted `all` > 0 times, `hit` of them as a ray end, on the value `val`.
// false: skipped at the clamp (:516-518), nothing is written.
__device__ inline bool update_value(const Frame &f, int all, int hit, double &val)
{
    const double upd = hit >= all - hit ? f.hit_log : f.miss_log;           // :512-513
    if ((upd >= 0 && val >= f.cmax) || (upd <= 0 && val <= f.cmin)) return false; // :516-518
    double nv = val + upd;                                                 // :530-531: std::min(std::max(. , clamp_min), clamp_max)
    nv = nv < f.cmin ? f.cmin : nv;
    nv = f.cmax < nv ? f.cmax : nv;
    val = nv;
    return true;
}

// voxel (x, y, z) takes the value nv: log_odds, occ and its bit of the plane together
__device__ inline void write_voxel(const Geo &g, int x, int y, int z, double nv, double *log_odds, unsigned char *occ, uint32_t *plane)
{
    const size_t col = (size_t)x * g.grid[1] + y, idx = col * g.grid[2] + z;
    log_odds[idx] = nv;
    const unsigned char o = nv > g.thr ? 1 : 0;
    occ[idx] = o;
    uint32_t *word = plane + col * g.wz + (z >> 5);
    if (o) atomicOr(word, 1u << (z & 31));
    else atomicAnd(word, ~(1u << (z & 31)));
}

// ---- the pose: what is computed once per frame, on the host for the single-frame call and by one lane per frame for the batch ----

// last_T_wc.block<3,3>(0,0).inverse() (:382) as adjugate / determinant, in the order tests/occmap_fusion_oracle.py inverse3 writes down
__host__ __device__ inline bool inverse3(const double *T, double *Ri)
{
    double C[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            C[i][j] = T[4 * i1 + j1] * T[4 * i2 + j2] - T[4 * i1 + j2] * T[4 * i2 + j1];
        }
    const double det = (T[0] * C[0][0] + T[1] * C[0][1]) + T[2] * C[0][2];
    if (!finite_all(&det, 1) || det == 0.0) return false;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Ri[3 * i + j] = C[j][i] / det;
    return finite_all(Ri, 9);
}

// R, t, last_R^-1 and last_t of a frame from its row-major 4 x 4 poses (last_T_wc only with f.last); false: a pose that is refused
__host__ __device__ inline bool set_pose(Frame &f, const double *T_wc, const double *last_T_wc)
{
    if (!finite_all(T_wc, 16)) return false;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) { f.R[3 * i + j] = T_wc[4 * i + j]; f.Ri[3 * i + j] = 0.0; }
        f.t[i] = T_wc[4 * i + 3]; f.lt[i] = 0.0;
    }
    if (f.last) {
        if (!finite_all(last_T_wc, 16) || !inverse3(last_T_wc, f.Ri)) return false;
        for (int i = 0; i < 3; i++) f.lt[i] = last_T_wc[4 * i + 3];
    }
    return true;
}

// the ray box: posToIndex(t -/+ max_ray_length) with two voxels of slack, clamped to the map; returns its size
__host__ __device__ inline size_t set_ray_box(Frame &f, const Geo &g)
{
    size_t nbox = 1;
    for (int k = 0; k < 3; k++) {
        int a = clamp_id(floored(f.t[k] - f.max_len, g.origin[k], g.res_inv)) - 2, e = clamp_id(floored(f.t[k] + f.max_len, g.origin[k], g.res_inv)) + 3;
        a = a < 0 ? 0 : a > g.grid[k] ? g.grid[k] : a;
        e = e > g.grid[k] ? g.grid[k] : e;
        e = e < a ? a : e;
        f.box[k] = a; f.box[3 + k] = e; f.bd[k] = e - a;
        nbox *= (size_t)f.bd[k];
    }
    return nbox;
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

struct Plan {
    Frame f;
    size_t nbmax, off[9], bytes;
};

// What every route's description shares -- N points per frame, the increments, the ray lengths, the round cap: fills those fields of
// the frame description (not the image's, not R, t, Ri, lt, the ray box) and the workspace layout.  nbmax, the bound on the ray
// box's size whatever the sensor position, sizes the per-voxel arrays.
inline bool plan_rays(const frp_nmpc_occmap *m, long long N, double hit_log, double miss_log, double min_len, double max_len, int max_rounds, Plan *out)
{
    if (!valid(m)) return false;
    const double par[4] = {hit_log, miss_log, min_len, max_len};
    if (!finite_all(par, 4) || max_len < min_len) return false;
    if (max_rounds < 0 || max_rounds > MAX_ROUNDS) return false;
    const double cells = std::ceil(max_len / m->resolution);
    double nb;
    if (!step_bound(max_len, m->resolution, &nb)) return false;
    if (N < 0 || N > MAX_PIXELS) return false;
    Frame &f = out->f;
    f.N = (int)N;
    f.depth = nullptr; f.last = nullptr; f.status = nullptr;
    f.hit_log = hit_log; f.miss_log = miss_log; f.min_len = min_len; f.max_len = max_len;
    f.cmin = m->clamp_min_log; f.cmax = m->clamp_max_log;
    f.nb = nb > 0.0 ? (int)nb : 0;
    f.max_rounds = max_rounds ? max_rounds : FRP_OCCMAP_FUSE_DEFAULT_ROUNDS;
    size_t nbmax = 1;
    for (int k = 0; k < 3; k++) {
        const double cap = 2.0 * (cells > 0.0 ? cells : 0.0) + 8.0; // the box's largest extent, whatever the pose
        nbmax *= (size_t)(cap < (double)m->grid[k] ? cap : (double)m->grid[k]);
    }
    if (nbmax >= ((size_t)1 << 30)) return false;
    out->nbmax = nbmax;
    const size_t n = (size_t)f.N;
    const size_t sizes[9] = {HDR_INTS * sizeof(int), 3 * n * sizeof(double), n * sizeof(int), n * sizeof(int), n * sizeof(int),
                             nbmax * sizeof(int), nbmax * sizeof(int), nbmax * sizeof(int), nbmax * sizeof(unsigned)};
    size_t at = 0;
    for (int i = 0; i < 9; i++) { out->off[i] = at; at += up256(sizes[i]); }
    out->bytes = at;
    return true;
}

// Everything about a depth frame's description that does not involve a pose or a pointer: the image's scan and camera on top of
// plan_rays.
inline bool plan_shape(const frp_nmpc_occmap *m, int rows, int cols, const double *K, double depth_scale, double mindist, double tol, int margin,
                       int skip, double hit_log, double miss_log, double min_len, double max_len, int max_rounds, Plan *out)
{
    if (rows < 1 || cols < 1 || skip < 1 || margin < 0) return false;
    if (!finite_all(K, 9)) return false;
    const double par[3] = {depth_scale, mindist, tol};
    if (!finite_all(par, 3) || !(depth_scale > 0.0)) return false;
    const long long span_v = (long long)rows - 2LL * margin, span_u = (long long)cols - 2LL * margin; // v = margin; v < rows - margin; v += skip
    const long long nv = span_v > 0 ? (span_v + skip - 1) / skip : 0, nu = span_u > 0 ? (span_u + skip - 1) / skip : 0;
    if (!plan_rays(m, nv * nu, hit_log, miss_log, min_len, max_len, max_rounds, out)) return false;
    Frame &f = out->f;
    f.rows = rows; f.cols = cols; f.margin = margin; f.skip = skip;
    f.nu = nu > 0 ? (int)nu : 1;
    f.fx = K[0]; f.cx = K[2]; f.fy = K[4]; f.cy = K[5];
    f.depth_scale = depth_scale; f.mindist = mindist; f.tol = tol;
    return true;
}

// ---- a batch of frames in one call: what frp_occmap_fuse_batch.hip and frp_occmap_fuse_points.hip share ----
namespace batch {

struct Desc {
    Frame f;
    int live;  // active and not refused: the frame runs the stages
    int fused; // live and converged: the frame takes part in the update (written by the status stage)
};

struct Batch {
    Desc *desc;   // [frames], at the start of the workspace
    char *slices; // frame k's arrays: ws_at(slices + k * slice, off)
    size_t slice, off[9];
    int frames;
};

__device__ inline Ws ws_of(const Batch &b, int k) { return ws_at(b.slices + (size_t)k * b.slice, b.off); }

// voxel (x, y, z) of the map in frame f's ray box: its index there, or OUTSIDE
__device__ inline int in_box(const Frame &f, int x, int y, int z)
{
    if (x < f.box[0] || x >= f.box[3] || y < f.box[1] || y >= f.box[4] || z < f.box[2] || z >= f.box[5]) return OUTSIDE;
    return ((x - f.box[0]) * f.bd[1] + (y - f.box[1])) * f.bd[2] + (z - f.box[2]);
}

// The ordered update, lane (j, i) = (blockIdx.y, the lane's index along x): voxel i of frame j's ray box.  A voxel is owned by the first fused frame whose box holds it; the owner applies
// the update of :512-531 for frames j, j + 1, ... in order on a value carried in a register and writes it once.  The descriptors are
// read through addresses that are the same for every lane of a workgroup (scalar loads); the per-voxel reads (all, hit, log_odds)
// run along z, the fastest index of the boxes and of the map alike.
__device__ inline void update_lane(const Batch &b, const Geo &g, double *log_odds, unsigned char *occ, uint32_t *plane)
{
    const int j = blockIdx.y;
    const Desc *desc = b.desc;
    if (!desc[j].fused) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const Frame &fj = desc[j].f;
    if (i >= fj.nbox) return;
    const int z = fj.box[2] + i % fj.bd[2], y = fj.box[1] + (i / fj.bd[2]) % fj.bd[1], x = fj.box[0] + i / (fj.bd[2] * fj.bd[1]);
    for (int k = 0; k < j; k++)
        if (desc[k].fused && in_box(desc[k].f, x, y, z) >= 0) return; // frame k's lane owns this voxel
    double v = 0.0;
    bool loaded = false, wrote = false;
    for (int k = j; k < b.frames; k++) {
        if (!desc[k].fused) continue;
        const Frame &fk = desc[k].f;
        const int ik = k == j ? i : in_box(fk, x, y, z);
        if (ik < 0) continue;
        const Ws w = ws_of(b, k);
        const int all = w.all[ik];
        if (all == 0) continue; // not in frame k's cache_voxel_
        if (!loaded) { v = log_odds[((size_t)x * g.grid[1] + y) * g.grid[2] + z]; loaded = true; }
        if (update_value(fk, all, w.hit[ik], v)) wrote = true;
    }
    if (wrote) write_voxel(g, x, y, z, v, log_odds, occ, plane);
}

struct BatchPlan {
    Plan p;
    size_t desc_bytes, bytes;
};

// the workspace of `frames` frames of the planned shape: the descriptors, then one slice per frame
inline void plan_slices(BatchPlan *bp, int frames)
{
    bp->desc_bytes = up256((size_t)frames * sizeof(Desc));
    bp->bytes = bp->desc_bytes + (size_t)frames * bp->p.bytes;
}

// the batch laid out in the caller's fuse workspace; false: no workspace, too small a one or a misaligned one
inline bool batch_at(void *fuse_workspace, size_t fuse_workspace_bytes, const BatchPlan &bp, int frames, Batch *b)
{
    if (!fuse_workspace || fuse_workspace_bytes < bp.bytes || ((uintptr_t)fuse_workspace & 7) != 0) return false;
    b->desc = static_cast<Desc *>(fuse_workspace);
    b->slices = static_cast<char *>(fuse_workspace) + bp.desc_bytes;
    b->slice = bp.p.bytes;
    for (int i = 0; i < 9; i++) b->off[i] = bp.p.off[i];
    b->frames = frames;
    return true;
}

// 256-lane workgroups over n lanes per frame: a frame's count and box are known on the device only, the grids take their bounds
inline dim3 blocks(const Batch &b, size_t n) { return dim3((unsigned)((n > 0 ? n : 1) + 255) / 256, (unsigned)b.frames); }

// The launches every route shares, around its own first stage (describe, then project or load, which fill the descriptors and the
// rays' ends): init after describe; then setup, the mark / stop rounds, status, count and the ordered update.  With the route's two
// that is 2 * max_rounds + 7 launches.  The kernels are frp_occmap_fuse_batch.hip's, the only copy in the library.
void launch_init(const Batch &b, const Plan &p, hipStream_t st);
int launch_from_setup(const Batch &b, const Plan &p, const frp_nmpc_occmap *map, void *workspace, hipStream_t st); // FRP_OK or FRP_ERR_HIP

} // namespace batch

} // namespace fuse
} // namespace occmap
} // namespace frp
