// frp_peers.hip -- frp_nmpc.h section (18): the fleet's peers.  For every vehicle, who is within a radius R of it: a neighbour grid built
// on the device from positions a period leaves there, a separation record that measures, and a peer cloud that appends the neighbours to
// the per-planner cloud the corridor reads.  No reference counterpart (the reference flies one vehicle); tests/peers_oracle.py is the
// executable statement -- brute force over all pairs, no grid -- and this file agrees with it to the bit.
//
//   * The grid is S stacked boxes of ncell = dims[0] * dims[1] * dims[2] cells; the key of a sample is s * ncell + (cz * dims[1] + cy) *
//     dims[0] + cx, so the three cells cx - 1 ... cx + 1 of a row are ONE contiguous range of `items`: the 27 surrounding cells are 9 ranges.
//   * build: five launches, stream-ordered, nothing waits on another workgroup.  clear (start <- 0); count (one thread per vehicle, its S
//     samples: the key, and the rank inside the cell that the int32 atomicAdd on the cell's counter returns -- the rank is kept, so the
//     fill needs no second atomic); sums (one workgroup per FRP_PEERS_SCAN_CHUNK = 2048 counters: their sum); scan (workgroup g adds the
//     sums of the workgroups before it -- integers, any order -- and scans its own 2048 counters exclusively, in place); fill (one thread
//     per sample: items[start[key] + rank] <- b).  The order inside a cell is the atomics' order: no result below depends on it.
//   * separation: one thread per vehicle, samples ascending.  Per sample the 18 range bounds are loaded first (independent loads), then
//     the ranges are walked; the minimum is over the key (d2, peer id), which no order of the items changes.  tick[0] is read by every
//     thread, so it advances in a launch of its own behind this one (the sensor noise's pattern).
//   * summary: launch 1, one workgroup per 256 vehicles, six eight-byte partials per workgroup; launch 2, ONE workgroup adds / compares
//     them in row order.  Integers and a minimum over the key (sep2_min, vehicle id): no order matters, the same bits every run.
//   * cloud: one wavefront per planner, four per workgroup.  The 9 ranges are flattened into one index space the lanes stride over;
//     a candidate within R goes to the wave's LDS list (ballot + prefix count), FRP_PEERS_MAX_CAND = 1024 entries of 12 bytes.  Before
//     a step that could pass the cap the list is reduced to its FRP_PEERS_MAX_NEAR = 64 smallest keys in place and goes on: the cap bounds
//     the memory, never the result.  The rank of a key is the count of smaller keys (keys are distinct: the id is part of them), so the
//     kept 64 and their order do not depend on the order of the items.  Then two passes over the <= 64 * 9 * 7 points: count, and -- where
//     the count fits P -- write.  LDS: 4 * (1024 * 12 + 64 * 12) = 52224 bytes per workgroup.  Waves of a workgroup share nothing: the
//     only synchronisation is the wavefront's own (SYNC below); there is no __syncthreads in that kernel.
//   * Every index is range-checked before the access: a cell index is formed from floor((p - origin) / cell) only after that double was
//     compared against 0 and dims (a NaN or a far position fails the comparison and never becomes an int); range bounds read from `start`
//     are clamped to [0, B * S]; an item is tested 0 <= q < B; a stage 0 <= st < N; a cloud row cloud_count + j < P.
//   * No contraction (the build passes -ffp-contract=off as well): (dx * dx + dy * dy) + dz * dz is three products and two sums.
//   * Every store is a plain C++ store from a vector lane; the only atomics are the int32 adds on cell counters; no inline assembly.
// (the walk over the 27 cells, the selection of the nearest peers and the grid's argument rules: frp_peers.hpp, shared with the peer boxes)
#include "frp_fleet.hpp"
#include "frp_peers.hpp"

namespace frp {
namespace peers {

constexpr int CHUNK = FRP_PEERS_SCAN_CHUNK;
constexpr int PER = CHUNK / THREADS;
constexpr int WORDS = FRP_PEERS_SUM_WORDS;
static_assert(CHUNK % THREADS == 0 && PER >= 1, "a thread scans PER consecutive counters");
static_assert(WORDS == FRP_PEERS_SUM_INTS + 1 && sizeof(long long) == 8 && sizeof(double) == 8, "one row is the minimum's bits and the integers");

// (int)floor((p - origin) / cell) where that is a cell of the axis, -1 otherwise: the double is compared first, so a NaN, an infinity or
// a quotient beyond int never reaches the conversion
__device__ inline int axis_cell(double p, double origin, double cell, int dim)
{
    const double f = floor((p - origin) / cell);
    return (f >= 0.0 && f < (double)dim) ? (int)f : -1;
}

__global__ __launch_bounds__(THREADS) void clear_kernel(int n1, int *start)
{
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i < n1) start[i] = 0;
}

__global__ __launch_bounds__(THREADS) void count_kernel(frp_nmpc_peers p, const double *pos, int stride, const unsigned char *active)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= p.B) return;
    const bool act = !active || active[b] != 0;
    const int ncell = ncell_of(p);
    int out = 0;
    for (int s = 0; s < p.S; s++) {
        const size_t bs = (size_t)b * p.S + s;
        int key = -1, slot = 0;
        if (act) {
            const double *row = pos + bs * stride;
            const double x = row[0], y = row[1], z = row[2];
            if (finite3(x, y, z)) {
                const int cx = axis_cell(x, p.origin[0], p.cell, p.dims[0]), cy = axis_cell(y, p.origin[1], p.cell, p.dims[1]),
                          cz = axis_cell(z, p.origin[2], p.cell, p.dims[2]);
                if (cx >= 0 && cy >= 0 && cz >= 0) key = s * ncell + (cz * p.dims[1] + cy) * p.dims[0] + cx;
            }
        }
        if (key >= 0) slot = atomicAdd(&p.start[key], 1);
        else out = 1;
        p.key[bs] = key;
        p.slot[bs] = slot;
    }
    p.outside[b] = out;
}

__device__ inline int wave_sum_i(int v)
{
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) v += __shfl_down(v, d, WAVE);
    return v; // (lane 0 holds the wave's sum)
}

// the sum of v over the workgroup, in every thread
__device__ inline int block_sum_i(int v, int *part)
{
    const int t = threadIdx.x;
    const int w = wave_sum_i(v);
    __syncthreads();
    if (t % WAVE == 0) part[t / WAVE] = w;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int i = 0; i < WAVES; i++) s += part[i];
    return s;
}

__global__ __launch_bounds__(THREADS) void sums_kernel(int n1, const int *start, int *block_sums)
{
    __shared__ int part[WAVES];
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * CHUNK;
    int v = 0;
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const long long at = base + t + (long long)i * THREADS;
        if (at < n1) v += start[at];
    }
    const int s = block_sum_i(v, part);
    if (t == 0) block_sums[blockIdx.x] = s;
}

__global__ __launch_bounds__(THREADS) void scan_kernel(int n1, int *start, const int *block_sums)
{
    __shared__ int part[WAVES];
    __shared__ int waves[WAVES];
    const int t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
    int before = 0;
    for (int g = t; g < (int)blockIdx.x; g += THREADS) before += block_sums[g];
    before = block_sum_i(before, part);
    const long long base = (long long)blockIdx.x * CHUNK + (long long)t * PER;
    int v[PER], mine = 0;
#pragma unroll
    for (int i = 0; i < PER; i++) {
        v[i] = base + i < n1 ? start[base + i] : 0;
        mine += v[i];
    }
    int incl = mine; // inclusive scan of the threads' sums inside the wave
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const int o = __shfl_up(incl, d, WAVE);
        if (lane >= d) incl += o;
    }
    if (lane == WAVE - 1) waves[wave] = incl;
    __syncthreads();
    int run = before + incl - mine;
#pragma unroll
    for (int w = 0; w < WAVES; w++)
        if (w < wave) run += waves[w];
#pragma unroll
    for (int i = 0; i < PER; i++) {
        if (base + i < n1) start[base + i] = run;
        run += v[i];
    }
}

__global__ __launch_bounds__(THREADS) void fill_kernel(frp_nmpc_peers p)
{
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    const long long n = (long long)p.B * p.S;
    if (i >= n) return;
    const int key = p.key[i];
    if (key < 0 || key >= p.S * ncell_of(p)) return;
    const long long at = (long long)p.start[key] + p.slot[i];
    if (at >= 0 && at < n) p.items[at] = (int)(i / p.S);
}

__global__ __launch_bounds__(THREADS) void separation_kernel(frp_nmpc_peers p, const double *pos, int stride, double R2, double warn2, double hit2)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= p.B) return;
    const long long now = p.tick[0];
    const int ncell = ncell_of(p), nitems = p.B * p.S;
    double best = p.sep2_min[b];
    int who = p.nearest[b], near = p.near_samples[b], hits = p.hit_samples[b], n = p.samples[b];
    long long first = p.first_hit[b];
    for (int s = 0; s < p.S; s++) {
        const size_t bs = (size_t)b * p.S + s;
        const int cid = p.key[bs] - s * ncell;
        if (cid < 0 || cid >= ncell) continue; // not entered
        n += 1;
        const int cx = cid % p.dims[0], cy = (cid / p.dims[0]) % p.dims[1], cz = cid / (p.dims[0] * p.dims[1]);
        const double *me = pos + bs * stride;
        const double mx = me[0], my = me[1], mz = me[2];
        int lo[9], hi[9];
#pragma unroll
        for (int r = 0; r < 9; r++) range_of(p, s, ncell, nitems, cx, cy, cz, r, lo[r], hi[r]);
        double m = INFINITY;
        int mp = INT_MAX;
        bool is_near = false, is_hit = false;
#pragma unroll
        for (int r = 0; r < 9; r++) {
            for (int j = lo[r]; j < hi[r]; j++) {
                const int q = p.items[j];
                if (q < 0 || q >= p.B || q == b) continue;
                const double *o = pos + ((size_t)q * p.S + s) * stride;
                const double d2 = sq3(mx - o[0], my - o[1], mz - o[2]);
                if (d2 <= R2) {
                    if (d2 < m || (d2 == m && q < mp)) { m = d2; mp = q; }
                    if (d2 <= warn2) is_near = true;
                    if (d2 <= hit2) is_hit = true;
                }
            }
        }
        if (mp != INT_MAX && m < best) { best = m; who = mp; }
        if (is_near) near += 1;
        if (is_hit) {
            hits += 1;
            if (first < 0) first = now;
        }
    }
    p.sep2_min[b] = best; p.nearest[b] = who; p.near_samples[b] = near; p.hit_samples[b] = hits; p.samples[b] = n; p.first_hit[b] = first;
}

// tick[0] += advance: launched after the kernel whose threads read it
__global__ void tick_kernel(long long *tick, int advance)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) tick[0] = (long long)((unsigned long long)tick[0] + (unsigned long long)(long long)advance);
}

__global__ __launch_bounds__(THREADS) void reset_kernel(frp_nmpc_peers p, const int *mask, double R2)
{
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= p.B) return;
    if (mask && mask[b] == 0) return;
    p.sep2_min[b] = R2; p.nearest[b] = -1; p.near_samples[b] = 0; p.hit_samples[b] = 0; p.samples[b] = 0; p.first_hit[b] = -1;
}

__device__ inline long long wave_sum_ll(long long v)
{
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) v += __shfl_down(v, d, WAVE);
    return v;
}

// launch 1: the partials of workgroup g over vehicles 256 g ... 256 g + 255 into row g of the workspace
__global__ __launch_bounds__(THREADS) void summary_partial_kernel(frp_nmpc_peers p, const int *mask, long long *ws)
{
    __shared__ long long wi[WAVES][FRP_PEERS_SUM_INTS];
    __shared__ double wd[WAVES];
    const int t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
    const int b = blockIdx.x * THREADS + t;
    const bool sel = b < p.B && (!mask || mask[b] != 0);
    double d = INFINITY;
    int id = INT_MAX;
    long long vi[FRP_PEERS_SUM_INTS] = {0, 0, 0, 0, 0};
    if (sel) {
        const int h = p.hit_samples[b];
        d = p.sep2_min[b]; id = b;
        vi[FRP_PEERS_I_WITH_HITS] = h > 0; vi[FRP_PEERS_I_NEAR] = p.near_samples[b]; vi[FRP_PEERS_I_HIT] = h; vi[FRP_PEERS_I_SAMPLES] = p.samples[b];
    }
#pragma unroll
    for (int k = WAVE / 2; k >= 1; k >>= 1) {
        const double e = __shfl_down(d, k, WAVE);
        const int j = __shfl_down(id, k, WAVE);
        if (before(e, j, d, id)) { d = e; id = j; }
    }
#pragma unroll
    for (int i = 1; i < FRP_PEERS_SUM_INTS; i++) {
        const long long s = wave_sum_ll(vi[i]);
        if (lane == 0) wi[wave][i] = s;
    }
    if (lane == 0) { wd[wave] = d; wi[wave][FRP_PEERS_I_NEAREST] = id; }
    __syncthreads();
    long long *row = ws + (size_t)blockIdx.x * WORDS;
    if (t == 0) {
        double e = wd[0];
        int j = (int)wi[0][FRP_PEERS_I_NEAREST];
#pragma unroll
        for (int w = 1; w < WAVES; w++)
            if (before(wd[w], (int)wi[w][FRP_PEERS_I_NEAREST], e, j)) { e = wd[w]; j = (int)wi[w][FRP_PEERS_I_NEAREST]; }
        reinterpret_cast<double *>(row)[FRP_PEERS_SUM_INTS] = e;
        row[FRP_PEERS_I_NEAREST] = j;
    } else if (t < FRP_PEERS_SUM_INTS) {
        long long s = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) s += wi[w][t];
        row[t] = s;
    }
}
static_assert(FRP_PEERS_I_NEAREST == 0, "thread 0 of the partial kernel writes the key, threads 1 ... the sums");

// launch 2, ONE workgroup: thread t takes word t of rows 0 ... G - 1 in that order
__global__ __launch_bounds__(THREADS) void summary_final_kernel(int G, const long long *ws, long long *out_i, double *out_f)
{
    const int t = threadIdx.x;
    if (t == 0) {
        double d = INFINITY;
        int id = INT_MAX;
        for (int g = 0; g < G; g++) {
            const double e = reinterpret_cast<const double *>(ws)[(size_t)g * WORDS + FRP_PEERS_SUM_INTS];
            const int j = (int)ws[(size_t)g * WORDS + FRP_PEERS_I_NEAREST];
            if (before(e, j, d, id)) { d = e; id = j; }
        }
        out_f[0] = d;
        out_i[FRP_PEERS_I_NEAREST] = id == INT_MAX ? -1 : id;
    } else if (t < FRP_PEERS_SUM_INTS) {
        long long s = 0;
        for (int g = 0; g < G; g++) s += ws[(size_t)g * WORDS + t];
        out_i[t] = s;
    }
}

// point t of planner b's emission order: kept peer t / (nc * per), centre (t / per) % nc, point t % per.  False where it is dropped.
__device__ inline bool peer_point(const frp_nmpc_peers &p, const frp_nmpc_peers_view &v, const double *pos, int stride, const int *kp, int nc, int per, int t,
                                  const double lo[3], const double hi[3], double q[3])
{
    const int peer = kp[t / (nc * per)], c = (t / per) % nc, k = t % per;
    if (peer < 0 || peer >= p.B) return false;
    const double *src;
    if (c == 0) {
        src = pos + (size_t)peer * stride;
    } else {
        if (v.have_traj[peer] == 0) return false;
        const int st = v.stages[c - 1];
        if (st < 0 || st >= v.N) return false;
        src = v.pre_plan + ((size_t)peer * v.N + st) * ROW + 8;
    }
    q[0] = src[0]; q[1] = src[1]; q[2] = src[2];
    if (k > 0) {
        const int axis = (k - 1) / 2;
        const double moved = (k - 1) % 2 == 0 ? q[axis] + v.r_body : q[axis] - v.r_body;
        if (axis == 0) q[0] = moved;
        else if (axis == 1) q[1] = moved;
        else q[2] = moved;
    }
    if (!finite3(q[0], q[1], q[2])) return false;
    return lo[0] <= q[0] && q[0] < hi[0] && lo[1] <= q[1] && q[1] < hi[1] && lo[2] <= q[2] && q[2] < hi[2];
}

__global__ __launch_bounds__(THREADS) void cloud_kernel(frp_nmpc_peers p, frp_nmpc_peers_view v, const double *pos, int stride, double R2)
{
    __shared__ double cand_d[WAVES][CAND];
    __shared__ int cand_p[WAVES][CAND];
    __shared__ double kept_d[WAVES][NEAR];
    __shared__ int kept_p[WAVES][NEAR];
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    const int b = blockIdx.x * WAVES + wave; // (uniform in the wave)
    if (b >= p.B) return;
    double *cd = cand_d[wave], *kd = kept_d[wave];
    int *cp = cand_p[wave], *kp = kept_p[wave];
    const int cc = v.cloud_count[b];
    if (cc < 0) { // the map's cloud already overflowed: the planner is left as it is
        if (lane == 0) { v.added[b] = 0; v.overflow[b] = 0; }
        return;
    }
    // (this selection is select_near of frp_peers.hpp, stated here as it was: called as that function the kernel came out with other bytes.
    //  KEEP IN STEP: an edit here is an edit there)
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
    const int m = keep_smallest(cd, cp, kd, kp, n, lane);
    const int nc = 1 + v.K, per = v.r_body == 0.0 ? 1 : 7;
    const int slots = m * nc * per;
    const int *box = v.local_box + (size_t)b * 6;
    double lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        lo[k] = v.origin[k] + (double)box[k] * v.resolution;
        hi[k] = v.origin[k] + (double)box[3 + k] * v.resolution;
    }
    int add = 0;
    for (int t0 = 0; t0 < slots; t0 += WAVE) {
        double q[3];
        const bool ok = t0 + lane < slots && peer_point(p, v, pos, stride, kp, nc, per, t0 + lane, lo, hi, q);
        add += (int)__popcll(__ballot(ok));
    }
    const bool fits = cc + add <= v.P;
    if (fits) {
        int at0 = cc;
        for (int t0 = 0; t0 < slots; t0 += WAVE) {
            double q[3];
            const bool ok = t0 + lane < slots && peer_point(p, v, pos, stride, kp, nc, per, t0 + lane, lo, hi, q);
            const unsigned long long mask = __ballot(ok);
            const int at = at0 + (int)__popcll(mask & ((1ull << lane) - 1ull));
            if (ok && at >= 0 && at < v.P) {
                double *dst = v.cloud + ((size_t)b * v.P + at) * 3;
                dst[0] = q[0]; dst[1] = q[1]; dst[2] = q[2];
            }
            at0 += (int)__popcll(mask);
        }
    }
    if (lane == 0) {
        v.cloud_count[b] = fits ? cc + add : -(cc + add);
        v.added[b] = add;
        v.overflow[b] = seen > NEAR ? 1 : 0;
    }
}

// ---- host: the argument rules ----

static bool record_ok(const frp_nmpc_peers *p)
{
    return p->sep2_min && p->nearest && p->near_samples && p->hit_samples && p->samples && p->first_hit && p->tick && p->sum_ws &&
           non_negative(p->d_hit) && p->d_hit <= p->d_warn && p->d_warn <= p->R;
}

} // namespace peers
} // namespace frp

extern "C" {

int frp_nmpc_peers_build(const frp_nmpc_peers *p, const double *pos, int stride, const unsigned char *active, void *stream)
{
    using namespace frp::peers;
    if (!grid_ok(p) || !pos_ok(p, pos, stride)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (p->B == 0) return FRP_OK;
    const int n1 = p->S * p->dims[0] * p->dims[1] * p->dims[2] + 1;
    const unsigned chunks = (unsigned)((n1 + CHUNK - 1) / CHUNK);
    if (launch(clear_kernel, blocks_for(n1), stream, n1, p->start) != FRP_OK) return FRP_ERR_HIP;
    if (launch(count_kernel, blocks_for(p->B), stream, *p, pos, stride, active) != FRP_OK) return FRP_ERR_HIP;
    if (launch(sums_kernel, chunks, stream, n1, (const int *)p->start, p->block_sums) != FRP_OK) return FRP_ERR_HIP;
    if (launch(scan_kernel, chunks, stream, n1, p->start, (const int *)p->block_sums) != FRP_OK) return FRP_ERR_HIP;
    return launch(fill_kernel, blocks_for((long long)p->B * p->S), stream, *p);
}

int frp_nmpc_peers_separation(const frp_nmpc_peers *p, const double *pos, int stride, int advance, void *stream)
{
    using namespace frp::peers;
    if (!grid_ok(p) || !record_ok(p) || !pos_ok(p, pos, stride) || advance < 0) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (p->B == 0) return FRP_OK;
    if (launch(separation_kernel, blocks_for(p->B), stream, *p, pos, stride, p->R * p->R, p->d_warn * p->d_warn, p->d_hit * p->d_hit) != FRP_OK)
        return FRP_ERR_HIP;
    hipLaunchKernelGGL(tick_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), p->tick, advance);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

int frp_nmpc_peers_reset(const frp_nmpc_peers *p, const int *mask, void *stream)
{
    using namespace frp::peers;
    if (!p || p->B < 0 || !positive(p->R) || !record_ok(p)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (p->B == 0) return FRP_OK;
    return launch(reset_kernel, blocks_for(p->B), stream, *p, mask, p->R * p->R);
}

int frp_nmpc_peers_summary(const frp_nmpc_peers *p, const int *mask, long long *out_i, double *out_f, void *stream)
{
    using namespace frp::peers;
    if (!p || p->B < 0 || !positive(p->R) || !record_ok(p) || !out_i || !out_f) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    const unsigned G = blocks_for(p->B);
    if (G > 0 && launch(summary_partial_kernel, G, stream, *p, mask, p->sum_ws) != FRP_OK) return FRP_ERR_HIP;
    return launch(summary_final_kernel, 1, stream, (int)G, (const long long *)p->sum_ws, out_i, out_f);
}

int frp_nmpc_peers_cloud(const frp_nmpc_peers *p, const frp_nmpc_peers_view *v, const double *pos, int stride, void *stream)
{
    using namespace frp::peers;
    if (!grid_ok(p) || p->S != 1 || !pos_ok(p, pos, stride) || !v) return FRP_ERR_ARG;
    if (v->N < 1 || v->K < 0 || v->K > FRP_PEERS_MAX_STAGES || v->P < 0 || !non_negative(v->r_body) || !positive(v->resolution)) return FRP_ERR_ARG;
    if (!finite_d(v->origin[0]) || !finite_d(v->origin[1]) || !finite_d(v->origin[2])) return FRP_ERR_ARG;
    if (!v->pre_plan || !v->have_traj || (v->K > 0 && !v->stages) || !v->local_box || (v->P > 0 && !v->cloud) || !v->cloud_count || !v->added || !v->overflow)
        return FRP_ERR_ARG;
    if ((long long)p->B * v->N * ROW > 0x7fffffffLL) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (p->B == 0) return FRP_OK;
    return launch(cloud_kernel, (unsigned)((p->B + WAVES - 1) / WAVES), stream, *p, *v, pos, stride, p->R * p->R);
}

} // extern "C"
