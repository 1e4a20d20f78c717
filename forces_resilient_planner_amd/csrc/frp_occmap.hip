// frp_nmpc.h section (8): the occupancy map of the reference (OccMap, occ_grid/src/occ_map.cpp) in device memory, and the
// views its three consumers take: the A*'s byte grid and local box, the corridor's local obstacle cloud, point queries.
//
//   * log_odds [gx][gy][gz] double is the reference's occupancy_buffer_ (index x * gy * gz + y * gz + z, :104); occ is the byte
//     view `log_odds > min_occupancy_log` that frp_nmpc_astar.occ takes.
//   * next to them, in the caller's workspace, a bit plane: WZ = ceil(gz / 32) 32-bit words per (x, y) column, bit z % 32 of word
//     z / 32 = occ[x][y][z].  It is 1/64 of the double buffer (1.0 MB for the reference's 400 x 400 x 50 map) and stays in L2, so
//     a local view of 4096 planners reads it instead of 4096 x 0.9 M doubles.
//   * local view: one workgroup per planner, one column per lane and tile of 256 columns in the reference's x-y loop order; a
//     lane masks its column's words to the z range and counts bits, a wavefront scan + four wave totals give every lane the index
//     of its first point, and the running total carries over to the next tile.  No atomics on the output: the order is the
//     reference's x, y, z loop order by construction (occ_map.cpp:192-194).
//   * every index and centre is the reference's sequence of IEEE operations (this file is compiled with -ffp-contract=off, like
//     the A*): floor((p - origin) * (1 / resolution)) and origin + (id + 0.5) * resolution, the latter rounded to float and widened
//     (pcl::PointXYZ).
//   * where the reference converts a double to int without looking (NaN, beyond int: undefined there), the tests are made on the
//     floored double: such a point is outside the map, such a local range is clamped like any other.
#include "frp_occmap.hpp"

namespace frp {
namespace occmap {

constexpr int LV_THREADS = 256;

// fill: log_odds and occ of every voxel (OccMap::init, :831)
__global__ __launch_bounds__(256) void fill_kernel(double *log_odds, unsigned char *occ, size_t n, double v, unsigned char o)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        log_odds[i] = v;
        occ[i] = o;
    }
}

// occ <- log_odds > min_occupancy_log (the test of :105, :159, :196)
__global__ __launch_bounds__(256) void threshold_kernel(const double *log_odds, unsigned char *occ, size_t n, double thr)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) occ[i] = log_odds[i] > thr ? 1 : 0;
}

// plane <- occ: one lane per 32-bit word of a column (the A*'s pack_map_kernel with narrower words, so that insert can use 32-bit atomics)
__global__ __launch_bounds__(256) void pack_kernel(const unsigned char *occ, size_t cols, int gz, int wz, uint32_t *plane)
{
    const size_t words = cols * (size_t)wz;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
        const size_t col = i / wz;
        const int z0 = (int)(i % wz) * 32, z1 = z0 + 32 < gz ? z0 + 32 : gz;
        const unsigned char *c = occ + col * gz;
        uint32_t w = 0;
        for (int z = z0; z < z1; z++) w |= c[z] ? (1u << (z - z0)) : 0u;
        plane[i] = w;
    }
}

// resetBuffer's loops (:30-35) over an index box that the host clamped into the map
__global__ __launch_bounds__(256) void clear_box_kernel(double *log_odds, unsigned char *occ, Geo g, int x0, int y0, int z0, int nx, int ny, int nz, double v, unsigned char o)
{
    const size_t n = (size_t)nx * ny * nz;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int z = z0 + (int)(i % nz), y = y0 + (int)((i / nz) % ny), x = x0 + (int)(i / ((size_t)nz * ny));
        const size_t idx = ((size_t)x * g.grid[1] + y) * g.grid[2] + z;
        log_odds[idx] = v;
        occ[idx] = o;
    }
}

// setOccupancy (:84-93) for every point of a pcl::PointXYZ cloud (globalCloudCallback, :612-619).  All writers of a voxel store the same values.
__global__ __launch_bounds__(256) void insert_kernel(const float *pts, int P, Geo g, double *log_odds, unsigned char *occ, uint32_t *plane, double v, unsigned char o)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    int id[3];
    for (int k = 0; k < 3; k++) {
        const double f = floored((double)pts[3 * (size_t)i + k], g.origin[k], g.res_inv);
        if (!(f >= 0.0 && f <= (double)(g.grid[k] - 1))) return; // isInMap (:66-69); a NaN fails both comparisons
        id[k] = (int)f;
    }
    const size_t col = (size_t)id[0] * g.grid[1] + id[1], idx = col * g.grid[2] + id[2];
    log_odds[idx] = v;
    occ[idx] = o;
    uint32_t *w = plane + col * g.wz + (id[2] >> 5);
    if (o) atomicOr(w, 1u << (id[2] & 31));
    else atomicAnd(w, ~(1u << (id[2] & 31)));
}

struct View {
    int B, P;
    const double *centre; // null: the whole map
    double radius[3];
    int *local_box;
    double *cloud;
    int *count;
};

// isInLocalMap's min_id / max_id (:47-55) around a centre (local_range_min_ / max_ = centre -/+ sensor_range_, :273-274, :580-581)
__device__ inline void local_ids(const Geo &g, const View &v, int b, int *lo, int *hi)
{
    for (int k = 0; k < 3; k++) {
        if (!v.centre) { lo[k] = 0; hi[k] = g.grid[k]; continue; }
        const double c = v.centre[3 * (size_t)b + k];
        const double rmin = c - v.radius[k], rmax = c + v.radius[k];
        const int a = clamp_id(floored(rmin, g.origin[k], g.res_inv)), e = clamp_id(floored(rmax, g.origin[k], g.res_inv));
        lo[k] = a > 0 ? a : 0;
        hi[k] = e < g.grid[k] ? e : g.grid[k];
    }
}

// localOccVisCallback (:181-206) / globalOccVisCallback (:153-167) for planner blockIdx.x
__global__ __launch_bounds__(LV_THREADS) void local_view_kernel(Geo g, View v, const uint32_t *plane)
{
    __shared__ int s_wave[2][LV_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int lo[3], hi[3];
    local_ids(g, v, b, lo, hi);
    if (v.local_box && tid < 6) v.local_box[6 * (size_t)b + tid] = tid < 3 ? lo[tid] : hi[tid - 3];
    if (!v.count) return;
    // the loops run x, y, z from min_id to max_id EXCLUSIVE (:192-194); max_id <= grid_size, min_id >= 0: every index is in the map
    const int nx = hi[0] > lo[0] ? hi[0] - lo[0] : 0, ny = hi[1] > lo[1] ? hi[1] - lo[1] : 0, nz = hi[2] > lo[2] ? hi[2] - lo[2] : 0;
    const int ncols = nz > 0 ? nx * ny : 0;
    double *out = v.cloud + (size_t)b * v.P * 3;
    int base = 0;
    for (int t0 = 0, it = 0; t0 < ncols; t0 += LV_THREADS, it ^= 1) {
        const int c = t0 + tid;
        int x = 0, y = 0, cnt = 0;
        const uint32_t *w = nullptr;
        if (c < ncols) {
            x = lo[0] + c / ny; y = lo[1] + c % ny;
            w = plane + ((size_t)x * g.grid[1] + y) * g.wz;
            for (int k = lo[2] >> 5; k <= (hi[2] - 1) >> 5; k++) {
                uint32_t m = w[k];
                const int zb = k << 5;
                if (lo[2] > zb) m &= ~0u << (lo[2] - zb);
                if (hi[2] < zb + 32) m &= ~0u >> (zb + 32 - hi[2]);
                cnt += __popc(m);
            }
        }
        int inc = cnt; // inclusive scan over the wavefront
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) s_wave[it][wave] = inc;
        __syncthreads(); // (the other buffer is written next: one barrier per tile)
        int before = 0, total = 0;
        for (int k = 0; k < LV_THREADS / 64; k++) {
            const int s = s_wave[it][k];
            before += k < wave ? s : 0;
            total += s;
        }
        int at = base + before + inc - cnt;
        if (cnt > 0 && at < v.P) {
            const double px = (double)(float)(g.origin[0] + ((double)x + 0.5) * g.res); // indexToPos (:77-82), pcl::PointXYZ (:203)
            const double py = (double)(float)(g.origin[1] + ((double)y + 0.5) * g.res);
            for (int k = lo[2] >> 5; k <= (hi[2] - 1) >> 5; k++) {
                uint32_t m = w[k];
                const int zb = k << 5;
                if (lo[2] > zb) m &= ~0u << (lo[2] - zb);
                if (hi[2] < zb + 32) m &= ~0u >> (zb + 32 - hi[2]);
                while (m && at < v.P) {
                    const int z = zb + __ffs(m) - 1;
                    m &= m - 1;
                    double *o = out + 3 * (size_t)at;
                    o[0] = px; o[1] = py;
                    o[2] = (double)(float)(g.origin[2] + ((double)z + 0.5) * g.res);
                    at++;
                }
            }
        }
        base += total;
    }
    if (tid == 0) v.count[b] = base > v.P ? -base : base; // more than P occupied voxels: the first P are kept, the true count is negated
}

// getVoxelState(pos) (:95-106)
__global__ __launch_bounds__(256) void query_kernel(Geo g, int Q, const double *pos, const int *planner, const int *local_box, const unsigned char *occ, int *state)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    int id[3];
    bool in_map = true;
    for (int k = 0; k < 3; k++) {
        const double f = floored(pos[3 * (size_t)q + k], g.origin[k], g.res_inv);
        in_map = in_map && f >= 0.0 && f <= (double)(g.grid[k] - 1);
        id[k] = in_map ? (int)f : 0;
    }
    if (!in_map) { state[q] = -1; return; }
    if (local_box) { // isInLocalMap (:56): min_id <= id <= max_id, INCLUSIVE on both sides
        const int *bx = local_box + 6 * (size_t)(planner ? planner[q] : 0);
        for (int k = 0; k < 3; k++)
            if (id[k] < bx[k] || id[k] > bx[3 + k]) { state[q] = 0; return; }
    }
    state[q] = occ[((size_t)id[0] * g.grid[1] + id[1]) * g.grid[2] + id[2]] ? 1 : 0;
}

static int repack(const frp_nmpc_occmap *m, void *ws, hipStream_t st)
{
    const size_t cols = (size_t)m->grid[0] * m->grid[1];
    const int wz = (m->grid[2] + 31) / 32;
    hipLaunchKernelGGL(pack_kernel, dim3(blocks_for(cols * wz)), dim3(256), 0, st, m->occ, cols, m->grid[2], wz, static_cast<uint32_t *>(ws));
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

} // namespace occmap
} // namespace frp

extern "C" {

size_t frp_nmpc_occmap_workspace_bytes(const frp_nmpc_occmap *m)
{
    return frp::occmap::valid(m) ? frp::occmap::plane_bytes(m) : 0;
}

int frp_nmpc_occmap_reset(const frp_nmpc_occmap *m, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace frp::occmap;
    if (!args_ok(m, workspace, workspace_bytes)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)m->grid[0] * m->grid[1] * m->grid[2];
    hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(n)), dim3(256), 0, st, m->log_odds, m->occ, n, m->clamp_min_log,
                       (unsigned char)(m->clamp_min_log > m->min_occupancy_log ? 1 : 0));
    return repack(m, workspace, st);
}

int frp_nmpc_occmap_refresh(const frp_nmpc_occmap *m, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace frp::occmap;
    if (!args_ok(m, workspace, workspace_bytes)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)m->grid[0] * m->grid[1] * m->grid[2];
    hipLaunchKernelGGL(threshold_kernel, dim3(blocks_for(n)), dim3(256), 0, st, m->log_odds, m->occ, n, m->min_occupancy_log);
    return repack(m, workspace, st);
}

int frp_nmpc_occmap_clear_box(const frp_nmpc_occmap *m, const double min_pos[3], const double max_pos[3], void *workspace,
                              size_t workspace_bytes, void *stream)
{
    using namespace frp::occmap;
    if (!args_ok(m, workspace, workspace_bytes) || !min_pos || !max_pos) return FRP_ERR_ARG;
    for (int k = 0; k < 3; k++)
        if (std::isnan(min_pos[k]) || std::isnan(max_pos[k])) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    const Geo g = geo(m);
    int lo[3], n[3];
    for (int k = 0; k < 3; k++) { // resetBuffer, :17-28 (min_range_ = origin_, max_range_ = origin_ + map_size_, :800-801)
        const double min_range = m->origin[k], max_range = m->origin[k] + m->map_size[k];
        const double a = min_pos[k] < min_range ? min_range : min_pos[k], e = max_range < max_pos[k] ? max_range : max_pos[k];
        int i0 = clamp_id(floored(a, g.origin[k], g.res_inv)), i1 = clamp_id(floored(e - m->resolution / 2, g.origin[k], g.res_inv));
        // (guard: by the clamping above the loops stay inside the buffer except for rounding at the far face)
        if (i0 < 0) i0 = 0;
        if (i1 > m->grid[k] - 1) i1 = m->grid[k] - 1;
        lo[k] = i0; n[k] = i1 - i0 + 1; // x <= max_id: inclusive (:30-32)
        if (n[k] <= 0) return FRP_OK;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(clear_box_kernel, dim3(blocks_for((size_t)n[0] * n[1] * n[2])), dim3(256), 0, st, m->log_odds, m->occ, g, lo[0], lo[1], lo[2],
                       n[0], n[1], n[2], m->clamp_min_log, (unsigned char)(m->clamp_min_log > m->min_occupancy_log ? 1 : 0));
    return repack(m, workspace, st);
}

int frp_nmpc_occmap_insert_cloud(const frp_nmpc_occmap *m, const float *points, int P, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace frp::occmap;
    if (!args_ok(m, workspace, workspace_bytes) || P < 0 || (P > 0 && !points)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (P == 0) return FRP_OK;
    hipLaunchKernelGGL(insert_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), points, P, geo(m), m->log_odds,
                       m->occ, static_cast<uint32_t *>(workspace), m->clamp_max_log, (unsigned char)(m->clamp_max_log > m->min_occupancy_log ? 1 : 0));
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

int frp_nmpc_occmap_local_view(const frp_nmpc_occmap *m, const frp_nmpc_occmap_view *v, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace frp::occmap;
    if (!args_ok(m, workspace, workspace_bytes) || !v || v->B <= 0 || (!v->centre && v->B != 1)) return FRP_ERR_ARG;
    if (!v->local_box && !v->cloud_count) return FRP_ERR_ARG; // nothing asked for
    if (v->cloud_count ? (v->P < 0 || v->P > FRP_CORRIDOR_MAX_POINTS || (v->P > 0 && !v->cloud)) : v->cloud != nullptr) return FRP_ERR_ARG;
    if (v->centre)
        for (int k = 0; k < 3; k++)
            if (std::isnan(m->local_radius[k])) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    View w;
    w.B = v->B; w.P = v->P; w.centre = v->centre; w.local_box = v->local_box; w.cloud = v->cloud; w.count = v->cloud_count;
    for (int k = 0; k < 3; k++) w.radius[k] = m->local_radius[k];
    hipLaunchKernelGGL(local_view_kernel, dim3((unsigned)v->B), dim3(LV_THREADS), 0, static_cast<hipStream_t>(stream), geo(m), w,
                       static_cast<const uint32_t *>(workspace));
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

int frp_nmpc_occmap_query(const frp_nmpc_occmap *m, int Q, const double *pos, const int *planner, const int *local_box, int *state,
                          void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace frp::occmap;
    if (!args_ok(m, workspace, workspace_bytes) || Q < 0 || (Q > 0 && (!pos || !state)) || (planner && !local_box)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (Q == 0) return FRP_OK;
    hipLaunchKernelGGL(query_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), geo(m), Q, pos, planner, local_box,
                       m->occ, state);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

} // extern "C"
