// frp_nmpc.h section (8), sixth part (include/frp_nmpc_occmap_view.h): the whole-map obstacle cloud and its uniform grid rebuilt from
// the bit plane by one asynchronous call, every count read from device memory.
//
//   * ordered compaction over many workgroups WITHOUT any workgroup waiting on another: the (x, y) columns are cut into W contiguous
//     runs of whole 256-column tiles, W <= FRP_OCCMAP_VIEW_MAX_GROUPS.  Launch 1 counts each run's bits, launch 2 (one workgroup) turns
//     the W totals into exclusive bases, launch 3 re-reads each run and emits at its base with local_view_kernel's tile scan.  The
//     x, y, z order is that of local_view_kernel by construction (runs in column order, tiles in column order, lanes in column order,
//     bits from low z to high z); the order between the launches is the stream's.  No flag, no look-back, no atomics on the cloud.
//   * the plane is 1/64 of the map (1.28 MB for 400 x 400 x 50) and stays in L2: reading it twice costs less than a hand-over
//     between workgroups inside one launch would, and cannot hang.
//   * the centres are local_view_kernel's expressions (this file is compiled with -ffp-contract=off like frp_occmap.hip): the cloud
//     equals frp_nmpc_occmap_local_view(centre = NULL)'s to the bit.
//   * the grid is frp_nmpc_cloud_grid_build's (frp_corridor.hip: grid_cell_of, grid_count / scan / scatter) with every loop bound read
//     from count[0]; the cell counts are taken by the emitting lanes while the point is in registers, and grid_start / cursor are zeroed
//     by launch 1, so the start array is complete for every count and a stale point beyond the count is in no cell.
#include "frp_occmap.hpp"

namespace frp {
namespace occmap {

constexpr int SV_THREADS = 256;

struct SharedView {
    int cap, cells, ncols, cols_per_group;
    double cell;
    int dims[3];
    double *cloud;
    int *count, *total;
    double *points;
    int *index, *start, *cursor, *sums;
};

// word k of a column with the bits at and above gz masked off (local_view_kernel's hi[2] mask for the whole map)
__device__ __forceinline__ uint32_t column_word(const uint32_t *w, int k, int gz)
{
    uint32_t m = w[k];
    const int zb = k << 5;
    if (gz < zb + 32) m &= ~0u >> (zb + 32 - gz);
    return m;
}

// one axis of grid_cell_of (frp_corridor.hip): NaN and coordinates beyond the grid go to border cells
__device__ __forceinline__ int cell_axis(double p, double origin, double cell, int dim)
{
    const double a = floor((p - origin) / cell);
    return !(a > 0) ? 0 : (a > dim - 1 ? dim - 1 : (int)a);
}

// launch 1: group_sums[w] = occupied voxels of run w; grid_start[0 .. cells] = 0, cursor[0 .. cells) = 0
__global__ __launch_bounds__(SV_THREADS) void view_count_kernel(Geo g, SharedView v, const uint32_t *plane)
{
    __shared__ int s_wave[SV_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = blockIdx.x * SV_THREADS + tid; i <= v.cells; i += gridDim.x * SV_THREADS) {
        v.start[i] = 0;
        if (i < v.cells) v.cursor[i] = 0;
    }
    const int c0 = blockIdx.x * v.cols_per_group, c1 = c0 + v.cols_per_group < v.ncols ? c0 + v.cols_per_group : v.ncols;
    int cnt = 0;
    for (int c = c0 + tid; c < c1; c += SV_THREADS) {
        const uint32_t *w = plane + (size_t)c * g.wz; // column c = x * gy + y
        for (int k = 0; k < g.wz; k++) cnt += __popc(column_word(w, k, g.grid[2]));
    }
    for (int d = 32; d; d >>= 1) cnt += __shfl_down(cnt, d, 64);
    if (lane == 0) s_wave[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int k = 0; k < SV_THREADS / 64; k++) s += s_wave[k];
        v.sums[blockIdx.x] = s;
    }
}

// launch 2: group_sums <- its exclusive prefix sum (groups <= 1024 = one element per lane), total, count
__global__ __launch_bounds__(FRP_OCCMAP_VIEW_MAX_GROUPS) void view_scan_kernel(SharedView v, int groups)
{
    __shared__ int s_part[FRP_OCCMAP_VIEW_MAX_GROUPS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x = tid < groups ? v.sums[tid] : 0;
    int inc = x;
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_part[wave] = inc;
    __syncthreads();
    int before = 0, total = 0;
    for (int k = 0; k < FRP_OCCMAP_VIEW_MAX_GROUPS / 64; k++) {
        const int s = s_part[k];
        before += k < wave ? s : 0;
        total += s;
    }
    if (tid < groups) v.sums[tid] = before + inc - x;
    if (tid == 0) {
        v.total[0] = total;
        v.count[0] = total < v.cap ? total : v.cap; // overflow keeps the first cap points; the count stays non-negative
    }
}

// launch 3: run blockIdx.x's centres from cloud[group_sums[blockIdx.x]] on, local_view_kernel's tile loop; every stored point is
// counted into start[cell + 1] (grid_count_kernel)
__global__ __launch_bounds__(SV_THREADS) void view_emit_kernel(Geo g, SharedView v, const uint32_t *plane)
{
    __shared__ int s_wave[2][SV_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * v.cols_per_group, c1 = c0 + v.cols_per_group < v.ncols ? c0 + v.cols_per_group : v.ncols;
    const int gy = g.grid[1], gz = g.grid[2];
    int base = v.sums[blockIdx.x];
    for (int t0 = c0, it = 0; t0 < c1 && base < v.cap; t0 += SV_THREADS, it ^= 1) { // (base is the same in every lane)
        const int c = t0 + tid;
        int x = 0, y = 0, cnt = 0;
        const uint32_t *w = nullptr;
        if (c < c1) {
            x = c / gy; y = c % gy;
            w = plane + (size_t)c * g.wz;
            for (int k = 0; k < g.wz; k++) cnt += __popc(column_word(w, k, gz));
        }
        int inc = cnt; // inclusive scan over the wavefront
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) s_wave[it][wave] = inc;
        __syncthreads(); // (the other buffer is written next: one barrier per tile)
        int before = 0, total = 0;
        for (int k = 0; k < SV_THREADS / 64; k++) {
            const int s = s_wave[it][k];
            before += k < wave ? s : 0;
            total += s;
        }
        int at = base + before + inc - cnt;
        if (cnt > 0 && at < v.cap) {
            const double px = (double)(float)(g.origin[0] + ((double)x + 0.5) * g.res); // indexToPos (:77-82), pcl::PointXYZ (:203)
            const double py = (double)(float)(g.origin[1] + ((double)y + 0.5) * g.res);
            const int ix = cell_axis(px, g.origin[0], v.cell, v.dims[0]), iy = cell_axis(py, g.origin[1], v.cell, v.dims[1]);
            for (int k = 0; k < g.wz; k++) {
                uint32_t m = column_word(w, k, gz);
                const int zb = k << 5;
                while (m && at < v.cap) {
                    const int z = zb + __ffs(m) - 1;
                    m &= m - 1;
                    const double pz = (double)(float)(g.origin[2] + ((double)z + 0.5) * g.res);
                    double *o = v.cloud + 3 * (size_t)at;
                    o[0] = px; o[1] = py; o[2] = pz;
                    const int iz = cell_axis(pz, g.origin[2], v.cell, v.dims[2]);
                    atomicAdd(&v.start[(iz * v.dims[1] + iy) * v.dims[0] + ix + 1], 1);
                    at++;
                }
            }
        }
        base += total;
    }
}

// launch 4: grid_scan_kernel (frp_corridor.hip): inclusive prefix sum of start[1 .. cells] in place, one workgroup in 1024-element chunks
__global__ __launch_bounds__(1024) void view_grid_scan_kernel(SharedView v)
{
    __shared__ int s_part[16], s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int base = 1; base <= v.cells; base += 1024) {
        const int i = base + tid;
        int x = i <= v.cells ? v.start[i] : 0;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(x, d, 64);
            if (lane >= d) x += o;
        }
        if (lane == 63) s_part[wave] = x;
        __syncthreads();
        int add = s_carry;
        for (int k = 0; k < wave; k++) add += s_part[k];
        if (i <= v.cells) v.start[i] = x + add;
        __syncthreads();
        if (tid == 1023) s_carry = x + add;
        __syncthreads();
    }
}

// launch 5: grid_scatter_kernel (frp_corridor.hip) over cloud[0 .. count[0])
__global__ __launch_bounds__(SV_THREADS) void view_grid_scatter_kernel(Geo g, SharedView v)
{
    const int n = v.count[0];
    for (int i = blockIdx.x * SV_THREADS + threadIdx.x; i < n; i += gridDim.x * SV_THREADS) {
        const double *pt = v.cloud + 3 * (size_t)i;
        const double px = pt[0], py = pt[1], pz = pt[2];
        const int ix = cell_axis(px, g.origin[0], v.cell, v.dims[0]), iy = cell_axis(py, g.origin[1], v.cell, v.dims[1]),
                  iz = cell_axis(pz, g.origin[2], v.cell, v.dims[2]);
        const int cell = (iz * v.dims[1] + iy) * v.dims[0] + ix;
        const int at = v.start[cell] + atomicAdd(&v.cursor[cell], 1); // order inside a cell is irrelevant (ties go by cloud index)
        if (at >= v.cap) continue;                                    // (cannot happen: start was counted over these points)
        v.points[3 * (size_t)at] = px; v.points[3 * (size_t)at + 1] = py; v.points[3 * (size_t)at + 2] = pz;
        v.index[at] = i;
    }
}

// dims[k] = ceil(map_size[k] / cell); false when the cell or the cell count is out of range
static bool view_dims(const frp_nmpc_occmap *m, double cell, int dims[3])
{
    if (!(cell > 0.0) || !std::isfinite(cell)) return false;
    double cells = 1.0;
    for (int k = 0; k < 3; k++) {
        const double n = std::ceil(m->map_size[k] / cell);
        if (!(n >= 1.0 && n <= (double)FRP_CORRIDOR_MAX_CELLS)) return false;
        dims[k] = (int)n;
        cells *= n;
    }
    return cells <= (double)FRP_CORRIDOR_MAX_CELLS;
}

} // namespace occmap
} // namespace frp

extern "C" {

int frp_nmpc_occmap_shared_view_dims(const frp_nmpc_occmap *m, double cell, int dims[3])
{
    int d[3];
    if (!frp::occmap::valid(m) || !dims || !frp::occmap::view_dims(m, cell, d)) return FRP_ERR_ARG;
    for (int k = 0; k < 3; k++) dims[k] = d[k];
    return FRP_OK;
}

// The five launches for a view of at most max_cap points.  Nothing in the kernels above depends on the capacity's size: every position
// (at, base, count, the grid's start / cursor / index entries) is a 32-bit int below 2^22, and every byte offset is taken as
// 3 * (size_t)at -- so the large entry (include/frp_nmpc_corridor_large.h) is this function with another bound.
static int shared_view_update(const frp_nmpc_occmap *m, const frp_nmpc_occmap_shared_view *v, void *workspace, size_t workspace_bytes, void *stream,
                              int max_cap)
{
    using namespace frp::occmap;
    if (!args_ok(m, workspace, workspace_bytes) || !v) return FRP_ERR_ARG;
    if (v->cap < 1 || v->cap > max_cap) return FRP_ERR_ARG;
    int d[3];
    if (!view_dims(m, v->cell, d) || d[0] != v->dims[0] || d[1] != v->dims[1] || d[2] != v->dims[2]) return FRP_ERR_ARG;
    if (!v->cloud || !v->count || !v->total || !v->grid_points || !v->grid_index || !v->grid_start || !v->cursor || !v->group_sums) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    SharedView s;
    s.cap = v->cap; s.cells = d[0] * d[1] * d[2]; s.cell = v->cell;
    for (int k = 0; k < 3; k++) s.dims[k] = d[k];
    s.cloud = v->cloud; s.count = v->count; s.total = v->total; s.points = v->grid_points; s.index = v->grid_index; s.start = v->grid_start;
    s.cursor = v->cursor; s.sums = v->group_sums;
    // runs of whole tiles: tiles_per_group * groups >= tiles, groups <= FRP_OCCMAP_VIEW_MAX_GROUPS (valid(): ncols < 2^30)
    s.ncols = m->grid[0] * m->grid[1];
    const int tiles = (s.ncols + SV_THREADS - 1) / SV_THREADS;
    const int tiles_per_group = (tiles + FRP_OCCMAP_VIEW_MAX_GROUPS - 1) / FRP_OCCMAP_VIEW_MAX_GROUPS;
    const int groups = (tiles + tiles_per_group - 1) / tiles_per_group;
    s.cols_per_group = tiles_per_group * SV_THREADS;
    const Geo g = geo(m);
    const uint32_t *plane = static_cast<const uint32_t *>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(view_count_kernel, dim3((unsigned)groups), dim3(SV_THREADS), 0, st, g, s, plane);
    hipLaunchKernelGGL(view_scan_kernel, dim3(1), dim3(FRP_OCCMAP_VIEW_MAX_GROUPS), 0, st, s, groups);
    hipLaunchKernelGGL(view_emit_kernel, dim3((unsigned)groups), dim3(SV_THREADS), 0, st, g, s, plane);
    hipLaunchKernelGGL(view_grid_scan_kernel, dim3(1), dim3(1024), 0, st, s);
    hipLaunchKernelGGL(view_grid_scatter_kernel, dim3(256), dim3(SV_THREADS), 0, st, g, s);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

int frp_nmpc_occmap_shared_view_update(const frp_nmpc_occmap *m, const frp_nmpc_occmap_shared_view *v, void *workspace, size_t workspace_bytes,
                                       void *stream)
{
    return shared_view_update(m, v, workspace, workspace_bytes, stream, FRP_CORRIDOR_MAX_POINTS);
}

int frp_nmpc_occmap_shared_view_update_large(const frp_nmpc_occmap *m, const frp_nmpc_occmap_shared_view *v, void *workspace,
                                             size_t workspace_bytes, void *stream)
{
    return shared_view_update(m, v, workspace, workspace_bytes, stream, FRP_CORRIDOR_LARGE_MAX_POINTS);
}

} // extern "C"
