// frp_nmpc.h section (8), frp_nmpc_occmap_fuse.h: one depth frame fused into the device occupancy map -- OccMap::projectDepthImage,
// raycastProcess and setCacheOccupancy (occ_grid/src/occ_map.cpp:314-563) with RayCaster::setInput / step (raycast.cpp:263-366), to the
// bit of the reference's serial scan.  tests/occmap_fusion_oracle.py is the statement-by-statement restatement this file follows
// (operation order of every Eigen expression included); compiled with -ffp-contract=off like frp_occmap.hip.
//
//   init     the per-voxel arrays of the ray box (all, hit, end owner, mark) and the header; the workspace arrives uninitialised
//   project  one lane per scanned pixel; the scan index n IS the sequence number of the point (no compaction: order is kept by n).
//            Shift filter, length test, clip, end voxel: all / hit += 1 there (setCacheOccupancy, :464 / :467), owner = min(owner, n)
//   setup    a point casts its ray when its end is outside the map (INVALID_IDX: no dedup, :470) or it owns its end voxel
//            (cache_rayend_, :472-477).  The ray's whole path is walked once for its length; cast rays go into a list
//   rounds   cache_traverse_ (:494-501) as a fixed point: count[n] = cells ray n processes, initially its whole path.
//            mark pass: mark[v] = min n over the first count[n] cells; stop pass: count[n] = 1 + first position whose voxel has
//            mark < n (the break voxel is counted before the break) or repeats the voxel before it (a ray meeting its own mark).
//            Rays 0 ... k are final after k + 1 rounds (ray n only looks at marks of rays below it), so the fixed point is unique and
//            is the serial scan.  Marks carry the round in their top byte (later round = smaller key), so no clearing between rounds.
//            max_rounds rounds are launched; round r > 1 returns at once when round r - 1 changed nothing.  No kernel waits for
//            another workgroup.
//   status   rounds used / minus the cap, rays cast; whether the frame converged
//   count    all[v] += 1 over the first count[n] cells of every cast ray (the :493 calls), only when converged
//   update   per voxel of the box with all > 0: the batch update of :505-532; log_odds, occ and the bit plane together
// The stages' bodies, the ray caster and the host checks of a description live in frp_occmap_fuse.hpp, shared with the batched call
// (frp_occmap_fuse_batch.hip).  Every traversal loop runs at most Frame.nb = 3 * (ceil(max_ray_length / resolution) + 2) <= 4096 steps.
#include "frp_occmap_fuse.hpp"

namespace frp {
namespace occmap {
namespace fuse {

__global__ __launch_bounds__(256) void init_kernel(Frame f, Ws w) { init_lane(f, w, blockIdx.x * blockDim.x + threadIdx.x); }

__global__ __launch_bounds__(256) void project_kernel(Geo g, Frame f, Ws w) { project_lane(g, f, w, blockIdx.x * blockDim.x + threadIdx.x); }

__global__ __launch_bounds__(256) void setup_kernel(Geo g, Frame f, Ws w) { setup_lane(g, f, w, blockIdx.x * blockDim.x + threadIdx.x); }

__global__ __launch_bounds__(256) void mark_kernel(Geo g, Frame f, Ws w, int round)
{
    if (round > 1 && w.hdr[round - 1] == 0) return; // the round before changed nothing: the frame is final
    mark_lane(g, f, w, round, blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(256) void stop_kernel(Geo g, Frame f, Ws w, int round)
{
    if (round > 1 && w.hdr[round - 1] == 0) return;
    stop_lane(g, f, w, round, blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ void status_kernel(Frame f, Ws w)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    status_lane(f, w);
}

__global__ __launch_bounds__(256) void count_kernel(Geo g, Frame f, Ws w)
{
    if (!w.hdr[H_CONVERGED]) return;
    count_lane(g, f, w, blockIdx.x * blockDim.x + threadIdx.x);
}

// the batch update (:505-532) of box voxel i
__global__ __launch_bounds__(256) void update_kernel(Geo g, Frame f, Ws w, double *log_odds, unsigned char *occ, uint32_t *plane)
{
    if (!w.hdr[H_CONVERGED]) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= f.nbox) return;
    const int all = w.all[i];
    if (all == 0) return; // not in cache_voxel_
    const int z = f.box[2] + i % f.bd[2], y = f.box[1] + (i / f.bd[2]) % f.bd[1], x = f.box[0] + i / (f.bd[2] * f.bd[1]);
    double v = log_odds[((size_t)x * g.grid[1] + y) * g.grid[2] + z];
    if (update_value(f, all, w.hit[i], v)) write_voxel(g, x, y, z, v, log_odds, occ, plane);
}

// Everything that can be refused without looking at a pointer; fills the frame description and the workspace layout.
static bool plan(const frp_nmpc_occmap *m, const frp_nmpc_occmap_fuse *q, Plan *out)
{
    if (!m || !q) return false;
    if (!plan_shape(m, q->rows, q->cols, q->K, q->depth_scale, q->depth_filter_mindist, q->depth_filter_tolerance, q->depth_filter_margin, q->skip_pixel,
                    q->prob_hit_log, q->prob_miss_log, q->min_ray_length, q->max_ray_length, q->max_rounds, out))
        return false;
    Frame &f = out->f;
    f.depth = q->depth; f.last = q->last_depth; f.status = q->status;
    if (!set_pose(f, q->T_wc, q->last_T_wc)) return false;
    const size_t nbox = set_ray_box(f, geo(m));
    if (nbox > out->nbmax) return false;
    f.nbox = (int)nbox;
    return true;
}

} // namespace fuse
} // namespace occmap
} // namespace frp

extern "C" {

size_t frp_nmpc_occmap_fuse_workspace_bytes(const frp_nmpc_occmap *map, const frp_nmpc_occmap_fuse *f)
{
    frp::occmap::fuse::Plan p;
    return frp::occmap::fuse::plan(map, f, &p) ? p.bytes : 0;
}

int frp_nmpc_occmap_fuse_depth(const frp_nmpc_occmap *map, const frp_nmpc_occmap_fuse *q, void *workspace, size_t workspace_bytes,
                               void *fuse_workspace, size_t fuse_workspace_bytes, void *stream)
{
    using namespace frp::occmap;
    using namespace frp::occmap::fuse;
    Plan p;
    if (!args_ok(map, workspace, workspace_bytes) || !plan(map, q, &p)) return FRP_ERR_ARG;
    if (!q->depth || !q->status || !fuse_workspace || fuse_workspace_bytes < p.bytes) return FRP_ERR_ARG;
    if (((uintptr_t)fuse_workspace & 7) != 0) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Ws w = ws_at(static_cast<char *>(fuse_workspace), p.off);
    const Frame &f = p.f;
    const Geo g = geo(map);
    const auto blocks = [](size_t n) { return dim3((unsigned)((n > 0 ? n : 1) + 255) / 256); };
    const dim3 rays = blocks((size_t)f.N), box = blocks((size_t)f.nbox);
    hipLaunchKernelGGL(init_kernel, blocks((size_t)(f.nbox > HDR_INTS ? f.nbox : HDR_INTS)), dim3(256), 0, st, f, w);
    hipLaunchKernelGGL(project_kernel, rays, dim3(256), 0, st, g, f, w);
    hipLaunchKernelGGL(setup_kernel, rays, dim3(256), 0, st, g, f, w);
    for (int r = 1; r <= f.max_rounds; r++) {
        hipLaunchKernelGGL(mark_kernel, rays, dim3(256), 0, st, g, f, w, r);
        hipLaunchKernelGGL(stop_kernel, rays, dim3(256), 0, st, g, f, w, r);
    }
    hipLaunchKernelGGL(status_kernel, dim3(1), dim3(64), 0, st, f, w);
    hipLaunchKernelGGL(count_kernel, rays, dim3(256), 0, st, g, f, w);
    hipLaunchKernelGGL(update_kernel, box, dim3(256), 0, st, g, f, w, map->log_odds, map->occ, static_cast<uint32_t *>(workspace));
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

} // extern "C"
