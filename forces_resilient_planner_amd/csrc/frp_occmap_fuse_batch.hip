// frp_nmpc.h section (8), frp_nmpc_occmap_fuse_batch.h: F depth frames fused into the device occupancy map in one call, to the bit of F
// successive frp_nmpc_occmap_fuse_depth calls (frp_occmap_fuse.hip), with every pose read on the device.  The stages are those of the
// single-frame call -- their bodies, the ray caster, walk and box_voxel are frp_occmap_fuse.hpp's, shared, not copied -- with the frame
// as the second grid dimension and every per-pixel / per-voxel array inside its frame's slice of the workspace.  Compiled with
// -ffp-contract=off like frp_occmap_fuse.hip.
//
//   describe one lane per frame: rotation, translation, last_R^-1, the ray box (set_pose / set_ray_box, the functions the host runs for
//            the single-frame call) into the frame's descriptor; status of an inactive ({0, 0}) or refused frame
//   init, project, setup, mark / stop rounds, count: as in frp_occmap_fuse.hip per frame.  A frame that is inactive or refused, and
//            in a round a frame whose previous round changed nothing, returns at its first instructions
//   status   one lane per frame; `fused` = the frame takes part in the update (live and converged)
//   update   ONE launch, ordered per voxel.  Lane (j, i) is voxel i of frame j's ray box.  A voxel is OWNED by the first fused
//            frame whose box holds it (geometry alone, so every lane decides it without reading per-voxel data); the owner applies
//            the update of :512-531 for frames j, j + 1, ..., F - 1 in order, for every fused frame whose box holds the voxel with
//            all > 0, on a value carried in a register, and writes log_odds, occ and the bit of the plane once.  Exactly one lane
//            owns a voxel, so no two lanes update the same voxel, and no kernel waits for another workgroup.
// Launches: 2 * max_rounds + 7, whatever F.  All but describe and project are launched by launch_init / launch_from_setup below, which
// the point scans' call (frp_occmap_fuse_points.hip) runs too, behind its own describe and load: the library holds these kernels once.
#include "frp_nmpc_occmap_fuse_batch.h"
#include "frp_occmap_fuse.hpp"

namespace frp {
namespace occmap {
namespace fuse {
namespace batch {

__global__ void describe_kernel(Batch b, Geo g, Frame shape, const unsigned short *depth, const unsigned short *last, const double *T_wc,
                                const double *last_T_wc, const int *active, int *status, size_t nbmax)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= b.frames) return;
    Frame f = shape;
    const size_t image = (size_t)f.rows * f.cols;
    f.depth = depth + k * image;
    f.last = last ? last + k * image : nullptr;
    f.status = status + 2 * k;
    int live = 1, refused = 0;
    if (active && active[k] == 0) {
        live = 0;
    } else if (!set_pose(f, T_wc + 16 * (size_t)k, last ? last_T_wc + 16 * (size_t)k : nullptr)) {
        live = 0; refused = 1;
    } else {
        const size_t nbox = set_ray_box(f, g);
        if (nbox > nbmax) { live = 0; refused = 1; } // (no finite pose: the bound holds for every box of posToIndex(t -/+ max_ray_length))
        else f.nbox = (int)nbox;
    }
    if (!live) {
        for (int i = 0; i < 6; i++) f.box[i] = 0;
        f.bd[0] = f.bd[1] = f.bd[2] = 0; f.nbox = 0;
        f.status[0] = refused ? FRP_OCCMAP_FUSE_REFUSED : 0;
        f.status[1] = 0;
    }
    b.desc[k].f = f;
    b.desc[k].live = live;
    b.desc[k].fused = 0;
}

__global__ __launch_bounds__(256) void init_kernel(Batch b)
{
    const Desc &d = b.desc[blockIdx.y];
    if (!d.live) return;
    const Frame f = d.f;
    init_lane(f, ws_of(b, blockIdx.y), blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(256) void project_kernel(Batch b, Geo g)
{
    const Desc &d = b.desc[blockIdx.y];
    if (!d.live) return;
    const Frame f = d.f;
    project_lane(g, f, ws_of(b, blockIdx.y), blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(256) void setup_kernel(Batch b, Geo g)
{
    const Desc &d = b.desc[blockIdx.y];
    if (!d.live) return;
    const Frame f = d.f;
    setup_lane(g, f, ws_of(b, blockIdx.y), blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(256) void mark_kernel(Batch b, Geo g, int round)
{
    const Desc &d = b.desc[blockIdx.y];
    if (!d.live) return;
    const Ws w = ws_of(b, blockIdx.y);
    if (round > 1 && w.hdr[round - 1] == 0) return; // the round before changed nothing: the frame is final
    const Frame f = d.f;
    mark_lane(g, f, w, round, blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(256) void stop_kernel(Batch b, Geo g, int round)
{
    const Desc &d = b.desc[blockIdx.y];
    if (!d.live) return;
    const Ws w = ws_of(b, blockIdx.y);
    if (round > 1 && w.hdr[round - 1] == 0) return;
    const Frame f = d.f;
    stop_lane(g, f, w, round, blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ void status_kernel(Batch b)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= b.frames) return;
    Desc &d = b.desc[k];
    if (!d.live) return; // fused stays 0
    const Ws w = ws_of(b, k);
    status_lane(d.f, w);
    d.fused = w.hdr[H_CONVERGED];
}

__global__ __launch_bounds__(256) void count_kernel(Batch b, Geo g)
{
    const Desc &d = b.desc[blockIdx.y];
    if (!d.fused) return;
    const Frame f = d.f;
    count_lane(g, f, ws_of(b, blockIdx.y), blockIdx.x * blockDim.x + threadIdx.x);
}

// The ordered update: lane (j, i) is voxel i of frame j's ray box (update_lane, frp_occmap_fuse.hpp)
__global__ __launch_bounds__(256) void update_kernel(Batch b, Geo g, double *log_odds, unsigned char *occ, uint32_t *plane)
{
    update_lane(b, g, log_odds, occ, plane);
}

// Everything that can be refused on the host: the shape of the frames and the parameters (no pose, no pointer)
static bool plan(const frp_nmpc_occmap *m, const frp_nmpc_occmap_fuse_batch *q, BatchPlan *out)
{
    if (!m || !q) return false;
    if (q->frames < 1 || q->frames > FRP_OCCMAP_FUSE_MAX_FRAMES) return false;
    if (!plan_shape(m, q->rows, q->cols, q->K, q->depth_scale, q->depth_filter_mindist, q->depth_filter_tolerance, q->depth_filter_margin, q->skip_pixel,
                    q->prob_hit_log, q->prob_miss_log, q->min_ray_length, q->max_ray_length, q->max_rounds, &out->p))
        return false;
    plan_slices(out, q->frames);
    return true;
}

static_assert(FRP_OCCMAP_FUSE_POINTS_MAX_SCANS == FRP_OCCMAP_FUSE_MAX_FRAMES, "one lane per frame or scan: the status launch serves both routes");

void launch_init(const Batch &b, const Plan &p, hipStream_t st)
{
    hipLaunchKernelGGL(init_kernel, blocks(b, p.nbmax > (size_t)HDR_INTS ? p.nbmax : (size_t)HDR_INTS), dim3(256), 0, st, b);
}

int launch_from_setup(const Batch &b, const Plan &p, const frp_nmpc_occmap *map, void *workspace, hipStream_t st)
{
    const Geo g = geo(map);
    const dim3 rays = blocks(b, (size_t)p.f.N), box = blocks(b, p.nbmax);
    hipLaunchKernelGGL(setup_kernel, rays, dim3(256), 0, st, b, g);
    for (int r = 1; r <= p.f.max_rounds; r++) {
        hipLaunchKernelGGL(mark_kernel, rays, dim3(256), 0, st, b, g, r);
        hipLaunchKernelGGL(stop_kernel, rays, dim3(256), 0, st, b, g, r);
    }
    hipLaunchKernelGGL(status_kernel, dim3(1), dim3(FRP_OCCMAP_FUSE_MAX_FRAMES), 0, st, b);
    hipLaunchKernelGGL(count_kernel, rays, dim3(256), 0, st, b, g);
    hipLaunchKernelGGL(update_kernel, box, dim3(256), 0, st, b, g, map->log_odds, map->occ, static_cast<uint32_t *>(workspace));
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

} // namespace batch
} // namespace fuse
} // namespace occmap
} // namespace frp

extern "C" {

size_t frp_nmpc_occmap_fuse_batch_workspace_bytes(const frp_nmpc_occmap *map, const frp_nmpc_occmap_fuse_batch *f)
{
    frp::occmap::fuse::batch::BatchPlan p;
    return frp::occmap::fuse::batch::plan(map, f, &p) ? p.bytes : 0;
}

int frp_nmpc_occmap_fuse_depth_batch(const frp_nmpc_occmap *map, const frp_nmpc_occmap_fuse_batch *q, void *workspace, size_t workspace_bytes,
                                     void *fuse_workspace, size_t fuse_workspace_bytes, void *stream)
{
    using namespace frp::occmap;
    using namespace frp::occmap::fuse;
    using namespace frp::occmap::fuse::batch;
    BatchPlan bp;
    if (!args_ok(map, workspace, workspace_bytes) || !plan(map, q, &bp)) return FRP_ERR_ARG;
    if (!q->depth || !q->T_wc || !q->status || (q->last_depth && !q->last_T_wc)) return FRP_ERR_ARG;
    Batch b;
    if (!batch_at(fuse_workspace, fuse_workspace_bytes, bp, q->frames, &b)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Plan &p = bp.p;
    hipLaunchKernelGGL(describe_kernel, dim3(1), dim3(FRP_OCCMAP_FUSE_MAX_FRAMES), 0, st, b, geo(map), p.f, q->depth, q->last_depth, q->T_wc, q->last_T_wc,
                       q->active, q->status, p.nbmax);
    launch_init(b, p, st);
    hipLaunchKernelGGL(project_kernel, blocks(b, (size_t)p.f.N), dim3(256), 0, st, b, geo(map));
    return launch_from_setup(b, p, map, workspace, st);
}

} // extern "C"
