// frp_nmpc.h section (8), frp_nmpc_occmap_fuse_points.h: S point-cloud scans ray-cast into the device occupancy map in one call --
// OccMap::raycastProcess (occ_grid/src/occ_map.cpp:441-533) for every scan, to the bit of running it scan after scan.  The scans are the
// frames of the batched depth call (frp_occmap_fuse_batch.hip): the descriptors, the workspace slices and the stage kernels from init
// and the ray set-up on are that unit's, launched through fuse::batch::launch_init / launch_from_setup (frp_occmap_fuse.hpp), not
// copied.  What is this file's own:
//
//   describe one lane per scan: the number of points (count[s] clamped to [0, P]), the sensor position and the ray box around it
//            (set_ray_box) into the scan's descriptor; status of an inactive ({0, 0}) or refused (a non-finite origin) scan
//   load     stands where the depth calls project.  A workgroup copies the coordinates of its 256 points -- one contiguous run of
//            768 doubles or floats, whatever their 24- or 12-byte stride per point -- into LDS with unit-stride loads, each lane
//            then takes its point from there, widens a float exactly, drops a point with a non-finite coordinate (it keeps its
//            index) and runs the head of raycastProcess's loop (end_lane: length test, clip, setCacheOccupancy on the end voxel, the
//            atomic minimum of the point index that is cache_rayend_'s dedup).  Nothing beyond count[s] points is read.
//   init, setup, mark / stop rounds, status, count, update: frp_occmap_fuse_batch.hip's kernels, the scan as the frame.
// Launches: 2 * max_rounds + 7, whatever S and P.  No kernel waits for another workgroup.  Compiled with -ffp-contract=off like the
// other fusion units.
#include "frp_nmpc_occmap_fuse_points.h"
#include "frp_occmap_fuse.hpp"

namespace frp {
namespace occmap {
namespace fuse {
namespace points {

using batch::Batch;
using batch::BatchPlan;
using batch::Desc;
using batch::ws_of;

constexpr int TILE = 256; // points per workgroup of the load stage = its lanes = those of batch::blocks

__global__ void describe_kernel(Batch b, Geo g, Frame shape, int P, const int *count, const double *origin, const int *active, int *status,
                                size_t nbmax)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= b.frames) return;
    Frame f = shape;
    f.status = status + 2 * k;
    int live = 1, refused = 0;
    if (active && active[k] == 0) {
        live = 0;
    } else {
        const double *t = origin + 3 * (size_t)k;
        if (!finite_all(t, 3)) {
            live = 0; refused = 1;
        } else {
            int n = count ? count[k] : P;
            f.N = n < 0 ? 0 : n > P ? P : n;
            for (int i = 0; i < 3; i++) f.t[i] = t[i];
            const size_t nbox = set_ray_box(f, g);
            if (nbox > nbmax) { live = 0; refused = 1; } // (no finite origin: the bound holds for every box of posToIndex(t -/+ max_ray_length))
            else f.nbox = (int)nbox;
        }
    }
    if (!live) {
        f.N = 0;
        for (int i = 0; i < 6; i++) f.box[i] = 0;
        f.bd[0] = f.bd[1] = f.bd[2] = 0; f.nbox = 0;
        f.status[0] = refused ? FRP_OCCMAP_FUSE_REFUSED : 0;
        f.status[1] = 0;
    }
    b.desc[k].f = f;
    b.desc[k].live = live;
    b.desc[k].fused = 0;
}

// T = double or float; `all` = [S][P][3].  Every lane of a workgroup takes the same branches up to the barrier: what they depend on
// (the scan's descriptor, the block's first point) is the same for all of them.
template <class T>
__global__ __launch_bounds__(TILE) void load_kernel(Batch b, Geo g, const T *all, int P)
{
    __shared__ T tile[3 * TILE];
    const Desc &d = b.desc[blockIdx.y];
    if (!d.live) return;
    const Frame f = d.f;
    const int first = blockIdx.x * TILE;
    const int here = f.N - first < TILE ? f.N - first : TILE; // points of this workgroup; the last value read is coordinate 3 * f.N - 1 of the scan
    if (here <= 0) return;
    const T *src = all + 3 * ((size_t)blockIdx.y * (size_t)P + (size_t)first);
    for (int i = threadIdx.x; i < 3 * here; i += TILE) tile[i] = src[i];
    __syncthreads();
    const int lane = threadIdx.x, n = first + lane;
    if (lane >= here) return;
    const Ws w = ws_of(b, blockIdx.y);
    w.endv[n] = NO_RAY;
    double p[3] = {(double)tile[3 * lane], (double)tile[3 * lane + 1], (double)tile[3 * lane + 2]};
    if (!finite_all(p, 3)) return; // "no return": not in the scan
    end_lane(g, f, w, n, p);
}

// Everything that can be refused on the host: the shape of the scans and the parameters (no origin, no pointer)
static bool plan(const frp_nmpc_occmap *m, const frp_nmpc_occmap_fuse_points *q, BatchPlan *out)
{
    if (!m || !q) return false;
    if (q->scans < 1 || q->scans > FRP_OCCMAP_FUSE_POINTS_MAX_SCANS) return false;
    if (!plan_rays(m, q->P, q->prob_hit_log, q->prob_miss_log, q->min_ray_length, q->max_ray_length, q->max_rounds, &out->p)) return false;
    batch::plan_slices(out, q->scans);
    return true;
}

} // namespace points
} // namespace fuse
} // namespace occmap
} // namespace frp

extern "C" {

size_t frp_nmpc_occmap_fuse_points_workspace_bytes(const frp_nmpc_occmap *map, const frp_nmpc_occmap_fuse_points *f)
{
    frp::occmap::fuse::batch::BatchPlan p{};
    return frp::occmap::fuse::points::plan(map, f, &p) ? p.bytes : 0;
}

int frp_nmpc_occmap_fuse_points_batch(const frp_nmpc_occmap *map, const frp_nmpc_occmap_fuse_points *q, void *workspace, size_t workspace_bytes,
                                      void *fuse_workspace, size_t fuse_workspace_bytes, void *stream)
{
    using namespace frp::occmap;
    using namespace frp::occmap::fuse;
    using namespace frp::occmap::fuse::points;
    BatchPlan bp{}; // (the image's fields of the frame description stay zero: no stage of this call reads them)
    if (!args_ok(map, workspace, workspace_bytes) || !plan(map, q, &bp)) return FRP_ERR_ARG;
    if (!q->origin || !q->status) return FRP_ERR_ARG;
    if (q->P > 0 && (q->points != nullptr) == (q->points_f32 != nullptr)) return FRP_ERR_ARG;
    Batch b;
    if (!batch::batch_at(fuse_workspace, fuse_workspace_bytes, bp, q->scans, &b)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Plan &p = bp.p;
    const Geo g = geo(map);
    const dim3 tiles = batch::blocks(b, (size_t)p.f.N); // (plan_rays: N = P; a scan's count is known on the device only)
    hipLaunchKernelGGL(describe_kernel, dim3(1), dim3(FRP_OCCMAP_FUSE_POINTS_MAX_SCANS), 0, st, b, g, p.f, q->P, q->count, q->origin, q->active, q->status,
                       p.nbmax);
    batch::launch_init(b, p, st);
    if (q->points_f32 && q->P > 0) hipLaunchKernelGGL(load_kernel<float>, tiles, dim3(TILE), 0, st, b, g, q->points_f32, q->P);
    else hipLaunchKernelGGL(load_kernel<double>, tiles, dim3(TILE), 0, st, b, g, q->points, q->P); // (P = 0: no scan has a point, nothing is read)
    return batch::launch_from_setup(b, p, map, workspace, st);
}

} // extern "C"
