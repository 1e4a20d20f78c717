// frp_nmpc.h section (8), frp_nmpc_occmap_render_scan.h: S point scans rendered from the device occupancy map's bit plane, one ray per
// entry of a table of beam directions -- the point-scan sibling of frp_occmap_render.hip.  The reference has no counterpart:
// tests/occmap_scan_oracle.py is the specification, and every double computed here is computed in the order it writes down.  Compiled
// with -ffp-contract=off like frp_occmap_render.hip.  The walk is that unit's, restated (frp_occmap_raywalk.hpp says why).
//
//   describe  one lane per scan: status[s] = {1, 0} rendered, {0, 0} inactive, {FRP_OCCMAP_FUSE_REFUSED, 0} a non-finite T_ws[s];
//             count[s] = P or 0; origin[s] = the translation of T_ws[s] as it stands (not for an inactive scan).  status[s][0] hands the
//             flag on to the render kernel: no scratch.
//   render    one lane per beam, 64 consecutive beams per wavefront, one wavefront per workgroup, the scan as the grid's second
//             dimension.  Consecutive beams of a firing-ordered table point in nearby directions: the wavefront's rays walk
//             neighbouring columns of the bit plane and share its cache lines, and are of similar length, which bounds the divergence
//             of the walk; no wavefront waits for another.  The scan's flag and pose are read through wave-uniform addresses.  A lane
//             keeps the last word of the plane it loaded: a step along z inside a word costs no load.  The 24-byte (12-byte) point
//             rows of the wavefront -- one contiguous run of 192 doubles (floats) -- go through LDS and out with unit-stride stores,
//             the mirror image of frp_occmap_fuse_points.hip's load stage.  status[s][1] is one ballot count and one vector atomic per
//             wavefront.  Every loop is bounded by the step bound, at most MAX_STEPS.
#include "frp_nmpc_occmap_render_scan.h"
#include "frp_occmap_raywalk.hpp"

namespace frp {
namespace occmap {
namespace render_scan {

constexpr int WAVE = 64;          // beams per workgroup = its lanes
constexpr int MAX_BEAMS = 1 << 24;

struct Shape {
    int scans, P, nb;
    double min_range, max_range, far_range;
};

__global__ void describe_kernel(int scans, int P, const double *T_ws, const int *active, double *origin, int *count, int *status)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= scans) return;
    const double *T = T_ws + 16 * (size_t)k;
    int flag = 1;
    if (active && active[k] == 0) flag = 0;
    else if (!finite_all(T, 16)) flag = FRP_OCCMAP_FUSE_REFUSED;
    status[2 * k] = flag;
    status[2 * k + 1] = 0;
    if (count) count[k] = flag == 1 ? P : 0;
    if (flag != 0)
        for (int i = 0; i < 3; i++) origin[3 * (size_t)k + i] = T[4 * i + 3];
}

using raywalk::next_axis;

__global__ __launch_bounds__(WAVE) void render_kernel(Shape sh, Geo g, const double *beams, const double *T_ws, const uint32_t *plane, double *points,
                                                      float *points_f32, double *range, int *voxel, int *status)
{
    __shared__ double tile[3 * WAVE];
    const int s = blockIdx.y;
    const int flag = status[2 * s]; // written by describe_kernel, the launch before this one
    if (flag == 0) return;           // inactive: nothing of the scan is written (the whole workgroup leaves)
    const int lane = threadIdx.x;
    const int first = blockIdx.x * WAVE; // < P: the grid has ceil(P / WAVE) workgroups per scan
    const int here = sh.P - first < WAVE ? sh.P - first : WAVE;
    const bool inside = lane < here;
    const int n = first + (inside ? lane : 0);
    const double nan = __builtin_nan("");
    double pt[3] = {nan, nan, nan}, rng = 0.0;
    int vox = -1;
    if (inside && flag == 1) {
        const double *T = T_ws + 16 * (size_t)s;
        const double b[3] = {beams[3 * (size_t)n], beams[3 * (size_t)n + 1], beams[3 * (size_t)n + 2]};
        double d[3], t[3], s_next[3], s_step[3];
        int c[3], step[3];
        for (int i = 0; i < 3; i++) {
            d[i] = (T[4 * i] * b[0] + T[4 * i + 1] * b[1]) + T[4 * i + 2] * b[2];
            t[i] = T[4 * i + 3];
        }
        const double length = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        if (finite_all(b, 3) && length > 0.0 && finite_all(&length, 1)) { // the beam is fired
            for (int k = 0; k < 3; k++) {
                c[k] = clamp_id(floored(t[k], g.origin[k], g.res_inv)); // posToIndex
                step[k] = 0; s_next[k] = INFINITY; s_step[k] = INFINITY;
                if (d[k] > 0.0) {
                    step[k] = 1;
                    const double face = g.origin[k] + (double)(c[k] + 1) * g.res;
                    s_next[k] = (face - t[k]) / d[k];
                    s_step[k] = g.res / fabs(d[k]);
                } else if (d[k] < 0.0) {
                    step[k] = -1;
                    const double face = g.origin[k] + (double)c[k] * g.res;
                    s_next[k] = (face - t[k]) / d[k];
                    s_step[k] = g.res / fabs(d[k]);
                }
            }
            int held = -1;      // index of the plane word in `word`
            uint32_t word = 0;
            const auto occupied = [&]() {
                if ((unsigned)c[0] >= (unsigned)g.grid[0] || (unsigned)c[1] >= (unsigned)g.grid[1] || (unsigned)c[2] >= (unsigned)g.grid[2]) return false;
                const int w = (c[0] * g.grid[1] + c[1]) * g.wz + (c[2] >> 5);
                if (w != held) { word = plane[w]; held = w; }
                return ((word >> (c[2] & 31)) & 1u) != 0;
            };
            bool hit = false;
            double s_mid = 0.0;
            if (!occupied()) { // a sensor inside an obstacle sees nothing
                for (int m = 0; m < sh.nb; m++) {
                    const int a = next_axis(s_next);
                    const double s_in = s_next[a];
                    if (!(s_in * length <= sh.max_range)) break;
                    // (c, step, s_next, s_step stay in registers: the three axes are written out, no indexing by a)
                    if (a == 0) { c[0] += step[0]; s_next[0] = s_next[0] + s_step[0]; }
                    else if (a == 1) { c[1] += step[1]; s_next[1] = s_next[1] + s_step[1]; }
                    else { c[2] += step[2]; s_next[2] = s_next[2] + s_step[2]; }
                    if (occupied()) {
                        const double s_out = s_next[next_axis(s_next)];
                        s_mid = (s_in + s_out) / 2.0;
                        const double r = s_mid * length;
                        if (!(r < sh.min_range)) {
                            hit = true;
                            rng = r;
                            vox = (c[0] * g.grid[1] + c[1]) * g.grid[2] + c[2];
                        }
                        break; // the walk does not go on behind the hit
                    }
                }
            }
            if (hit) {
                for (int i = 0; i < 3; i++) pt[i] = t[i] + s_mid * d[i];
            } else if (sh.far_range > 0.0) {
                const double s_far = sh.far_range / length;
                for (int i = 0; i < 3; i++) pt[i] = t[i] + s_far * d[i];
            }
        }
    }
    for (int i = 0; i < 3; i++) tile[3 * lane + i] = pt[i];
    if (inside) {
        const size_t at = (size_t)s * (size_t)sh.P + (size_t)n;
        if (range) range[at] = rng;
        if (voxel) voxel[at] = vox;
    }
    __syncthreads(); // every lane of the workgroup arrives: the only exit above is taken by all of them
    const size_t base = 3 * ((size_t)s * (size_t)sh.P + (size_t)first); // the last element written is 3 * (s * P + first + here) - 1 < 3 * S * P
    if (points)
        for (int i = lane; i < 3 * here; i += WAVE) points[base + i] = tile[i];
    if (points_f32)
        for (int i = lane; i < 3 * here; i += WAVE) points_f32[base + i] = (float)tile[i];
    const unsigned long long hits = __ballot(vox >= 0);
    if (lane == 0 && hits != 0) atomicAdd(&status[2 * s + 1], __popcll(hits));
}

// Everything that can be refused on the host (no pose, no beam: they are on the device)
static bool plan(const frp_nmpc_occmap *m, const frp_nmpc_occmap_render_scan *r, Shape *sh)
{
    if (!valid(m) || !r) return false;
    if (r->scans < 1 || r->scans > FRP_OCCMAP_FUSE_POINTS_MAX_SCANS) return false;
    if (r->P < 1 || r->P > MAX_BEAMS) return false;
    const double par[3] = {r->min_range, r->max_range, r->far_range};
    if (!finite_all(par, 3) || !(r->min_range >= 0.0) || !(r->max_range > 0.0) || r->min_range > r->max_range) return false;
    if (r->far_range != 0.0 && !(r->far_range >= r->max_range)) return false;
    double nb;
    if (!step_bound(r->max_range, m->resolution, &nb)) return false;
    sh->scans = r->scans; sh->P = r->P; sh->nb = (int)nb;
    sh->min_range = r->min_range; sh->max_range = r->max_range; sh->far_range = r->far_range;
    return true;
}

} // namespace render_scan
} // namespace occmap
} // namespace frp

extern "C" {

int frp_nmpc_occmap_render_scan_batch(const frp_nmpc_occmap *map, const frp_nmpc_occmap_render_scan *r, void *workspace, size_t workspace_bytes,
                                      void *stream)
{
    using namespace frp::occmap;
    using namespace frp::occmap::render_scan;
    Shape sh;
    if (!args_ok(map, workspace, workspace_bytes) || !plan(map, r, &sh)) return FRP_ERR_ARG;
    if (!r->beams || !r->T_ws || !r->origin || !r->status || (!r->points && !r->points_f32)) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(describe_kernel, dim3(1), dim3(FRP_OCCMAP_FUSE_POINTS_MAX_SCANS), 0, st, sh.scans, sh.P, r->T_ws, r->active, r->origin, r->count,
                       r->status);
    hipLaunchKernelGGL(render_kernel, dim3((unsigned)((sh.P + WAVE - 1) / WAVE), (unsigned)sh.scans), dim3(WAVE), 0, st, sh, geo(map), r->beams, r->T_ws,
                       static_cast<const uint32_t *>(workspace), r->points, r->points_f32, r->range, r->voxel, r->status);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

} // extern "C"
