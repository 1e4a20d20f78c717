// frp_nmpc.h section (8), frp_nmpc_occmap_render.h: F depth images rendered from the device occupancy map's bit plane, one ray per
// pixel, and the camera poses of a batch of planner states.  The reference has no counterpart (its images come from a simulator):
// tests/occmap_render_oracle.py is the specification, and every double computed here is computed in the order it writes down.
// Compiled with -ffp-contract=off like frp_occmap_fuse.hip.
//
//   describe  one lane per frame: status[f] = {1, 0} rendered, {0, 0} inactive, {FRP_OCCMAP_FUSE_REFUSED, 0} a non-finite T_wc[f].
//             Rotation and translation are entries of T_wc[f] as they stand, so the flag is all that has to be handed on, and
//             status[f][0] carries it: no scratch.
//   render    one lane per pixel, one 8 x 8 pixel tile per wavefront (four tiles, 16 x 16 pixels, per workgroup): neighbouring rays
//             walk neighbouring columns of the bit plane and share its cache lines, and a tile's rays are of similar length, which
//             is what bounds the divergence of the walk (the same text as frp_occmap_render_scan.hip's: frp_occmap_raywalk.hpp says why).  The frame's flag and pose are read through wave-uniform addresses.  A lane
//             keeps the last word of the plane it loaded: a step along z inside a word costs no load.  status[f][1] is one ballot
//             count and one vector atomic per wavefront.  Every loop is bounded by the step bound, at most MAX_STEPS.
//   poses     one lane per planner: T_wc = T_wb(state) * T_bc with the model's rotation (frp_model.hpp).
#include "frp_nmpc_occmap_render.h"
#include "frp_model.hpp"
#include "frp_occmap_fuse.hpp"
#include "frp_occmap_raywalk.hpp"

namespace frp {
namespace occmap {
namespace render {

constexpr int TILE = 8, BLOCK_TILES = 2, BLOCK_PIX = TILE * BLOCK_TILES; // a workgroup: 2 x 2 tiles of 8 x 8 pixels, one per wavefront

struct Shape {
    int frames, rows, cols, tiles_u, nb;
    double fx, cx, fy, cy, depth_scale, max_range;
};

__global__ void describe_kernel(int frames, const double *T_wc, const int *active, int *status)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= frames) return;
    int flag = 1;
    if (active && active[k] == 0) flag = 0;
    else if (!finite_all(T_wc + 16 * (size_t)k, 16)) flag = FRP_OCCMAP_FUSE_REFUSED;
    status[2 * k] = flag;
    status[2 * k + 1] = 0;
}

using raywalk::next_axis;

__global__ __launch_bounds__(256) void render_kernel(Shape sh, Geo g, const double *T_wc, const uint32_t *plane, unsigned short *depth, int *voxel,
                                                     int *status)
{
    const int f = blockIdx.y;
    const int flag = status[2 * f]; // written by describe_kernel, the launch before this one
    if (flag == 0) return;           // inactive: the image is not written
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int bu = blockIdx.x % sh.tiles_u, bv = blockIdx.x / sh.tiles_u;
    const int u = bu * BLOCK_PIX + (wave & 1) * TILE + (lane & 7), v = bv * BLOCK_PIX + (wave >> 1) * TILE + (lane >> 3);
    const bool inside = u < sh.cols && v < sh.rows;
    const size_t at = ((size_t)f * sh.rows + (inside ? v : 0)) * sh.cols + (inside ? u : 0);
    int pix = 0, vox = -1;
    if (inside && flag == 1) {
        const double *T = T_wc + 16 * (size_t)f;
        const double dcx = ((double)u - sh.cx) / sh.fx, dcy = ((double)v - sh.cy) / sh.fy;
        double d[3], t[3], s_next[3], s_step[3];
        int c[3], step[3];
        for (int i = 0; i < 3; i++) {
            d[i] = (T[4 * i] * dcx + T[4 * i + 1] * dcy) + T[4 * i + 2];
            t[i] = T[4 * i + 3];
        }
        const double length = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
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
        if (!occupied()) { // a camera inside an obstacle sees nothing
            for (int n = 0; n < sh.nb; n++) {
                const int a = next_axis(s_next);
                const double s_in = s_next[a];
                if (!(s_in * length <= sh.max_range)) break;
                // (c, step, s_next, s_step stay in registers: the three axes are written out, no indexing by a)
                if (a == 0) { c[0] += step[0]; s_next[0] = s_next[0] + s_step[0]; }
                else if (a == 1) { c[1] += step[1]; s_next[1] = s_next[1] + s_step[1]; }
                else { c[2] += step[2]; s_next[2] = s_next[2] + s_step[2]; }
                if (occupied()) {
                    const double s_out = s_next[next_axis(s_next)];
                    const double s_mid = (s_in + s_out) / 2.0;
                    const double p = floor(s_mid * sh.depth_scale + 0.5);
                    if (p >= 1.0 && p <= 65535.0) {
                        pix = (int)p;
                        vox = (c[0] * g.grid[1] + c[1]) * g.grid[2] + c[2];
                    }
                    break;
                }
            }
        }
    }
    if (inside) {
        depth[at] = (unsigned short)pix;
        if (voxel) voxel[at] = vox;
    }
    const unsigned long long hits = __ballot(pix != 0);
    if (lane == 0 && hits != 0) atomicAdd(&status[2 * f + 1], __popcll(hits));
}

struct Mat4 {
    double m[4][4];
};

__global__ void poses_kernel(int B, const double *state, double *T_wc, Mat4 Bc)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= B) return;
    const double *x = state + 9 * (size_t)k;
    const double e[3] = {x[6], x[7], x[8]};
    const Trig tg = make_trig(e);
    const double sr = tg.sr, cr = tg.cr, sp = tg.sp, cp = tg.cp, sy = tg.sy, cy = tg.cy;
    // T_wb, the entries of workloads._rot in its operation order
    const double A[4][4] = {{cy * cp, cy * sp * sr - cr * sy, cy * sp * cr + sy * sr, x[0]},
                            {cp * sy, cy * cr + sy * sp * sr, sy * sp * cr - cy * sr, x[1]},
                            {-sp, cp * sr, cp * cr, x[2]},
                            {0.0, 0.0, 0.0, 1.0}};
    double *out = T_wc + 16 * (size_t)k;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) out[4 * i + j] = ((A[i][0] * Bc.m[0][j] + A[i][1] * Bc.m[1][j]) + A[i][2] * Bc.m[2][j]) + A[i][3] * Bc.m[3][j];
}

// Everything that can be refused on the host (no pose: they are on the device)
static bool plan(const frp_nmpc_occmap *m, const frp_nmpc_occmap_render *r, Shape *sh)
{
    if (!valid(m) || !r) return false;
    if (r->frames < 1 || r->frames > FRP_OCCMAP_FUSE_MAX_FRAMES) return false;
    if (r->rows < 1 || r->cols < 1 || (long long)r->rows * r->cols > (long long)fuse::MAX_PIXELS) return false;
    if (!finite_all(r->K, 9) || r->K[0] == 0.0 || r->K[4] == 0.0) return false;
    const double par[2] = {r->depth_scale, r->max_range};
    if (!finite_all(par, 2) || !(r->depth_scale > 0.0) || !(r->max_range > 0.0)) return false;
    double nb;
    if (!step_bound(r->max_range, m->resolution, &nb)) return false;
    sh->frames = r->frames; sh->rows = r->rows; sh->cols = r->cols;
    sh->tiles_u = (r->cols + BLOCK_PIX - 1) / BLOCK_PIX;
    sh->nb = (int)nb;
    sh->fx = r->K[0]; sh->cx = r->K[2]; sh->fy = r->K[4]; sh->cy = r->K[5];
    sh->depth_scale = r->depth_scale; sh->max_range = r->max_range;
    return true;
}

} // namespace render
} // namespace occmap
} // namespace frp

extern "C" {

int frp_nmpc_occmap_render_depth(const frp_nmpc_occmap *map, const frp_nmpc_occmap_render *r, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace frp::occmap;
    using namespace frp::occmap::render;
    Shape sh;
    if (!args_ok(map, workspace, workspace_bytes) || !plan(map, r, &sh)) return FRP_ERR_ARG;
    if (!r->T_wc || !r->depth || !r->status) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned tiles_v = (unsigned)((sh.rows + BLOCK_PIX - 1) / BLOCK_PIX); // tiles_u * tiles_v <= 2^24 / 256 + rows + cols: far inside a grid's x
    hipLaunchKernelGGL(describe_kernel, dim3(1), dim3(FRP_OCCMAP_FUSE_MAX_FRAMES), 0, st, sh.frames, r->T_wc, r->active, r->status);
    hipLaunchKernelGGL(render_kernel, dim3((unsigned)sh.tiles_u * tiles_v, (unsigned)sh.frames), dim3(256), 0, st, sh, geo(map), r->T_wc,
                       static_cast<const uint32_t *>(workspace), r->depth, r->voxel, r->status);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

int frp_nmpc_occmap_camera_poses(int B, const double *state, const double T_bc[16], double *T_wc, void *stream)
{
    using namespace frp::occmap;
    if (B < 0 || !T_bc || (B > 0 && (!state || !T_wc))) return FRP_ERR_ARG;
    if (!device_ok()) return FRP_ERR_NO_DEVICE;
    if (B == 0) return FRP_OK;
    render::Mat4 Bc;
    for (int i = 0; i < 16; i++) Bc.m[i / 4][i % 4] = T_bc[i];
    hipLaunchKernelGGL(render::poses_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), B, state, T_wc, Bc);
    return hipGetLastError() == hipSuccess ? FRP_OK : FRP_ERR_HIP;
}

} // extern "C"
