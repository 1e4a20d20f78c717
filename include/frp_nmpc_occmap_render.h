/* frp_nmpc.h section (8), fifth part: depth images RENDERED from the device occupancy map -- the sensor of a simulated fleet.
 * frp_nmpc.h includes it, and including it alone works too (it pulls in frp_nmpc.h for frp_nmpc_occmap and the batch fusion's
 * constants, and carries its own extern "C").  A header of its own for the reason frp_nmpc_occmap_fuse.h gives:
 * tests/test_occmap_cpu.py pins the frp_nmpc_occmap_* names that frp_nmpc.h itself declares.  The two prototypes are covered by
 * tests/test_occmap_render_cpu.py and by the load-time check of solver.RENDER_EXPORTS.  Same section, same ABI version, no existing
 * struct changed.
 *
 * NO COUNTERPART IN THE REFERENCE: it takes its depth images from a simulator that is not in its tree.  What is shared with it is
 * the camera model of projectDepthImage (occ_grid/src/occ_map.cpp:337-340) and posToIndex (:71-75), so that the images rendered
 * here are what frp_nmpc_occmap_fuse_depth_batch takes: world -> depth -> belief map runs with nothing on the host.
 * tests/occmap_render_oracle.py is the SPECIFICATION (plain doubles, one statement per operation); the kernel follows it to the bit.
 *
 * Pixel (u, v) of frame f looks along d_cam = ((u - K[2]) / K[0], (v - K[5]) / K[4], 1), d_w[i] = (R[i][0] * d_cam[0] + R[i][1] *
 * d_cam[1]) + R[i][2]; the ray is t + s * d_w from the translation t of T_wc[f], so s is the camera-z depth projectDepthImage
 * multiplies back in.  The ray is walked cell by cell from the camera's cell (posToIndex of t) by an exact slab traversal with the
 * true direction: per axis the next face crossing s_next = (face - t) / d_w and the spacing resolution / |d_w|; an axis with a zero
 * direction component is never stepped along and nothing divides by it.  A cell outside the map is free, a camera outside the map
 * looks in.  The walk ends in the first occupied voxel, when s * |d_w| exceeds max_range at a cell's entry, or after
 * 3 * (ceil(max_range / resolution) + 2) steps.  A return writes the MIDPOINT of the ray's segment inside the hit voxel,
 * pixel = floor((s_in + s_out) / 2 * depth_scale + 0.5) -- a point on the entry face would re-project into either neighbour and
 * fusing the image would grow every obstacle towards the camera.  0 (voxel -1): no return, a value of 0 or above 65535, a camera
 * whose own cell is occupied, a refused frame.
 *
 * Like every call of this section: asynchronous on `stream`, allocates nothing, reads nothing back, capturable; T_wc, active and
 * the state array are DEVICE arrays read when the kernels run, so a replayed capture sees what the caller has written since.  Only
 * the bit plane is read: log_odds and occ are not touched.  Two launches per render call, one per camera_poses call. */
#ifndef FRP_NMPC_OCCMAP_RENDER_H
#define FRP_NMPC_OCCMAP_RENDER_H

#include "frp_nmpc.h" /* (a no-op when frp_nmpc.h is the includer) */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct frp_nmpc_occmap_render {
    int frames;                 /* F >= 1, at most FRP_OCCMAP_FUSE_MAX_FRAMES                                              */
    int rows, cols;             /* >= 1, rows * cols <= 2^24                                                               */
    const double *T_wc;         /* [F][16] DEVICE, row-major camera-to-world                                               */
    const int *active;          /* [F] DEVICE or NULL; 0: the frame is not rendered                                        */
    double K[9];                /* HOST, as in frp_nmpc_occmap_fuse                                                        */
    double depth_scale;         /* > 0; 1000 in the launch file                                                            */
    double max_range;           /* metres along the ray, > 0                                                               */
    unsigned short *depth;      /* [F][rows][cols] DEVICE out                                                              */
    int *voxel;                 /* [F][rows][cols] DEVICE out or NULL: linear voxel index (x * gy + y) * gz + z of the
                                   return, -1 where depth is 0                                                             */
    int *status;                /* [F][2] DEVICE out: {1, pixels with a return} rendered; {0, 0} inactive (its image is not
                                   written); {FRP_OCCMAP_FUSE_REFUSED, 0} a non-finite T_wc[f] (its image is zeroed)       */
} frp_nmpc_occmap_render;

/* Render the F frames.  workspace: the MAP's workspace (the bit plane), the only thing read; no scratch.
 * FRP_ERR_ARG before anything is launched: a map the other calls refuse, a null r / T_wc / depth / status, frames < 1 or above
 * FRP_OCCMAP_FUSE_MAX_FRAMES, rows or cols < 1 or rows * cols > 2^24, a non-finite K, K[0] or K[4] equal to 0, a depth_scale that
 * is not finite or <= 0, a max_range that is not finite or <= 0, a step bound 3 * (ceil(max_range / resolution) + 2) above 4096, a
 * short workspace.  FRP_ERR_NO_DEVICE without a device. */
int frp_nmpc_occmap_render_depth(const frp_nmpc_occmap *map, const frp_nmpc_occmap_render *r, void *workspace, size_t workspace_bytes,
                                 void *stream);

/* T_wc[b] = T_wb(state[b]) * T_bc for B planner states [B][9] (position, velocity, Euler angles roll, pitch, yaw; DEVICE) and the
 * body-to-camera transform T_bc (HOST, row-major 4 x 4); T_wc [B][16] DEVICE out, row-major.  T_wb = [R p; 0 0 0 1] with the
 * model's rotation R = Rz(yaw) Ry(pitch) Rx(roll) (csrc/frp_model.hpp, workloads._rot); every entry of the product is
 * ((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3.  The arithmetic of depthOdomCallback (occ_map.cpp:218-290) with Euler angles where the
 * reference has a quaternion: planner state -> pose -> render -> fuse needs no host round trip.  B = 0 launches nothing.
 * FRP_ERR_ARG: B < 0, a null T_bc, with B > 0 a null state or T_wc.  FRP_ERR_NO_DEVICE without a device. */
int frp_nmpc_occmap_camera_poses(int B, const double *state, const double T_bc[16], double *T_wc, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FRP_NMPC_OCCMAP_RENDER_H */
