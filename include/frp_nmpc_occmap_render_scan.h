/* frp_nmpc.h section (8): point scans RENDERED from the device occupancy map -- the range sensor of a simulated fleet that is not a
 * pinhole camera (a spinning LiDAR, a ToF array).  The point-scan sibling of frp_nmpc_occmap_render.h: for S sensor poses and a table
 * of P beam directions it returns the points such a sensor measures in the map, in beam order and in the format
 * frp_nmpc_occmap_fuse_points_batch reads, with the scan origins and counts written on the device, so that
 * camera_poses -> render_scan_batch (on the world) -> fuse_points_batch (on the belief) runs with nothing on the host and can be
 * captured with the tick.  frp_nmpc.h includes this file, and including it alone works too (it pulls in frp_nmpc.h and carries its own
 * extern "C").  A header of its own for the reason frp_nmpc_occmap_fuse.h gives: tests/test_occmap_cpu.py pins the frp_nmpc_occmap_*
 * names that frp_nmpc.h itself declares.  The prototype is covered by tests/test_occmap_scan_cpu.py and by the load-time check of
 * solver.RENDER_SCAN_EXPORTS.  Same section, same ABI version, no existing struct changed.
 *
 * NO COUNTERPART IN THE REFERENCE, like the depth renderer.  tests/occmap_scan_oracle.py is the SPECIFICATION (plain doubles, one
 * statement per operation); the kernel follows it to the bit.
 *
 * Beam p of scan s, with R and t the rotation and translation of T_ws[s] and b = beams[p]:
 *   d_w[i] = (R[i][0] * b[0] + R[i][1] * b[1]) + R[i][2] * b[2],  length = sqrt((d0*d0 + d1*d1) + d2*d2);
 * the ray is t + s * d_w and the metres along the beam are s * length.  The table need not be normalised.  A beam with a non-finite
 * component, or whose length is 0 or not finite, is NOT FIRED: its point is NaN whatever far_range is.
 * The walk is the depth renderer's: from the sensor's cell (posToIndex of t), an exact slab traversal with the true direction -- per
 * axis the next face crossing (face - t) / d_w and the spacing resolution / |d_w|, the comparison tree of RayCaster::step; an axis
 * with a zero direction component is never stepped along.  A cell outside the map is free, a sensor outside the map looks in, a
 * sensor whose own cell is occupied sees nothing.  The walk ends in the first occupied voxel, when s_in * length exceeds max_range at
 * a cell's entry, or after 3 * (ceil(max_range / resolution) + 2) steps.
 * A return is the MIDPOINT of the ray's segment inside the hit voxel, s_mid = (s_in + s_out) / 2, range = s_mid * length,
 * point[i] = t[i] + s_mid * d_w[i] -- for the reason frp_nmpc_occmap_render.h gives: a point on the entry face would index into either
 * neighbour and fusing the scan would grow every obstacle towards the sensor.  A hit with range < min_range is no return, and the
 * walk does not go on behind it.
 * A fired beam without a return gives a NaN point when far_range is 0 -- the "no return" that fuse_points drops -- and otherwise the
 * point at far_range metres along the beam, s_far = far_range / length, point[i] = t[i] + s_far * d_w[i]: fused with
 * max_ray_length < far_range it is a miss, and free space is carved along the beam.  Its range is 0 and its voxel -1 like every
 * beam's without a return, and status[s][1] counts returns only.
 *
 * Like every call of this section: asynchronous on `stream`, allocates nothing, reads nothing back, capturable; beams, T_ws and
 * active are DEVICE arrays read when the kernels run, so a replayed capture sees what the caller has written since.  Only the bit
 * plane is read: log_odds and occ are not touched.  Two launches per call. */
#ifndef FRP_NMPC_OCCMAP_RENDER_SCAN_H
#define FRP_NMPC_OCCMAP_RENDER_SCAN_H

#include "frp_nmpc.h" /* (a no-op when frp_nmpc.h is the includer) */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct frp_nmpc_occmap_render_scan {
    int scans;              /* S >= 1, <= FRP_OCCMAP_FUSE_POINTS_MAX_SCANS                                                   */
    int P;                  /* beams per scan, 1 <= P <= 2^24                                                                */
    const double *beams;    /* [P][3] DEVICE: beam directions in the SENSOR frame, any length, shared by the scans; the index
                               is the firing order and becomes the point index                                              */
    const double *T_ws;     /* [S][16] DEVICE row-major sensor-to-world (what frp_nmpc_occmap_camera_poses writes)           */
    const int *active;      /* [S] DEVICE or NULL; 0: the scan is not rendered                                               */
    double min_range, max_range; /* metres along the beam; 0 <= min_range <= max_range, max_range > 0                        */
    double far_range;       /* 0: a beam without a return gives a NaN point.  >= max_range: it gives the point at far_range
                               along the beam, which fusion with max_ray_length < far_range treats as a miss and carves free
                               space along                                                                                   */
    double *points;         /* [S][P][3] DEVICE out or NULL  } at least one; both may be given; the float is                 */
    float *points_f32;      /* [S][P][3] DEVICE out or NULL  } the double rounded once to nearest                            */
    double *origin;         /* [S][3] DEVICE out: the translation of T_ws[s] as it stands (fuse_points' origin)              */
    int *count;             /* [S] DEVICE out or NULL: P for a rendered scan, 0 otherwise                                    */
    double *range;          /* [S][P] DEVICE out or NULL: metres along the beam of the return, 0 where none                  */
    int *voxel;             /* [S][P] DEVICE out or NULL: linear index (x * gy + y) * gz + z of the hit voxel, -1 where none */
    int *status;            /* [S][2] DEVICE out: {1, returns} rendered / {0, 0} inactive (nothing of the scan is written but
                               count = 0) / {FRP_OCCMAP_FUSE_REFUSED, 0} a non-finite T_ws[s] (points NaN, range 0, voxel -1,
                               count 0, origin as it stands -- fuse_points refuses it too)                                   */
} frp_nmpc_occmap_render_scan;

/* Render the S scans.  workspace: the MAP's workspace (the bit plane), the only thing read; no scratch.
 * FRP_ERR_ARG before anything is launched: a map the other calls refuse; a null r, beams, T_ws, origin or status; both point outputs
 * null; scans < 1 or above FRP_OCCMAP_FUSE_POINTS_MAX_SCANS; P < 1 or above 2^24; a min_range that is not finite or negative; a
 * max_range that is not finite or <= 0; min_range > max_range; a far_range that is neither 0 nor a finite value >= max_range; a step
 * bound 3 * (ceil(max_range / resolution) + 2) above 4096; a short workspace.  FRP_ERR_NO_DEVICE without a device. */
int frp_nmpc_occmap_render_scan_batch(const frp_nmpc_occmap *map, const frp_nmpc_occmap_render_scan *r, void *workspace, size_t workspace_bytes,
                                      void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FRP_NMPC_OCCMAP_RENDER_SCAN_H */
