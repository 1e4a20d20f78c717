/* frp_nmpc.h section (8), second part: depth-image fusion into the device occupancy map.  frp_nmpc.h includes it, and including
 * it alone works too (it pulls in frp_nmpc.h for frp_nmpc_occmap and carries its own extern "C").
 * Why a file of its own: tests/test_occmap_cpu.py pins the exact set of frp_nmpc_occmap_* names that frp_nmpc.h itself declares,
 * and that test is not this change's to edit.  The price: the "every declared symbol is exported" check of tests/test_capi_cpu.py
 * reads frp_nmpc.h only, so these two prototypes are covered by tests/test_occmap_fusion_cpu.py and by the load-time check of
 * solver.FUSE_EXPORTS instead.  Same section, same ABI version.
 *
 * One camera frame is fused the way OccMap::depthCallback does it (occ_grid/src/occ_map.cpp:291-292): projectDepthImage
 * (:314-439) turns the scanned pixels into world points, raycastProcess (:441-533) casts a ray from every point back to the
 * camera (RayCaster::setInput / step, raycast.cpp:263-366), counts per voxel how often it was traversed (cache_all_) and how often
 * it was a ray end (cache_hit_), and adds prob_hit_log or prob_miss_log to every touched voxel, clamped.  The result is the
 * reference's serial result TO THE BIT, including its two order-dependent early exits:
 *   * cache_rayend_ -- of the points that end in one voxel, the first in scan order casts the ray -- is an atomic minimum of the
 *     scan index;
 *   * cache_traverse_ -- a ray stops at the first voxel a ray BEFORE it in scan order has marked -- is solved by rounds: every ray
 *     starts with its whole path; a round marks every voxel with the lowest ray whose current prefix holds it, then cuts every
 *     ray at the first voxel marked by a lower ray.  After k + 1 rounds rays 0 ... k are final, the fixed point is unique and is
 *     the serial scan.  Real frames need a few dozen rounds.
 * max_rounds rounds are launched; a round after the first that changed nothing returns at once.  If no round within max_rounds
 * changes nothing, the map is left EXACTLY as it was and status[0] = -max_rounds: a partly relaxed frame is never written.
 * log_odds, occ and the bit plane are updated together for the touched voxels, so local_view and query see the frame without a
 * refresh.
 *
 * Evaluation order (the reference's Eigen expressions, written down; tests/occmap_fusion_oracle.py is the executable statement):
 *   p_cam = ((u - K[2]) * depth / K[0], (v - K[5]) * depth / K[4], depth),  depth = pixel / depth_scale
 *   p_w[i] = ((R[i][0] * x + R[i][1] * y) + R[i][2] * z) + t[i],  length = sqrt((dx * dx + dy * dy) + dz * dz)
 *   clipped end = (d / length) * max_ray_length + t per component;  the RayCaster takes p / resolution per component
 *   shift filter: q = p_w - last_t, r = last_R^-1 q in the same order, last_R^-1 = adjugate / determinant computed once on the host.
 * RayCaster::step ends only on the end cell and rounding can make it miss it (the reference then never returns): every traversal
 * here takes at most 3 * (ceil(max_ray_length / resolution) + 2) steps, which no ray that reaches its end needs. */
#ifndef FRP_NMPC_OCCMAP_FUSE_H
#define FRP_NMPC_OCCMAP_FUSE_H

#include "frp_nmpc.h" /* (a no-op when frp_nmpc.h is the includer) */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct frp_nmpc_occmap_fuse {
    int rows, cols;                  /* the depth image (cv::Mat rows, cols)                                                   */
    const unsigned short *depth;     /* [rows][cols] device, uint16 (depth_image.at<uint16_t>(v, u), :331)                      */
    const unsigned short *last_depth;/* [rows][cols] device or NULL.  NULL: the unfiltered loops (:327-355).  Otherwise the shift
                                        filter (:364-419) against the previous frame: a point that reprojects into the previous image
                                        is kept when |last_depth / depth_scale - z| < depth_filter_tolerance, one that reprojects
                                        outside it is kept.  (The reference projects nothing on its first filtered frame,
                                        has_first_depth_: the caller simply does not call.)                                    */
    double last_T_wc[16];            /* HOST, row-major 4 x 4: the previous frame's pose; read only with last_depth             */
    double K[9];                     /* HOST, row-major 3 x 3 intrinsics: fx = K[0], cx = K[2], fy = K[4], cy = K[5]            */
    double T_wc[16];                 /* HOST, row-major 4 x 4 camera-to-world pose; its translation is the ray origin t_wc      */
    double depth_scale;              /* occ_map/depth_scale (1000), > 0                                                         */
    double depth_filter_mindist;     /* pixels with depth below it are skipped (:334)                                           */
    double depth_filter_tolerance;
    int depth_filter_margin;         /* v, u run from margin to rows - margin, cols - margin EXCLUSIVE (:327-329), >= 0         */
    int skip_pixel;                  /* ... in steps of skip_pixel, >= 1                                                        */
    double prob_hit_log, prob_miss_log; /* the update of a voxel with hit >= all - hit, and of the others (:512-513)            */
    double min_ray_length, max_ray_length; /* shorter rays are dropped (:459), longer ones clipped and end in a miss (:461-465) */
    int max_rounds;                  /* relaxation rounds launched; 0: FRP_OCCMAP_FUSE_DEFAULT_ROUNDS; at most 255              */
    int *status;                     /* [2] device out: [0] rounds used, counted up to and including the first that changed nothing
                                        (>= 1), or -max_rounds: not converged, map untouched; [1] rays cast (points that passed the
                                        length test and the end-voxel dedup)                                                    */
} frp_nmpc_occmap_fuse;

#define FRP_OCCMAP_FUSE_DEFAULT_ROUNDS 128

/* Bytes of the fusion workspace for this map and frame description (image size, margin, skip, max_ray_length; the pose does not
 * enter); 0 for a description that frp_nmpc_occmap_fuse_depth refuses.  The pointers of `f` are not looked at. */
size_t frp_nmpc_occmap_fuse_workspace_bytes(const frp_nmpc_occmap *map, const frp_nmpc_occmap_fuse *f);

/* Fuse one frame.  workspace: the MAP's workspace (the bit plane).  fuse_workspace: scratch of its own -- the caller neither
 * initialises it nor has to preserve it between calls.  Asynchronous on `stream`, no host synchronisation, capturable into a
 * hipGraph (K, the poses and the parameters are read during the call).
 * FRP_ERR_ARG before anything is launched: a map the other calls refuse, a null f / depth / status, rows or cols < 1 or more than
 * 2^24 scanned pixels, a non-finite K / T_wc / parameter, with last_depth a non-finite last_T_wc or a singular rotation in it,
 * skip_pixel < 1, margin < 0, depth_scale <= 0, max_ray_length < min_ray_length, a step bound
 * 3 * (ceil(max_ray_length / resolution) + 2) above 4096, max_rounds < 0 or > 255, a short workspace of either kind.
 * FRP_ERR_NO_DEVICE without a device. */
int frp_nmpc_occmap_fuse_depth(const frp_nmpc_occmap *map, const frp_nmpc_occmap_fuse *f, void *workspace, size_t workspace_bytes,
                               void *fuse_workspace, size_t fuse_workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FRP_NMPC_OCCMAP_FUSE_H */
