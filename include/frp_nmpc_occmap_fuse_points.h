/* frp_nmpc.h section (8), the part for sensors that are not a pinhole depth camera: a BATCH of point-cloud scans (a spinning LiDAR, a
 * stereo rig, a ToF array, a simulator's scan) ray-cast into the device occupancy map in one call.  frp_nmpc.h includes it, and
 * including it alone works too (it pulls in frp_nmpc.h and carries its own extern "C").  A file of its own for the reason
 * frp_nmpc_occmap_fuse.h gives: tests/test_occmap_cpu.py pins the frp_nmpc_occmap_* names that frp_nmpc.h itself declares.  The two
 * prototypes are covered by tests/test_occmap_fuse_points_cpu.py and by the load-time check of solver.FUSE_POINTS_EXPORTS.  Same
 * section, same ABI version, no existing struct changed.
 *
 * What a call computes.  The reference's fusion has a seam: projectDepthImage (occ_map.cpp:314-439) fills proj_points_, and
 * raycastProcess(t_wc) (:441-533) reads nothing but those world points and the sensor position.  This entry is raycastProcess for S
 * scans.  After the call, log_odds, occ and the bit plane are BIT FOR BIT what results from running, for s = 0, 1, ..., S - 1 in
 * that order, raycastProcess(origin[s]) over points[s][0 .. count[s]) in index order -- the index is the scan order that
 * cache_rayend_ (the first point of an end voxel casts the ray, :470-478) and cache_traverse_ (:494-501) depend on.  Scans that are
 * inactive, refused or not converged are skipped in that chain.  The ray loop never reads the map, so the S scans deduplicate and
 * relax at the same time, each in its own slice of the workspace; the update (:505-532) is applied per voxel in scan order (the
 * clamps do not commute) on a value carried in a register, written once -- as frp_nmpc_occmap_fuse_batch.h does for depth frames.
 * From the ray set-up on, the code IS that of the depth entries (frp_occmap_fuse.hpp); only the stage that produces the points
 * differs: a load where they project.
 *
 * The rules of frp_nmpc_occmap_fuse.h hold unchanged: its "Evaluation order" (length = sqrt((dx*dx + dy*dy) + dz*dz), the clipped end
 * d / length * max_ray_length + origin per component, p / resolution per component), the step bound
 * 3 * (ceil(max_ray_length / resolution) + 2) <= 4096, the ray box from origin -/+ max_ray_length that sizes the per-voxel arrays,
 * and the rule that a round that changed nothing ends the work.
 *
 * NON-FINITE POINTS -- the one deliberate departure from the reference.  LiDAR drivers mark "no return" with NaN or an infinity.  The
 * reference would hand such a point to posToIndex, an undefined float -> int cast.  Here a point with ANY non-finite coordinate is
 * dropped, as if it were not in the scan: it casts no ray and touches no voxel.  It keeps its index, and later points keep theirs.
 * A float point is widened to double exactly and then treated as a double point.
 *
 * Nothing about a scan is read on the host: points, count, origin and active are DEVICE arrays, read when the kernels run.  The call
 * is asynchronous on `stream`, allocates nothing, reads nothing back, synchronises nothing, and a captured call replays with
 * whatever the caller has written into those arrays since.
 *
 * status[s] = {rounds, rays cast}, the meanings of frp_nmpc_occmap_fuse_batch.h:
 *   {0, 0}                          active[s] == 0: the scan is not fused;
 *   {-max_rounds, rays}             no fixed point within max_rounds: the scan contributes nothing (the map is never partly written
 *                                   by it), the other scans are fused as usual;
 *   {FRP_OCCMAP_FUSE_REFUSED, 0}    origin[s] is not finite.  A refused scan contributes nothing and stops nothing;
 *   {1, 0}                          a scan without a ray (count 0, P = 0, every point dropped): what the depth route gives a frame
 *                                   without points.
 *
 * Launches per call: 2 * max_rounds + 7, whatever S and P (the scan is the second grid dimension of every stage). */
#ifndef FRP_NMPC_OCCMAP_FUSE_POINTS_H
#define FRP_NMPC_OCCMAP_FUSE_POINTS_H

#include "frp_nmpc.h" /* (a no-op when frp_nmpc.h is the includer) */

#ifdef __cplusplus
extern "C" {
#endif

#define FRP_OCCMAP_FUSE_POINTS_MAX_SCANS 64 /* = FRP_OCCMAP_FUSE_MAX_FRAMES */

typedef struct frp_nmpc_occmap_fuse_points {
    int scans;                /* S >= 1, <= FRP_OCCMAP_FUSE_POINTS_MAX_SCANS                                                   */
    int P;                    /* capacity of one scan in points, 0 <= P <= 2^24                                                */
    const double *points;     /* [S][P][3] DEVICE world frame, or NULL                                                         */
    const float *points_f32;  /* [S][P][3] DEVICE, or NULL; exactly one of the two is non-NULL (P > 0); a float is widened to
                                 double exactly, then treated as a double point                                                */
    const int *count;         /* [S] DEVICE or NULL (NULL: every scan holds P points).  count[s] is clamped to [0, P]; storage
                                 beyond count[s] is NOT read                                                                   */
    const double *origin;     /* [S][3] DEVICE: the sensor position t_wc of each scan (the ray origin)                         */
    const int *active;        /* [S] DEVICE or NULL; 0: the scan is not fused, status {0, 0}                                   */
    double prob_hit_log, prob_miss_log, min_ray_length, max_ray_length; /* as in frp_nmpc_occmap_fuse                          */
    int max_rounds;           /* 0: FRP_OCCMAP_FUSE_DEFAULT_ROUNDS; at most 255                                                */
    int *status;              /* [S][2] DEVICE out: {rounds, rays cast}, see above                                             */
} frp_nmpc_occmap_fuse_points;

/* Bytes of the fusion workspace for this map and description: S slices of the single-frame layout for P points, plus the per-scan
 * descriptors.  0 for a description that frp_nmpc_occmap_fuse_points_batch refuses.  The pointers of `f` are not looked at. */
size_t frp_nmpc_occmap_fuse_points_workspace_bytes(const frp_nmpc_occmap *map, const frp_nmpc_occmap_fuse_points *f);

/* Fuse the scans.  workspace: the MAP's workspace (the bit plane).  fuse_workspace: scratch -- it arrives uninitialised and carries
 * nothing between calls.  FRP_ERR_ARG before anything is launched: a map the other calls refuse; a null f, origin or status; both
 * or neither of points / points_f32 with P > 0; scans < 1 or above FRP_OCCMAP_FUSE_POINTS_MAX_SCANS; P < 0 or above 2^24; a
 * non-finite parameter; max_ray_length < min_ray_length; a step bound above 4096; max_rounds outside 0 ... 255; a short workspace
 * of either kind; a fuse_workspace that is not 8-byte aligned.  P = 0 is valid: every active scan with a finite origin gets
 * {1, 0} and the map is untouched.  FRP_ERR_NO_DEVICE without a device. */
int frp_nmpc_occmap_fuse_points_batch(const frp_nmpc_occmap *map, const frp_nmpc_occmap_fuse_points *f, void *workspace, size_t workspace_bytes,
                                      void *fuse_workspace, size_t fuse_workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FRP_NMPC_OCCMAP_FUSE_POINTS_H */
