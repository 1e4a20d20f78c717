/* frp_nmpc.h section (8), fourth part: a BATCH of depth frames fused into the device occupancy map in one call.  frp_nmpc.h includes
 * it, and including it alone works too (it pulls in frp_nmpc.h and carries its own extern "C").  A file of its own for the reason
 * frp_nmpc_occmap_fuse.h gives: tests/test_occmap_cpu.py pins the frp_nmpc_occmap_* names that frp_nmpc.h itself declares.  The two
 * prototypes are covered by tests/test_occmap_fusion_batch_cpu.py and by the load-time check of solver.FUSE_BATCH_EXPORTS.  Same
 * section, same ABI version.
 *
 * What a call computes.  After it, log_odds, occ and the bit plane are BIT FOR BIT what frp_nmpc_occmap_fuse_depth
 * (frp_nmpc_occmap_fuse.h) leaves after being called for frames 0, 1, ..., F - 1 in that order with the same parameters; frames that
 * are inactive, refused or not converged are skipped in that chain.  Why this is exact: projectDepthImage and the ray loop of
 * raycastProcess (occ_map.cpp:314-503) never read the map -- which voxels a frame touches, and whether each gets the hit or the miss
 * increment, depends on that frame alone -- so the F frames project, deduplicate and relax at the same time, each in its own slice
 * of the workspace.  Only the batch update (:505-532) reads the map, per voxel: every voxel then applies the frames' increments in
 * frame order (the clamps do not commute), carries the value in a register and is written once.
 *
 * Nothing about a pose is read on the host: T_wc, last_T_wc, active, the images and status are DEVICE arrays, read when the kernels
 * run.  The call is asynchronous on `stream`, allocates nothing, reads nothing back, and a captured call replays with whatever the
 * caller has written into those arrays since.  Rotation, translation, last_R^-1 (adjugate / determinant, the order of
 * frp_nmpc_occmap_fuse.h) and the ray box of every frame are computed by one lane per frame, with the host code's operations.
 *
 * status[f] = {rounds, rays} with the single-frame call's meaning for frame f, and
 *   {0, 0}                          active[f] == 0: the frame is not fused;
 *   {-max_rounds, rays}             no fixed point within max_rounds: the frame contributes nothing (a partly relaxed frame is never
 *                                   written), the other frames are fused as usual;
 *   {FRP_OCCMAP_FUSE_REFUSED, 0}    a pose the single-frame call refuses on the host: a non-finite entry of T_wc[f]; with last_depth, a
 *                                   non-finite last_T_wc[f] or a rotation in it whose adjugate / determinant inverse is not finite.
 *                                   (Also a ray box larger than the pose-independent bound that sizes the workspace, which no
 *                                   finite pose produces.)  A refused frame contributes nothing and stops nothing.
 *
 * Launches per call: 2 * max_rounds + 7, whatever F (the frame is the second grid dimension of every stage; one update launch). */
#ifndef FRP_NMPC_OCCMAP_FUSE_BATCH_H
#define FRP_NMPC_OCCMAP_FUSE_BATCH_H

#include "frp_nmpc.h" /* (a no-op when frp_nmpc.h is the includer) */

#ifdef __cplusplus
extern "C" {
#endif

#define FRP_OCCMAP_FUSE_MAX_FRAMES 64
#define FRP_OCCMAP_FUSE_REFUSED (-256) /* below every -max_rounds (max_rounds <= 255) */

typedef struct frp_nmpc_occmap_fuse_batch {
    int frames;                       /* F >= 1, at most FRP_OCCMAP_FUSE_MAX_FRAMES                                             */
    int rows, cols;                   /* every frame has this size                                                              */
    const unsigned short *depth;      /* [F][rows][cols] DEVICE                                                                 */
    const unsigned short *last_depth; /* [F][rows][cols] DEVICE or NULL (NULL: the unfiltered loops for every frame)            */
    const double *T_wc;               /* [F][16] DEVICE, row-major 4 x 4                                                        */
    const double *last_T_wc;          /* [F][16] DEVICE; required with last_depth, otherwise not read                           */
    const int *active;                /* [F] DEVICE or NULL; 0: the frame is not fused, its status is {0, 0}                    */
    double K[9];                      /* HOST, shared by the frames                                                             */
    double depth_scale;               /* the fields from here to max_rounds: as in frp_nmpc_occmap_fuse, shared by the frames   */
    double depth_filter_mindist;
    double depth_filter_tolerance;
    int depth_filter_margin;
    int skip_pixel;
    double prob_hit_log, prob_miss_log;
    double min_ray_length, max_ray_length;
    int max_rounds;
    int *status;                      /* [F][2] DEVICE out                                                                      */
} frp_nmpc_occmap_fuse_batch;

/* Bytes of the fusion workspace for this map and batch description: F frame slices of the single-frame layout
 * (frp_nmpc_occmap_fuse_workspace_bytes for the same image and parameters) plus the per-frame descriptors.  0 for a description
 * that frp_nmpc_occmap_fuse_depth_batch refuses.  The pointers of `f` are not looked at. */
size_t frp_nmpc_occmap_fuse_batch_workspace_bytes(const frp_nmpc_occmap *map, const frp_nmpc_occmap_fuse_batch *f);

/* Fuse the batch.  workspace: the MAP's workspace (the bit plane).  fuse_workspace: scratch -- it arrives uninitialised and need not
 * be preserved between calls.  FRP_ERR_ARG before anything is launched: everything frp_nmpc_occmap_fuse_depth refuses that does not
 * involve a pose (the map, the image size, K, the parameters, max_rounds, the step bound), frames < 1 or above
 * FRP_OCCMAP_FUSE_MAX_FRAMES, a null depth / T_wc / status, last_depth without last_T_wc, a short workspace of either kind, a
 * fuse_workspace that is not 8-byte aligned.  FRP_ERR_NO_DEVICE without a device. */
int frp_nmpc_occmap_fuse_depth_batch(const frp_nmpc_occmap *map, const frp_nmpc_occmap_fuse_batch *f, void *workspace, size_t workspace_bytes,
                                     void *fuse_workspace, size_t fuse_workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FRP_NMPC_OCCMAP_FUSE_BATCH_H */
