/* frp_nmpc.h section (8), seventh part: SHARED CLOUDS BEYOND FRP_CORRIDOR_MAX_POINTS.  The shared-cloud route of the corridor
 * (frp_nmpc_corridor_batch_cut / _view on the whole-map cloud with its uniform grid) for maps of up to
 * FRP_CORRIDOR_LARGE_MAX_POINTS occupied voxels, and the device-built view of that capacity.  frp_nmpc.h includes it, and including
 * it alone works too (it pulls in frp_nmpc.h for frp_nmpc_corridor, frp_nmpc_corridor_cut, frp_nmpc_occmap and
 * frp_nmpc_occmap_shared_view, and carries its own extern "C").  A header of its own for the reason frp_nmpc_occmap_fuse.h gives.
 * The prototypes are covered by tests/test_corridor_large_cpu.py and by the load-time check of solver.LARGE_EXPORTS.  Same ABI
 * version: no existing struct, entry point, limit or refusal changes -- frp_nmpc_corridor_batch, _cut, _view and
 * frp_nmpc_occmap_shared_view_update keep refusing more than FRP_CORRIDOR_MAX_POINTS points.
 *
 * WHY the old limit and why it is not needed here.  FRP_CORRIDOR_MAX_POINTS comes from three bit masks over CLOUD positions in LDS
 * (3 x P / 8 bytes).  Only the last kernel of the hand-over chain, the plain-cloud workgroup kernel, indexes masks by cloud
 * position, and only for a planner whose local box holds more than 8192 points.  The one-wavefront kernel reads points through the
 * grid alone; the grid workgroup kernel works on a dense in-box list of at most 8192 entries and its masks are over LIST positions.
 * The large chain therefore runs those two kernels as they are, with LDS sized for the list, and replaces the third by a kernel
 * that gathers the in-box points through the grid into a per-workgroup list in device memory (the workspace below) and runs the
 * same scans over list positions -- masks over FRP_CORRIDOR_LARGE_LIST positions, 24 KB of LDS whatever P is.
 *
 * Results: bit for bit those of the plain-cloud kernel on the same visible points -- the per-point expressions are the shared ones
 * and minima are tie-broken by original cloud index -- hence those of frp_nmpc_corridor_batch on per-planner clouds
 * (frp_nmpc_occmap_local_view) when the cut carries that view's local_box rows.
 *
 * A local box with more than FRP_CORRIDOR_LARGE_LIST points in it is REFUSED for that planner, never answered with a wrong
 * polytope:  overflow[b] = 1,  poly_count[b] = INT_MIN (where given),  poly_nfaces[b][0 .. N) = 0,  poly_index[b][0 .. N) = 0.
 * Every other planner of the batch gets overflow[b] = 0 and the result it would have had without that planner.  (65 536 points of
 * a 0.1 m voxel map fill the reference's 4.1 x 4 x 2 m local box twice over.) */
#ifndef FRP_NMPC_CORRIDOR_LARGE_H
#define FRP_NMPC_CORRIDOR_LARGE_H

#include "frp_nmpc.h" /* (a no-op when frp_nmpc.h is the includer) */

#ifdef __cplusplus
extern "C" {
#endif

#define FRP_CORRIDOR_LARGE_MAX_POINTS (1 << 22)   /* shared cloud / view capacity of the large entries       */
#define FRP_CORRIDOR_LARGE_LIST       65536       /* in-box points one planner may hold in the fallback list */
#define FRP_CORRIDOR_LARGE_GROUPS     512         /* workgroups (= lists in the workspace) of the fallback   */

typedef struct frp_nmpc_corridor_large {
    void  *workspace;       /* device, frp_nmpc_corridor_large_workspace_bytes(B) bytes: the fallback's lists */
    size_t workspace_bytes;
    int   *overflow;        /* [B] device, out, may be NULL: 1 = some local box held more than FRP_CORRIDOR_LARGE_LIST points */
} frp_nmpc_corridor_large;

/* min(B, FRP_CORRIDOR_LARGE_GROUPS) lists of FRP_CORRIDOR_LARGE_LIST 32-bit entries: 256 KB per list, 128 MB from B = 512 on;
 * 0 for B < 1.  Host arithmetic only. */
size_t frp_nmpc_corridor_large_workspace_bytes(int B);

/* The chain of frp_nmpc_corridor_batch_view for a shared cloud of 0 <= p->P <= FRP_CORRIDOR_LARGE_MAX_POINTS points:
 *   1. the one-wavefront kernel and 2. the grid workgroup kernel, as in every other entry (with or without the cut);
 *   3. for the planners the grid kernel left flagged (more than 8192 points in a local box): the large fallback -- min(B,
 *      FRP_CORRIDOR_LARGE_GROUPS) workgroups walk the planners b = wg, wg + groups, ..., skip the unflagged ones, and write
 *      overflow[b] for every b.  No queue, no flag polled across workgroups, no grid barrier.
 * The grid is REQUIRED (p->grid_start, grid_points, grid_index, a positive grid_cell, grid_dims >= 1) and so is a non-zero
 * p->bbox: without them there is no large route.  p->cloud_count may be a device [1] count -- the caller then asserts, as for
 * frp_nmpc_corridor_batch_view, that the grid was built for exactly cloud[0 .. cloud_count[0]) -- or NULL: p->P points are live.
 * cut may be NULL (no visibility cut).  p->P is the capacity of cloud / grid_points / grid_index; it sizes nothing in LDS.
 * FRP_ERR_ARG before anything is launched: everything frp_nmpc_corridor_batch_cut refuses other than P <= FRP_CORRIDOR_MAX_POINTS,
 * P above FRP_CORRIDOR_LARGE_MAX_POINTS, cloud_per_planner != 0, a missing grid, an all-zero bbox, a null w, a null workspace or
 * one shorter than frp_nmpc_corridor_large_workspace_bytes(p->B); then FRP_ERR_NO_DEVICE without a device.  Asynchronous on `stream`, allocates nothing, reads nothing
 * back, can be captured into a hipGraph. */
int frp_nmpc_corridor_batch_large(const frp_nmpc_corridor *p, const frp_nmpc_corridor_cut *cut,
                                  const frp_nmpc_corridor_large *w, void *stream);

/* frp_nmpc_occmap_shared_view_update with 1 <= view->cap <= FRP_CORRIDOR_LARGE_MAX_POINTS: the same struct, the same five
 * launches, the same overflow rule (count = min(total, cap)), the same x, y, z order, the same refusals otherwise.  (Every index
 * of those kernels is a 32-bit int and every byte offset a size_t: nothing in them depended on the old limit.) */
struct frp_nmpc_occmap_shared_view; /* frp_nmpc_occmap_view.h (named by its tag: this header also compiles when that one is the includer) */
int frp_nmpc_occmap_shared_view_update_large(const frp_nmpc_occmap *map, const struct frp_nmpc_occmap_shared_view *view,
                                             void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FRP_NMPC_CORRIDOR_LARGE_H */
