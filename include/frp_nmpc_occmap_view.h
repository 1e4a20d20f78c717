/* frp_nmpc.h section (8), sixth part: the SHARED VIEW of the occupancy map rebuilt on the device -- the whole-map obstacle cloud
 * and its uniform grid in caller-owned buffers of fixed capacity, and the corridor entry point that takes them with the grid ON.
 * frp_nmpc.h includes it, and including it alone works too (it pulls in frp_nmpc.h for frp_nmpc_occmap, frp_nmpc_corridor and
 * frp_nmpc_corridor_cut, and carries its own extern "C").  A header of its own for the reason frp_nmpc_occmap_fuse.h gives:
 * tests/test_occmap_cpu.py pins the frp_nmpc_occmap_* names that frp_nmpc.h itself declares.  The prototypes are covered by
 * tests/test_occmap_shared_view_cpu.py and by the load-time check of solver.VIEW_EXPORTS.  Same section, same ABI version, no
 * existing struct changed.
 *
 * WHY: the shared-cloud route (frp_nmpc_corridor_cut) needs the whole-map cloud and a grid over it after every map change.  Made
 * with frp_nmpc_occmap_local_view(centre = NULL) + frp_nmpc_cloud_grid_build that is one workgroup walking every column, a count
 * read back to the host, and a grid built for a HOST point count.  With depth fusion the map changes every tick.  Here the same
 * cloud and the same grid are rebuilt by one asynchronous call that reads the count from device memory throughout.
 *
 * The cloud: every occupied voxel's centre origin + (id + 0.5) * resolution rounded to float and widened, in x, y, z loop order --
 * bit for bit the first `count` points of frp_nmpc_occmap_local_view(centre = NULL, P = cap) (the order matters: the corridor breaks
 * ties by cloud index).  count[0] = min(total[0], cap), total[0] = the occupied voxels of the map.  On overflow (total > cap) the
 * first cap points in loop order are kept; count stays NON-NEGATIVE (the negated count of frp_nmpc_occmap_view would read as an
 * empty cloud in the corridor) and the loss is read from total[0] > count[0].  Nothing beyond cloud[count] is written.
 * The grid: frp_nmpc_cloud_grid_build's arithmetic over cloud[0 .. count), origin = the map's origin, dims[k] =
 * ceil(map_size[k] / cell) (frp_nmpc_occmap_shared_view_dims).  grid_start is rebuilt completely by every update, for every count, 0
 * included: a point of an earlier, larger update that still lies in cloud or grid_points beyond the count is in no cell.
 *
 * FIVE launches per update, whatever the map holds, each ordered behind the one before by the stream alone -- NO kernel waits on
 * another workgroup (no flags, no look-back, no grid barrier):
 *   1. count   W <= FRP_OCCMAP_VIEW_MAX_GROUPS workgroups, each over a contiguous run of (x, y) columns: the run's population count ->
 *              group_sums[w]; the same launch zeroes grid_start and cursor
 *   2. scan    one workgroup: exclusive prefix sum of group_sums in place, total[0], count[0]
 *   3. emit    the W workgroups again: each writes its run's centres from cloud[group_sums[w]] on (the tile scan of
 *              frp_nmpc_occmap_local_view's kernel), and counts every point it stores into its grid cell
 *   4. scan    one workgroup: inclusive prefix sum of grid_start (frp_nmpc_cloud_grid_build's)
 *   5. scatter cloud[0 .. count[0]) into grid_points / grid_index (order inside a cell is free: ties go by cloud index)
 * Like every call of this section: asynchronous on `stream`, allocates nothing, reads nothing back, capturable. */
#ifndef FRP_NMPC_OCCMAP_VIEW_H
#define FRP_NMPC_OCCMAP_VIEW_H

#include "frp_nmpc.h" /* (a no-op when frp_nmpc.h is the includer) */

#ifdef __cplusplus
extern "C" {
#endif

#define FRP_OCCMAP_VIEW_MAX_GROUPS 1024 /* workgroups of the count and emit launches                                        */
#define FRP_OCCMAP_VIEW_LAUNCHES 5      /* kernel launches per frp_nmpc_occmap_shared_view_update, independent of the map    */

typedef struct frp_nmpc_occmap_shared_view {
    int cap;             /* points the buffers hold, 1 <= cap <= FRP_CORRIDOR_MAX_POINTS: frp_nmpc_corridor.P of the consumer     */
    double cell;         /* grid cell edge in metres, finite and > 0                                                              */
    int dims[3];         /* frp_nmpc_occmap_shared_view_dims(map, cell, .); anything else is FRP_ERR_ARG                          */
    /* all DEVICE, all caller-owned, none may alias another or the map's arrays                                                   */
    double *cloud;       /* [cap][3]                out: frp_nmpc_corridor.cloud                                                  */
    int *count;          /* [1]                     out: frp_nmpc_corridor.cloud_count                                            */
    int *total;          /* [1]                     out: occupied voxels of the map; > count[0]: the cloud overflowed             */
    double *grid_points; /* [cap][3]                out: frp_nmpc_corridor.grid_points                                            */
    int *grid_index;     /* [cap]                   out: frp_nmpc_corridor.grid_index                                             */
    int *grid_start;     /* [cells + 1]             out: frp_nmpc_corridor.grid_start, cells = dims[0] * dims[1] * dims[2]         */
    int *cursor;         /* [cells]                 scratch                                                                       */
    int *group_sums;     /* [FRP_OCCMAP_VIEW_MAX_GROUPS] scratch                                                                  */
} frp_nmpc_occmap_shared_view;

/* dims[k] = ceil(map_size[k] / cell) and FRP_OK; FRP_ERR_ARG (dims untouched) for a map the other calls refuse, a null dims, a cell
 * that is not finite and positive, or more than FRP_CORRIDOR_MAX_CELLS cells.  Host arithmetic only. */
int frp_nmpc_occmap_shared_view_dims(const frp_nmpc_occmap *map, double cell, int dims[3]);

/* Rebuild cloud, count, total and the grid from the map's bit plane.  workspace: the MAP's workspace, the only thing read.
 * FRP_ERR_ARG before a device is touched: a map the other calls refuse, a short or null workspace, a null view or a null buffer
 * among the eight, cap < 1 or above FRP_CORRIDOR_MAX_POINTS, a cell that is not finite and positive, dims other than
 * frp_nmpc_occmap_shared_view_dims gives (more than FRP_CORRIDOR_MAX_CELLS cells included).  FRP_ERR_NO_DEVICE without a device. */
int frp_nmpc_occmap_shared_view_update(const frp_nmpc_occmap *map, const frp_nmpc_occmap_shared_view *view, void *workspace,
                                       size_t workspace_bytes, void *stream);

/* frp_nmpc_corridor_batch_cut's chain of launches (one-wavefront kernel, grid kernel, plain-cloud kernel) for a cloud whose live
 * count is on the DEVICE and whose grid was built for exactly that count -- what frp_nmpc_occmap_shared_view_update leaves:
 *   p->cloud_count ([1], device) is REQUIRED; the caller asserts that p->grid_* describe cloud[0 .. cloud_count[0]);
 *   the grid is used whenever p->grid_start is set and p->bbox is not all zero (the other entry points turn it off when a count is
 *   given, and keep doing so);  p->P is the CAPACITY of cloud / grid_points / grid_index: it sizes the LDS masks, bounds the rounds
 *   and is the one-wavefront kernel's first density guess, for which any value gives the same result.
 * cut may be NULL (no visibility cut).  FRP_ERR_ARG before anything is launched: everything frp_nmpc_corridor_batch_cut refuses, a
 * null cloud_count, cloud_per_planner != 0.  Asynchronous on `stream`, allocates nothing, capturable. */
int frp_nmpc_corridor_batch_view(const frp_nmpc_corridor *p, const frp_nmpc_corridor_cut *cut, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FRP_NMPC_OCCMAP_VIEW_H */
