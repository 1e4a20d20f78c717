/* frp_nmpc.h section (8), third part: the collision checks of the reference's safety timer on the device occupancy map.
 * frp_nmpc.h includes it, and including it alone works too (it pulls in frp_nmpc.h for frp_nmpc_occmap and carries its own
 * extern "C").  A header of its own for the reason frp_nmpc_occmap_fuse.h gives: tests/test_occmap_cpu.py pins the set of
 * frp_nmpc_occmap_* names that frp_nmpc.h itself declares.  These three prototypes are covered by tests/test_occmap_check_cpu.py
 * and by the load-time check of solver.CHECK_EXPORTS.  Same section, same ABI version, no existing struct changed.
 *
 * What is restated: OccMap::checkPosSurround (occ_grid/src/occ_map.cpp:625-643) and the two halves of its only caller,
 * NMPCManage::checkReplanCallback (plan_manage/src/nmpc_manage.cpp:285-341): the goal test with the search for another goal
 * (:289-316) and the walk along the kinodynamic path (:329-340).  The FSM transitions that follow them stay with the caller, who
 * reads goal_blocked and first_hit -- or hands both to frp_nmpc_fsm_safety (section (11), frp_nmpc_fsm.h), which restates them.  tests/occmap_check_oracle.py is the executable statement.
 *
 * checkPosSurround(pos, ratio) probes getVoxelState(pos + Vector3d(i, j, k) * resolution) for |i|, |j| <= ceil(ego_r * ratio /
 * resolution) and |k| <= ceil(ego_h * ratio / resolution) and returns true ("free") when every probe is 0: a probe outside the
 * map (-1, a NaN included) or on an occupied voxel (1) is a collision, a probe inside the map but outside the planner's local
 * box (tested inclusively, as frp_nmpc_occmap_query does) is free.  The half-extents are computed once on the host in exactly
 * that order of operations; one that is negative, not finite or above 31 is FRP_ERR_ARG.
 * The device evaluates the probe box as the product it is: per axis, the index floor(((pos[a] + (double)i * resolution) -
 * origin[a]) * (1 / resolution)) of every offset i with the reference's operations (one rounding each -- NOT floor(pos) + i, which
 * differs at voxel faces), then the surviving z indices as a mask over the words of the map's bit plane and one masked word per
 * (x, y) column.  The verdict is the reference's for every input; log_odds and occ are not read.
 *
 * Like every call of this section: asynchronous on `stream`, capturable, nothing read back to the host, FRP_ERR_ARG before any
 * launch, FRP_ERR_NO_DEVICE without a device.  workspace: the MAP's workspace (the bit plane).  Every array is device memory.
 * local_box: [.][6] of a local view, or NULL: the whole map is local. */
#ifndef FRP_NMPC_OCCMAP_CHECK_H
#define FRP_NMPC_OCCMAP_CHECK_H

#include "frp_nmpc.h" /* (a no-op when frp_nmpc.h is the includer) */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct frp_nmpc_occmap_body {
    double ego_r, ego_h; /* occ_map/ego_r, ego_h: 0.27, 0.0425 in the reference's launch file */
} frp_nmpc_occmap_body;

/* free_out[q] = 1 where checkPosSurround(pos[q], inflate_ratio) returns true, else 0, for Q positions [Q][3].  planner [Q]: the row
 * of local_box for each position, or NULL: row 0; planner without local_box is FRP_ERR_ARG.  Q = 0 launches nothing. */
int frp_nmpc_occmap_check_surround(const frp_nmpc_occmap *map, const frp_nmpc_occmap_body *body, double inflate_ratio, int Q,
                                   const double *pos, const int *planner, const int *local_box, int *free_out, void *workspace,
                                   size_t workspace_bytes, void *stream);

/* The loop of :329-340 for B planners: the samples 0, stride, 2 * stride, ... < min(kino_size[b], K) of kino_path [B][K][3]
 * (frp_nmpc_astar.kino_path / kino_size) are checked at inflate_ratio against row b of local_box; first_hit[b] = the smallest
 * colliding sample index, or -1: none, have_traj[b] == 0 (have_traj NULL: every planner has one) or a size <= 0.  Storage beyond
 * the size is not read.  K and stride >= 1. */
int frp_nmpc_occmap_check_paths(const frp_nmpc_occmap *map, const frp_nmpc_occmap_body *body, double inflate_ratio, int B, int K,
                                int stride, const double *kino_path, const int *kino_size, const int *have_traj,
                                const int *local_box, int *first_hit, void *workspace, size_t workspace_bytes, void *stream);

/* :289-316 for B planners, as written.  end_pt [B][3] is tested at inflate_check (1.2 there); goal_blocked[b] = 1 when it
 * collides.  A blocked goal walks table [n_groups * group_size][3] in order: candidate c is (end_pt.x + table[c][0],
 * end_pt.y + table[c][1], table[c][2]) -- the third entry is an ABSOLUTE z -- and one that is free at inflate_search (1.5 there)
 * replaces end_pt at once and ends its group (the reference's `break` leaves only the innermost loop); the walk goes on FROM THE
 * MOVED GOAL through every remaining group.  goal_hits[b] counts the replacements; a blocked goal without a free candidate keeps its
 * value.  have_target[b] == 0 (NULL: every planner has one): end_pt untouched, goal_blocked = goal_hits = 0.
 * The table is made on the host (the reference's r / theta / nz loops: solver.goal_search_table()), so that the device adds and
 * evaluates no cos.  group_size >= 1, n_groups >= 0 (0: no candidates, table may be NULL). */
int frp_nmpc_occmap_check_goals(const frp_nmpc_occmap *map, const frp_nmpc_occmap_body *body, double inflate_check,
                                double inflate_search, int B, double *end_pt, const int *have_target, const int *local_box,
                                int n_groups, int group_size, const double *table, int *goal_blocked, int *goal_hits,
                                void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FRP_NMPC_OCCMAP_CHECK_H */
