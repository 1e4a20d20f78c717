/* frp_nmpc.h section (8), frp_nmpc_occmap_distance.h: the truncated distance field of the device occupancy map and the clearance
 * queries on it.  frp_nmpc.h includes it, and including it alone works too (it pulls in frp_nmpc.h for frp_nmpc_occmap and carries its
 * own extern "C").  A header of its own for the reason frp_nmpc_occmap_fuse.h gives: tests/test_occmap_cpu.py pins the set of
 * frp_nmpc_occmap_* names that frp_nmpc.h itself declares.  These prototypes are covered by tests/test_occmap_distance_cpu.py and by
 * the load-time check of solver.DISTANCE_EXPORTS.  Same section, same ABI version, no existing struct changed.
 *
 * NO REFERENCE COUNTERPART: the reference's map (occ_grid/src/occ_map.cpp) answers yes / no questions only and keeps no distance
 * information.  tests/occmap_distance_oracle.py is the executable statement, written as brute force.  Tracking error and the rest of a
 * flight record are section (14) of frp_nmpc.h (frp_nmpc_flight_*), whose summary takes this header's min_clear and hits.
 *
 * The field.  For a map with grid (gx, gy, gz), a radius R in voxels, 1 <= R <= FRP_OCCMAP_DIST_MAX_R, and a flag `border`:
 *     D2[x][y][z]    = min over "occupied" voxels u of |(x, y, z) - u|^2                       (integers)
 *     field[x][y][z] = D2 <= R * R ? D2 : FRP_OCCMAP_DIST_FAR                                   uint16 at x * gy * gz + y * gz + z
 * "Occupied": the voxel's bit in the map's bit plane is set (the plane lives in the map's workspace: ceil(gz / 32) words per (x, y)
 * column, bit z % 32 of word z / 32); log_odds and occ are NOT read.  Bits at z >= gz of a column's last word are never taken for
 * voxels.  With border != 0 every voxel OUTSIDE the map counts as occupied as well -- the reading checkPosSurround takes, where a probe
 * outside the map is a collision --, so that D2 of a voxel of the map is also bounded by min(x + 1, gx - x)^2 and likewise in y and z.
 * An occupied voxel has field = 0; an empty map with border = 0 is FRP_OCCMAP_DIST_FAR everywhere.  R * R <= 4096 leaves uint16 room.
 * The arithmetic is exact: the field equals the definition to the bit.
 *
 * Clearance.  The voxel of a position is the reference's posToIndex (occ_map.cpp:71-75): floor((pos - origin) * (1 / resolution)) per
 * axis, tested as a double against 0 and grid - 1 (isInMap, :66-69) as frp_nmpc_occmap_query does.  Inside the map
 *     clear = resolution * sqrt((double)D2)            one rounding for the square root, one for the product; +inf where the field is FAR
 * and outside the map, or with a coordinate that is NaN or infinite, clear = 0.0 (d2 = -1): the vehicle has left the known world, which
 * the reference treats as a collision.
 * WHAT THE NUMBER MEANS: a distance between voxel CENTRES -- from the centre of the voxel that holds the position to the centre of the
 * nearest occupied voxel.  By the triangle inequality (each of the two points is within sqrt(3) / 2 voxels of its centre) the distance
 * from the position itself to any point of any occupied voxel is at least resolution * (sqrt(D2) - sqrt(3)).  The body's radius is the
 * caller's to subtract.  clear == 0.0 exactly: inside an occupied voxel, outside the map, or not finite.
 *
 * Like every call of this section: every array is device memory, the call is asynchronous on `stream` and capturable, nothing is
 * allocated, nothing is read back to the host, no kernel waits on another workgroup; FRP_ERR_ARG before any launch, FRP_ERR_NO_DEVICE
 * without a device. */
#ifndef FRP_NMPC_OCCMAP_DISTANCE_H
#define FRP_NMPC_OCCMAP_DISTANCE_H

#include <stddef.h>
#include <stdint.h>

#include "frp_nmpc.h" /* (a no-op when frp_nmpc.h is the includer) */

#ifdef __cplusplus
extern "C" {
#endif

#define FRP_OCCMAP_DIST_FAR 65535 /* field value: no occupied voxel within R */
#define FRP_OCCMAP_DIST_MAX_R 64  /* the largest radius, in voxels */

/* Bytes of scratch frp_nmpc_occmap_distance_update needs for this map and radius: an 8-bit and a 16-bit volume, the results of the
 * first two passes.  0 for a map description the calls refuse, or R outside [1, FRP_OCCMAP_DIST_MAX_R]. */
size_t frp_nmpc_occmap_distance_scratch_bytes(const frp_nmpc_occmap *map, int R);

/* field [gx][gy][gz] uint16 <- the definition above, from the bit plane in map_workspace (the MAP's workspace) as it is on `stream`
 * when the call runs.  Three launches, one pass per axis.  FRP_ERR_ARG: a NULL pointer, an invalid map, R outside
 * [1, FRP_OCCMAP_DIST_MAX_R], scratch_bytes below frp_nmpc_occmap_distance_scratch_bytes, map_workspace_bytes below
 * frp_nmpc_occmap_workspace_bytes.  scratch: 256-byte aligned, the caller's between calls. */
int frp_nmpc_occmap_distance_update(const frp_nmpc_occmap *map, int R, int border, uint16_t *field, void *scratch, size_t scratch_bytes,
                                    void *map_workspace, size_t map_workspace_bytes, void *stream);

/* clear[q] (and d2[q] where d2 is not NULL: the field's integer, FRP_OCCMAP_DIST_FAR included, -1 outside) of Q positions [Q][3].
 * R: the radius the field was built with (checked for its range only).  Q = 0 launches nothing. */
int frp_nmpc_occmap_clearance(const frp_nmpc_occmap *map, const uint16_t *field, int R, int Q, const double *pos, double *clear, int *d2,
                              void *stream);

/* The same for the S samples of B vehicles, accumulated: pos points at the first position of a [B][S][stride] array of doubles whose
 * first three entries per sample are the position (stride = 9 reads frp_nmpc_vehicle's trace directly; stride >= 3).  One thread per
 * vehicle takes its samples in order: min_clear[b] = min(min_clear[b], clear); hits[b] += 1 where clear == 0.0 (a NaN position is a
 * hit with clearance 0, not swallowed by the minimum); samples[b] += 1.  active [B] or NULL (everybody): where active[b] == 0 nothing
 * of vehicle b changes.  B = 0 launches nothing; S >= 1. */
int frp_nmpc_occmap_clearance_trace(const frp_nmpc_occmap *map, const uint16_t *field, int R, int B, int S, int stride, const double *pos,
                                    const int *active, double *min_clear, int *hits, int *samples, void *stream);

/* min_clear[b] <- +inf, hits[b] <- 0, samples[b] <- 0 where mask[b] != 0 (mask NULL: everywhere). */
int frp_nmpc_occmap_clearance_reset(int B, const int *mask, double *min_clear, int *hits, int *samples, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FRP_NMPC_OCCMAP_DISTANCE_H */
