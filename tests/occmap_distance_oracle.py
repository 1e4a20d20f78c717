"""Executable statement of the occupancy map's truncated distance field and its clearance queries (include/frp_nmpc_occmap_distance.h),
written as BRUTE FORCE, not separably: the minimum over all occupied voxels of the integer squared offset, the border terms, the cut
at R * R, the clearance rule for points with the reference's index arithmetic as tests/occmap_oracle.py states it, and the trace
accumulation.  There is no reference counterpart: the reference's map (occ_grid/src/occ_map.cpp) keeps no distance.

    D2[x][y][z]    = min over occupied voxels u of |(x, y, z) - u|^2                       integers
    field[x][y][z] = D2 if D2 <= R * R else FAR (65535)                                    uint16

"Occupied": the voxel's bit in the map's bit plane (ceil(gz / 32) words per (x, y) column, bit z % 32 of word z // 32); bits at
z >= gz of the last word are not voxels.  border: every voxel OUTSIDE the map counts as occupied too; the nearest of those to a voxel of
the map lies straight along an axis, so D2 is also bounded by min(x + 1, gx - x)^2 and likewise in y and z
(tests/test_occmap_distance_cpu.py holds that against a map padded by a shell of occupied voxels).
"""
import numpy as np

FAR = 65535     # FRP_OCCMAP_DIST_FAR
MAX_R = 64      # FRP_OCCMAP_DIST_MAX_R
_NONE = np.int64(1) << 40


def pack_plane(occ):
    """The bit plane of a boolean [gx, gy, gz] volume: uint32 [gx, gy, ceil(gz / 32)], bit z % 32 of word z // 32."""
    occ = np.asarray(occ, dtype=bool)
    gx, gy, gz = occ.shape
    wz = (gz + 31) // 32
    padded = np.zeros((gx, gy, wz * 32), dtype=np.uint64)
    padded[:, :, :gz] = occ
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    return (padded.reshape(gx, gy, wz, 32) * weights).sum(axis=3).astype(np.uint32)


def unpack_plane(plane, gz):
    """The voxels of a bit plane [gx, gy, wz]: boolean [gx, gy, gz].  Bits at z >= gz are dropped, whatever they hold."""
    plane = np.asarray(plane, dtype=np.uint32)
    gx, gy, wz = plane.shape
    assert wz == (gz + 31) // 32
    bits = (plane[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(gx, gy, wz * 32)[:, :, :gz].astype(bool)


def squared_distance(occ, border):
    """D2 as int64 [gx, gy, gz] (a value >= 2^40 where nothing is occupied anywhere): every voxel against every occupied voxel."""
    occ = np.asarray(occ, dtype=bool)
    gx, gy, gz = occ.shape
    vox = np.stack(np.meshgrid(np.arange(gx), np.arange(gy), np.arange(gz), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64)
    pts = np.argwhere(occ).astype(np.int64)
    d2 = np.full(len(vox), _NONE, dtype=np.int64)
    if len(pts):
        step = max(1, (1 << 22) // len(pts))
        for i in range(0, len(vox), step):
            off = vox[i:i + step, None, :] - pts[None, :, :]
            d2[i:i + step] = (off * off).sum(axis=2).min(axis=1)
    if border:
        for a, g in enumerate((gx, gy, gz)):
            edge = np.minimum(vox[:, a] + 1, g - vox[:, a])
            d2 = np.minimum(d2, edge * edge)
    return d2.reshape(gx, gy, gz)


def field(occ, R, border):
    """The field of a boolean volume: uint16 [gx, gy, gz]."""
    assert 1 <= R <= MAX_R
    d2 = squared_distance(occ, border)
    return np.where(d2 <= R * R, d2, FAR).astype(np.uint16)


def field_of_plane(plane, gz, R, border):
    """The field of a bit plane, as the device reads it."""
    return field(unpack_plane(plane, gz), R, border)


def voxel_of(m, pos):
    """The voxel of a position for the map geometry m (a tests/occmap_oracle.py OccMapOracle): posToIndex before the conversion to int,
    isInMap on the doubles -- None outside the map, for a NaN and for an infinity."""
    f = m.pos_to_index_f(pos)
    if not m._in_map_f(f):
        return None
    return tuple(int(v) for v in f)


def clearance(m, fld, pos):
    """(clear, d2) of one position: resolution * sqrt(d2), one rounding each; +inf where the field is FAR; (0.0, -1) outside."""
    v = voxel_of(m, pos)
    if v is None:
        return 0.0, -1
    d2 = int(fld[v])
    if d2 == FAR:
        return float("inf"), d2
    return float(np.float64(m.resolution) * np.sqrt(np.float64(d2))), d2


def clearances(m, fld, pos):
    """(clear float64 [Q], d2 int32 [Q]) of positions [Q, 3]."""
    out = [clearance(m, fld, p) for p in np.asarray(pos, dtype=np.float64).reshape(-1, 3)]
    return np.array([c for c, _ in out], dtype=np.float64), np.array([d for _, d in out], dtype=np.int32)


def trace_accumulate(m, fld, trace, min_clear, hits, samples, active=None):
    """frp_nmpc_occmap_clearance_trace: the S samples of trace [B, S, stride >= 3] in order into copies of min_clear / hits / samples."""
    trace = np.asarray(trace, dtype=np.float64)
    min_clear, hits, samples = np.array(min_clear, dtype=np.float64), np.array(hits, dtype=np.int32), np.array(samples, dtype=np.int32)
    for b in range(trace.shape[0]):
        if active is not None and active[b] == 0:
            continue
        for s in range(trace.shape[1]):
            c, _ = clearance(m, fld, trace[b, s, 0:3])
            if c < min_clear[b]:
                min_clear[b] = c
            if c == 0.0:
                hits[b] += 1
            samples[b] += 1
    return min_clear, hits, samples
