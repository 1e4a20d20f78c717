"""CPU restatement of the reference's occupancy map (occ_grid/src/occ_map.cpp; line numbers below are that file's), plain NumPy,
one statement of the reference per statement here.  It is what tests/test_gpu_occmap.py compares the device map against, to the
bit: every quantity is an integer, a byte, or a double that went through float32.

Where the reference converts a floored double to int without a test (NaN, beyond int: undefined behaviour in C++), this file -- like
include/frp_nmpc.h (8) -- decides on the double: such a point is outside the map (_in_map_f), and the index of a local range is
clamped to +-2^30 first (_to_int), which the max(0, .) / min(grid_size, .) of the reference then clamps like any other value.
"""
import numpy as np

ID_LIM = 2.0 ** 30


def _to_int(f):
    """int(f) for a floored double, defined for every input: NaN and anything below -2^30 -> -2^30, above 2^30 -> 2^30."""
    f = float(f)
    if not (f >= -ID_LIM):
        f = -ID_LIM
    if f > ID_LIM:
        f = ID_LIM
    return int(f)


class OccMapOracle:
    def __init__(self, origin, map_size, resolution, local_radius=(6.0, 6.0, 3.0), clamp_min_log=0.12, clamp_max_log=0.97,
                 min_occupancy_log=0.80):
        self.origin = np.array(origin, dtype=np.float64)
        self.map_size = np.array(map_size, dtype=np.float64)
        self.resolution = np.float64(resolution)
        self.sensor_range = np.array(local_radius, dtype=np.float64)                                   # :730-732
        self.clamp_min_log, self.clamp_max_log, self.min_occupancy_log = float(clamp_min_log), float(clamp_max_log), float(min_occupancy_log)  # :752-754
        self.resolution_inv = np.float64(1) / self.resolution                                          # :787
        self.grid_size = np.array([int(np.ceil(self.map_size[i] / self.resolution)) for i in range(3)])  # :788-789
        self.min_range = self.origin.copy()                                                            # :800
        self.max_range = self.origin + self.map_size                                                   # :801
        self.buffer = np.full(tuple(self.grid_size), self.clamp_min_log, dtype=np.float64)             # :831, index [x][y][z] (:104)

    # ---- index arithmetic ----
    def pos_to_index_f(self, pos):
        """posToIndex (:71-75) before the conversion to int: floor((pos - origin_) * resolution_inv_) per axis, as doubles."""
        with np.errstate(invalid="ignore", over="ignore"):
            return np.floor((np.asarray(pos, dtype=np.float64) - self.origin) * self.resolution_inv)

    def pos_to_index(self, pos):
        return [_to_int(f) for f in self.pos_to_index_f(pos)]

    def index_to_pos(self, idx):
        """indexToPos (:77-82): pos = origin_; pos(i) += (id(i) + 0.5) * resolution_."""
        pos = self.origin.copy()
        for i in range(3):
            pos[i] += (np.float64(idx[i]) + 0.5) * self.resolution
        return pos

    def _in_map_f(self, f):
        """isInMap (:66-69) on the floored doubles: 0 <= id <= grid_size - 1 on every axis (a NaN is outside)."""
        return bool(all(f[i] >= 0.0 and f[i] <= float(self.grid_size[i] - 1) for i in range(3)))

    def is_in_map(self, idx):
        return all(0 <= idx[i] <= self.grid_size[i] - 1 for i in range(3))                             # :68

    # ---- writers ----
    def reset(self):
        self.buffer[...] = self.clamp_min_log                                                          # :831

    def set_occupancy(self, pos):
        """setOccupancy (:84-93)."""
        f = self.pos_to_index_f(pos)                                                                   # :87
        if not self._in_map_f(f):                                                                      # :89-90
            return
        self.buffer[int(f[0]), int(f[1]), int(f[2])] = self.clamp_max_log                              # :92

    def insert_cloud(self, points):
        """globalCloudCallback's loop (:612-619): every pcl::PointXYZ (float32) promoted to double, then setOccupancy."""
        pts = np.asarray(points).astype(np.float32)                                                    # :605-606, pcl::PointXYZ
        for i in range(len(pts)):
            p3d = pts[i].astype(np.float64)                                                            # :617
            self.set_occupancy(p3d)                                                                    # :618

    def reset_buffer(self, min_pos, max_pos):
        """resetBuffer(min_pos, max_pos) (:15-36)."""
        min_pos = np.array(min_pos, dtype=np.float64); max_pos = np.array(max_pos, dtype=np.float64)
        for i in range(3):
            min_pos[i] = max(min_pos[i], self.min_range[i])                                            # :17-19
            max_pos[i] = min(max_pos[i], self.max_range[i])                                            # :21-23
        min_id = self.pos_to_index(min_pos)                                                            # :27
        max_id = self.pos_to_index(max_pos - np.full(3, self.resolution / 2))                          # :28
        for i in range(3):  # (guard of the device call, inactive unless rounding at the far face: the loops stay inside the buffer)
            min_id[i] = max(min_id[i], 0); max_id[i] = min(max_id[i], int(self.grid_size[i]) - 1)
        for x in range(min_id[0], max_id[0] + 1):                                                      # :30, x <= max_id
            for y in range(min_id[1], max_id[1] + 1):                                                  # :31
                for z in range(min_id[2], max_id[2] + 1):                                              # :32
                    self.buffer[x, y, z] = self.clamp_min_log                                          # :34

    # ---- readers ----
    def occ(self):
        """The byte view: occupancy_buffer_ > min_occupancy_log_ (:105)."""
        return (self.buffer > self.min_occupancy_log).astype(np.uint8)

    def local_box(self, centre):
        """min_id / max_id of isInLocalMap (:47-55) with local_range_min_ / max_ = centre -/+ sensor_range_ (:273-274, :580-581).
        centre None: the whole map."""
        if centre is None:
            return [0, 0, 0] + [int(g) for g in self.grid_size]
        centre = np.asarray(centre, dtype=np.float64)
        local_range_min = centre - self.sensor_range                                                   # :580
        local_range_max = centre + self.sensor_range                                                   # :581
        min_id = self.pos_to_index(local_range_min)                                                    # :48
        max_id = self.pos_to_index(local_range_max)                                                    # :49
        for i in range(3):
            min_id[i] = max(0, min_id[i])                                                              # :50-52
            max_id[i] = min(int(self.grid_size[i]), max_id[i])                                         # :53-55
        return min_id + max_id

    def is_in_local_map(self, idx, box):
        """:56 -- INCLUSIVE on both sides."""
        return all(idx[i] - box[i] >= 0 and box[3 + i] - idx[i] >= 0 for i in range(3))

    def get_voxel_state(self, pos, box=None):
        """getVoxelState(pos) (:95-106); box = local_box(centre), None: everything is local."""
        f = self.pos_to_index_f(pos)                                                                   # :98
        if not self._in_map_f(f):                                                                      # :99-100
            return -1
        idx = [int(v) for v in f]
        if box is not None and not self.is_in_local_map(idx, box):                                     # :101-102
            return 0
        return 1 if self.buffer[idx[0], idx[1], idx[2]] > self.min_occupancy_log else 0                # :105

    def local_cloud_loops(self, centre):
        """localOccVisCallback (:181-206) (centre None: globalOccVisCallback, :153-167) as written: three nested loops with EXCLUSIVE
        upper bounds, indexToPos, pcl::PointXYZ (float32), push_back.  Returns the points widened to double, [n, 3]."""
        box = self.local_box(centre)                                                                   # :183-191
        pts = []
        for x in range(box[0], box[3]):                                                                # :192, x < max_id
            for y in range(box[1], box[4]):                                                            # :193
                for z in range(box[2], box[5]):                                                        # :194
                    if self.buffer[x, y, z] > self.min_occupancy_log:                                  # :196
                        pos = self.index_to_pos((x, y, z))                                             # :200
                        pc = pos.astype(np.float32)                                                    # :203
                        pts.append(pc.astype(np.float64))                                              # :204 (read back by cloudCallback, nmpc_solver.cpp:990-995)
        return np.array(pts, dtype=np.float64).reshape(-1, 3)

    def local_cloud(self, centre):
        """The same cloud without Python loops (for thousands of planners): the occupied voxels of the block
        [min_id, max_id) in C order = x, y, z loop order; the same three operations per coordinate.  tests/test_occmap_cpu.py
        holds it against local_cloud_loops."""
        box = self.local_box(centre)
        lo = [min(box[i], int(self.grid_size[i])) for i in range(3)]
        hi = [max(box[3 + i], lo[i]) for i in range(3)]
        sub = self.buffer[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] > self.min_occupancy_log
        idx = np.argwhere(sub) + np.array(lo)
        pos = self.origin[None, :] + (idx.astype(np.float64) + 0.5) * self.resolution
        return pos.astype(np.float32).astype(np.float64).reshape(-1, 3)


def from_world(world, **kw):
    """The oracle map of a workloads.astar_world dict: its occupied voxels at clamp_max_log, the others at clamp_min_log."""
    m = OccMapOracle(world["origin"], world["map_size"], world["resolution"], **kw)
    assert tuple(m.grid_size) == world["occ"].shape
    m.buffer[world["occ"] != 0] = m.clamp_max_log
    return m
