"""CPU restatement of the reference's depth-image fusion (occ_grid/src/occ_map.cpp:314-563 -- projectDepthImage, raycastProcess,
setCacheOccupancy -- and RayCaster::setInput / step, raycast.cpp:6-29, 263-366; line numbers below are those files'), built on
tests/occmap_oracle.py.  Plain Python floats (IEEE doubles), one statement of the reference per statement here, serial.  It is what
tests/test_gpu_occmap_fusion.py compares frp_nmpc_occmap_fuse_depth against, to the bit.

Structurally unpinned, like SURVEY rows f-2 ... f-4: the reference's vector statements (T_wc.block<3,3>(0,0) * p + t, .inverse(),
.norm(), (p - t) / length * max + t, p / resolution) are Eigen expressions whose evaluation order is decided by Eigen's templates,
and Eigen cannot be compiled next to this repository.  The operation order is therefore WRITTEN DOWN here (each place says how) and
the device code follows this file, not a compiled reference binary.

Decisions where the reference is undefined or does not end:
  * a floored double is converted to int through occmap_oracle._to_int (NaN / beyond +-2^30 are clamped), as in section (8);
  * RayCaster::step ends only ON the end cell; rounding in tMax can make it step past it and never return.  Every traversal here
    takes at most step_bound() = 3 * (ceil(max_ray_length / resolution) + 2) steps -- more than any ray that does reach its end;
  * cells whose voxel lies outside the ray box (ray_box(): the camera +- max_ray_length, two voxels of slack, clamped to the map)
    are treated like cells outside the map.  No ray that ends reaches one; self.box_skips counts them and the tests check it is 0.
"""
import math

import numpy as np

from tests.occmap_oracle import OccMapOracle, _to_int

INVALID_IDX = -1                                                                                      # occ_map.h:22
# plan_manage/launch/advanced_param.xml:69-92
FUSE_DEFAULTS = dict(depth_scale=1000.0, depth_filter_mindist=0.1, depth_filter_tolerance=0.2, depth_filter_margin=1, skip_pixel=2,
                     prob_hit_log=1.2, prob_miss_log=-0.5, min_ray_length=0.1, max_ray_length=6.0)
LAUNCH_CLAMPS = dict(clamp_min_log=-1.0, clamp_max_log=2.0, min_occupancy_log=1.70)                    # :88-90 of the same file
INF = float("inf")


def _div(a, b):
    """IEEE a / b for Python floats (which raise on a zero divisor)."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return float("nan")
    return math.copysign(INF, a) * math.copysign(1.0, b)


def _floor(v):
    """std::floor as a double (math.floor refuses an infinity or a NaN)."""
    return float(math.floor(v)) if math.isfinite(v) else v


def _floor_int(v):
    """(int)std::floor(v), defined for every input."""
    return _to_int(_floor(v))


def signum(x):                                                                                        # raycast.cpp:6-9
    return 0 if x == 0 else (-1 if x < 0 else 1)


def mod(value, modulus):                                                                              # raycast.cpp:11-14
    return math.fmod(math.fmod(value, modulus) + modulus, modulus) if math.isfinite(value) else float("nan")


def intbound(s, ds):                                                                                  # raycast.cpp:16-29
    if ds < 0:
        return intbound(-s, -ds)
    s = mod(s, 1.0)
    return _div(1.0 - s, ds)


def inverse3(R):
    """last_T_wc.block<3,3>(0,0).inverse() (:382), once per frame, as adjugate / determinant in THIS order (the device call does the
    same on the host): cofactors a*b - c*d, det = (R00*C00 + R01*C01) + R02*C02, inv[i][j] = C[j][i] / det.  None: singular."""
    R = [[float(R[i][j]) for j in range(3)] for i in range(3)]
    C = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            C[i][j] = R[i1][j1] * R[i2][j2] - R[i1][j2] * R[i2][j1]
    det = (R[0][0] * C[0][0] + R[0][1] * C[0][1]) + R[0][2] * C[0][2]
    if not math.isfinite(det) or det == 0.0:
        return None
    return [[C[j][i] / det for j in range(3)] for i in range(3)]


class RayCaster:
    """raycast.cpp:263-366."""

    def set_input(self, start, end):                                                                  # :263-310
        self.x, self.y, self.z = (_floor_int(start[k]) for k in range(3))                            # :271-273
        self.end = tuple(_floor_int(end[k]) for k in range(3))                                        # :274-276
        dx, dy, dz = float(self.end[0] - self.x), float(self.end[1] - self.y), float(self.end[2] - self.z)   # :281-283
        self.step_x, self.step_y, self.step_z = signum(int(dx)), signum(int(dy)), signum(int(dz))     # :286-288
        self.tmax_x, self.tmax_y, self.tmax_z = intbound(start[0], dx), intbound(start[1], dy), intbound(start[2], dz)   # :292-294
        self.tdelta_x, self.tdelta_y, self.tdelta_z = _div(float(self.step_x), dx), _div(float(self.step_y), dy), _div(float(self.step_z), dz)   # :297-299
        return not (self.step_x == 0 and self.step_y == 0 and self.step_z == 0)                       # :306-309

    def step(self):                                                                                   # :312-366: (ray_pt, went on)
        ray_pt = (self.x, self.y, self.z)                                                             # :315
        if ray_pt == self.end:                                                                        # :321-324
            return ray_pt, False
        if self.tmax_x < self.tmax_y:                                                                 # :336
            if self.tmax_x < self.tmax_z:                                                             # :338
                self.x += self.step_x; self.tmax_x += self.tdelta_x                                   # :341-343
            else:
                self.z += self.step_z; self.tmax_z += self.tdelta_z                                   # :347-348
        else:
            if self.tmax_y < self.tmax_z:                                                             # :353
                self.y += self.step_y; self.tmax_y += self.tdelta_y                                   # :355-356
            else:
                self.z += self.step_z; self.tmax_z += self.tdelta_z                                   # :360-361
        return ray_pt, True


class FusionOracle(OccMapOracle):
    def __init__(self, origin, map_size, resolution, **kw):
        f = dict(FUSE_DEFAULTS)
        for k in list(kw):
            if k in f:
                f[k] = kw.pop(k)
        super().__init__(origin, map_size, resolution, **kw)
        self.depth_scale, self.depth_filter_mindist, self.depth_filter_tolerance = float(f["depth_scale"]), float(f["depth_filter_mindist"]), float(f["depth_filter_tolerance"])
        self.depth_filter_margin, self.skip_pixel = int(f["depth_filter_margin"]), int(f["skip_pixel"])
        self.prob_hit_log, self.prob_miss_log = float(f["prob_hit_log"]), float(f["prob_miss_log"])
        self.min_ray_length, self.max_ray_length = float(f["min_ray_length"]), float(f["max_ray_length"])
        self._o = [float(v) for v in self.origin]
        self._res, self._res_inv = float(self.resolution), float(self.resolution_inv)
        self._g = [int(v) for v in self.grid_size]
        self.has_first_depth = False                                                                  # :785
        self.last = None
        self.box_skips = 0
        self._box = None
        self.stats = {}
        self.last_counts = {}

    # ---- projectDepthImage (:314-439) ----
    def project(self, depth_u16, K, T_wc, last=None):
        """The projected points of one frame, in scan order: a list of (x, y, z).  last = (last_depth, last_T_wc): the shift filter
        of :364-419; None: the unfiltered loops of :327-355."""
        d = np.asarray(depth_u16)
        assert d.dtype == np.uint16 and d.ndim == 2
        rows, cols = d.shape                                                                          # :318-319
        K = [[float(v) for v in r] for r in np.asarray(K, dtype=np.float64).reshape(3, 3)]
        T = [[float(v) for v in r] for r in np.asarray(T_wc, dtype=np.float64).reshape(4, 4)]
        if last is not None:
            ld = np.asarray(last[0]); assert ld.dtype == np.uint16 and ld.shape == d.shape
            LT = [[float(v) for v in r] for r in np.asarray(last[1], dtype=np.float64).reshape(4, 4)]
            Rinv = inverse3([r[:3] for r in LT])
            assert Rinv is not None, "singular last_T_wc"
        pts = []
        m, s = self.depth_filter_margin, self.skip_pixel
        for v in range(m, rows - m, s):                                                               # :327 / :366
            for u in range(m, cols - m, s):                                                           # :329 / :368
                depth = int(d[v, u]) / self.depth_scale                                               # :331 / :370 (never NaN or inf: :332, :371)
                if depth < self.depth_filter_mindist:                                                 # :334 / :374
                    continue
                x = _div((u - K[0][2]) * depth, K[0][0])                                               # :337 / :376
                y = _div((v - K[1][2]) * depth, K[1][1])                                               # :338 / :377
                z = depth                                                                             # :339 / :378
                # :340 / :381, written order: ((R[i][0] * x + R[i][1] * y) + R[i][2] * z) + t[i]
                p = tuple(((T[i][0] * x + T[i][1] * y) + T[i][2] * z) + T[i][3] for i in range(3))
                if last is None:
                    pts.append(p)                                                                     # :341
                    continue
                # :382, written order: q = p - last_t per component, then ((Rinv[i][0] * q0 + Rinv[i][1] * q1) + Rinv[i][2] * q2)
                q = [p[i] - LT[i][3] for i in range(3)]
                r = [(Rinv[i][0] * q[0] + Rinv[i][1] * q[1]) + Rinv[i][2] * q[2] for i in range(3)]
                uu = _div(r[0] * K[0][0], r[2]) + K[0][2]                                             # :383
                vv = _div(r[1] * K[1][1], r[2]) + K[1][2]                                             # :384
                if uu >= 0 and uu < cols and vv >= 0 and vv < rows:                                   # :385
                    drift_dis = abs(int(ld[int(vv), int(uu)]) / self.depth_scale - r[2])              # :387
                    if drift_dis < self.depth_filter_tolerance:                                       # :389
                        pts.append(p)                                                                 # :391
                else:
                    pts.append(p)                                                                     # :407 "new point"
        return pts

    # ---- setCacheOccupancy (:535-563) ----
    def _index(self, pos):
        """posToIndex + isInMap + the ray box: the voxel (x, y, z) or None."""
        f = [_floor((pos[k] - self._o[k]) * self._res_inv) for k in range(3)]                          # :71-75
        for k in range(3):
            if not (f[k] >= 0.0 and f[k] <= float(self._g[k] - 1)):                                    # :545, :66-69
                return None
        id_ = (int(f[0]), int(f[1]), int(f[2]))
        if self._box is not None and not all(self._box[k] <= id_[k] < self._box[3 + k] for k in range(3)):
            self.box_skips += 1
            return None
        return id_

    def _set_cache_occupancy(self, pos, occ):
        id_ = self._index(pos)                                                                        # :542-548
        if id_ is None:
            return INVALID_IDX
        self.cache_all[id_] = self.cache_all.get(id_, 0) + 1                                          # :552 (the dict's insertion order is cache_voxel_, :554-557)
        if occ == 1:
            self.cache_hit[id_] = self.cache_hit.get(id_, 0) + 1                                      # :559-560
        return id_

    def step_bound(self):
        return 3 * (int(math.ceil(self.max_ray_length / self._res)) + 2)

    def ray_box(self, t_wc):
        """[lo(3), hi(3)) in voxels: posToIndex(t_wc -/+ max_ray_length) -/+ 2, clamped to the map.  Every in-map voxel a ray of at
        most max_ray_length can touch is inside; the device sizes its per-voxel arrays by it."""
        lo, hi = [], []
        for k in range(3):
            a = _to_int(_floor((t_wc[k] - self.max_ray_length - self._o[k]) * self._res_inv)) - 2
            e = _to_int(_floor((t_wc[k] + self.max_ray_length - self._o[k]) * self._res_inv)) + 3
            a = min(max(a, 0), self._g[k]); e = max(min(e, self._g[k]), a)
            lo.append(a); hi.append(e)
        return lo + hi

    def _batch_update(self):
        """:505-532."""
        for id_, all_ in self.cache_all.items():                                                      # :506-510
            hit = self.cache_hit.get(id_, 0)
            log_odds_update = self.prob_hit_log if hit >= all_ - hit else self.prob_miss_log           # :512-513
            cur = float(self.buffer[id_])
            if (log_odds_update >= 0 and cur >= self.clamp_max_log) or (log_odds_update <= 0 and cur <= self.clamp_min_log):   # :516-518
                continue
            self.buffer[id_] = min(max(cur + log_odds_update, self.clamp_min_log), self.clamp_max_log)   # :530-531
        self.last_counts = {id_: (all_, self.cache_hit.get(id_, 0)) for id_, all_ in self.cache_all.items()}   # (for the tests: {voxel: (all, hit)} of this frame)
        self.cache_all, self.cache_hit = {}, {}                                                       # :514

    def _ends(self, points, t_wc):
        """:453-478 for every point: the rays that are cast, [(sequence number, ray start)], after the end-voxel bookkeeping."""
        t = [float(v) for v in t_wc]
        self._box = self.ray_box(t)
        self.cache_all, self.cache_hit = {}, {}
        rayend = set()
        rays = []
        for i, p in enumerate(points):                                                                # :453
            pt_w = [float(v) for v in p]                                                              # :456
            d = [pt_w[k] - t[k] for k in range(3)]
            s2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            length = math.sqrt(s2) if s2 >= 0 else float("nan")                                        # :457, written order
            if length < self.min_ray_length:                                                          # :459-460
                continue
            elif length > self.max_ray_length:                                                        # :461
                pt_w = [_div(d[k], length) * self.max_ray_length + t[k] for k in range(3)]            # :463, written order
                idx = self._set_cache_occupancy(pt_w, 0)                                              # :464
            else:
                idx = self._set_cache_occupancy(pt_w, 1)                                              # :467
            if idx != INVALID_IDX:                                                                    # :470
                if idx in rayend:                                                                     # :472-475
                    continue
                rayend.add(idx)                                                                       # :477
            rays.append((i, pt_w))
        return t, rays

    # ---- raycastProcess (:441-533) ----
    def raycast(self, points, t_wc):
        """One frame into self.buffer, serially, as written.  Returns the stops: {sequence number: cells processed by the while loop}."""
        if len(points) == 0:                                                                          # :443-444
            self.stats = dict(rays=0, serial_steps=0, stops={})
            return {}
        t, rays = self._ends(points, t_wc)
        traverse = set()
        stops, nb = {}, self.step_bound()
        for i, pt_w in rays:
            rc = RayCaster()
            need_ray = rc.set_input([_div(pt_w[k], self._res) for k in range(3)], [_div(t[k], self._res) for k in range(3)])   # :483, p / resolution per component
            if not need_ray:                                                                          # :484-485
                continue
            ray_pt, on = rc.step()                                                                    # :488: the ray start is skipped
            if not on:
                continue
            n = 0
            while n < nb:                                                                             # (the step bound; the reference: while (raycaster.step(ray_pt)), :490)
                ray_pt, on = rc.step()
                if not on:
                    break
                n += 1
                tmp = [(ray_pt[k] + 0.5) * self._res for k in range(3)]                               # :492
                idx = self._set_cache_occupancy(tmp, 0)                                               # :493
                if idx != INVALID_IDX:                                                                # :494
                    if idx in traverse:                                                               # :497-498: counted above, then break
                        break
                    traverse.add(idx)                                                                 # :500
            stops[i] = n
        self.stats = dict(rays=len(rays), serial_steps=sum(stops.values()), stops=stops)
        self._batch_update()
        return stops

    def paths(self, points, t_wc):
        """The full voxel path of every cast ray (no early exit): (t, rays, {sequence number: [voxel or None per cell]})."""
        t, rays = self._ends(points, t_wc)
        nb, out = self.step_bound(), {}
        for i, pt_w in rays:
            rc = RayCaster()
            if not rc.set_input([_div(pt_w[k], self._res) for k in range(3)], [_div(t[k], self._res) for k in range(3)]):
                continue
            if not rc.step()[1]:
                continue
            path = []
            while len(path) < nb:
                ray_pt, on = rc.step()
                if not on:
                    break
                path.append(self._index([(ray_pt[k] + 0.5) * self._res for k in range(3)]))
            out[i] = path
        return t, rays, out

    def raycast_relaxed(self, points, t_wc, max_rounds=None):
        """The same frame by rounds -- what the device does.  State: count[i] = cells ray i processes (start: its whole path).
        A round: mark[v] = the lowest i whose first count[i] cells hold v; then count[i] = 1 + the first position whose voxel has
        mark < i, or is the voxel of the position before it (a ray that meets its own mark, :497); no such position: the whole
        path.  Rounds are counted up to and including the first that changes nothing.  Returns (stops, rounds); with max_rounds
        and no such round within it: (None, -max_rounds) and the map is left as it was."""
        if len(points) == 0:
            self.stats = dict(rays=0, serial_steps=0, full_steps=0, stops={})
            return {}, 1
        _, rays, paths = self.paths(points, t_wc)
        full = {i: len(p) for i, p in paths.items()}
        count = dict(full)
        rounds = 0
        while True:
            rounds += 1
            mark = {}
            for i, p in paths.items():
                for v in p[:count[i]]:
                    if v is not None and mark.get(v, i) >= i:
                        mark[v] = i
            changed = False
            for i, p in paths.items():
                c, prev = len(p), None
                for k, v in enumerate(p):
                    if v is not None and (mark.get(v, i) < i or v == prev):
                        c = k + 1
                        break
                    prev = v if v is not None else prev
                if c != count[i]:
                    count[i], changed = c, True
            if not changed:
                break
            if max_rounds is not None and rounds >= max_rounds:
                self.cache_all, self.cache_hit = {}, {}
                return None, -max_rounds
        for i, p in paths.items():
            for v in p[:count[i]]:
                if v is not None:
                    self.cache_all[v] = self.cache_all.get(v, 0) + 1
        self.stats = dict(rays=len(rays), serial_steps=sum(count.values()), full_steps=sum(full.values()), stops=dict(count))
        self._batch_update()
        return dict(count), rounds

    # ---- depthCallback's pair of calls (:291-292) with the frame kept for the shift filter (:360-361, :423-424) ----
    def fuse(self, depth_u16, K, T_wc, shift_filter=False, relaxed=False):
        T = np.asarray(T_wc, dtype=np.float64).reshape(4, 4)
        if not shift_filter:
            pts = self.project(depth_u16, K, T)
        else:
            if not self.has_first_depth:
                self.has_first_depth = True                                                           # :360-361: nothing is projected
                pts = []
            else:
                pts = self.project(depth_u16, K, T, last=self.last)
            self.last = (np.array(depth_u16, copy=True), T.copy())                                    # :423-424
        return self.raycast_relaxed(pts, T[:3, 3]) if relaxed else self.raycast(pts, T[:3, 3])


# ---- the synthetic frames of the fusion tests (CPU and GPU tests share them) ----
TEST_GEO = dict(origin=(-3.2, -3.2, 0.0), map_size=(6.4, 6.4, 3.2), resolution=0.1)                   # 64 x 64 x 32 voxels
TEST_ROWS, TEST_COLS = 48, 64
TEST_K = np.array([[40.0, 0.0, 31.5], [0.0, 40.0, 23.5], [0.0, 0.0, 1.0]])
SCENES = ("wall", "steps", "random")
PLACEMENTS = {"middle": (0.03, -0.02, 1.61), "near_face": (0.04, 2.9, 1.57)}                          # the second: 0.3 m from the +y face, half of its rays leave the map


def pose(t, yaw=0.3, pitch=-0.1):
    """Camera-to-world: the optical axis (camera z) along world x turned by yaw about world z and pitch about the camera's x;
    camera x = -world y, camera y = -world z at yaw = pitch = 0 (the rotation of the reference's T_ic0_, occ_map.cpp:794-797)."""
    base = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    Rz = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    T = np.eye(4)
    T[:3, :3] = Rz @ base @ Rx
    T[:3, 3] = t
    return T


def scene(name, seed=0, rows=TEST_ROWS, cols=TEST_COLS):
    """A uint16 depth image in millimetres: "wall" 1.2 m everywhere (neighbouring pixels share end voxels); "steps" columns alternating between 3 m and 6.5 m (beyond
    max_ray_length: clipped) in bands of 6 pixels; "random" uniform in [0.05, 7] m with a few zeros (no return)."""
    rng = np.random.default_rng(100 + seed)
    if name == "wall":
        d = np.full((rows, cols), 1200, dtype=np.uint16)
    elif name == "steps":
        d = np.where((np.arange(cols) // 6) % 2 == 0, 3000, 6500).astype(np.uint16)[None, :].repeat(rows, 0)
    elif name == "random":
        d = rng.integers(50, 7000, (rows, cols)).astype(np.uint16)
        d[rng.random((rows, cols)) < 0.03] = 0
    else:
        raise KeyError(name)
    return np.ascontiguousarray(d)
