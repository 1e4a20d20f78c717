"""The occupancy map on the device and what is read off it: sensor fusion and rendering, local and shared views with their grids, the
safety timer's checks, the distance field and per-flight clearance (frp_nmpc_occmap_*, _cloud_grid_build)."""
import ctypes

import numpy as np

from .capi import (CORRIDOR_LARGE_MAX_POINTS, CORRIDOR_MAX_CELLS, CORRIDOR_MAX_POINTS, FRP_ERR_ARG, OCCMAP_DIST_MAX_R, OCCMAP_VIEW_MAX_GROUPS,
                   CorridorCut, CorridorLarge, OccMap, OccMapBody, OccMapFuse, OccMapFuseBatch, OccMapFusePoints, OccMapRender, OccMapRenderScan,
                   OccMapSharedView, OccMapView, _check, checked_ptr, lib, optional_ptr, stream_ptr, tensor_ptr)

# OccMap's ROS parameter defaults (occ_map.cpp:752-754) and the local range of the reference's launch files
OCCMAP_DEFAULTS = dict(clamp_min_log=0.12, clamp_max_log=0.97, min_occupancy_log=0.80, local_radius=(6.0, 6.0, 3.0))

# depth fusion: the occ_map/* values of the reference's launch file (plan_manage/launch/advanced_param.xml:69-92); max_rounds 0 = the
# library's default number of relaxation rounds (FRP_OCCMAP_FUSE_DEFAULT_ROUNDS)
OCCMAP_FUSE_DEFAULTS = dict(depth_scale=1000.0, depth_filter_mindist=0.1, depth_filter_tolerance=0.2, depth_filter_margin=1, skip_pixel=2,
                            prob_hit_log=1.2, prob_miss_log=-0.5, min_ray_length=0.1, max_ray_length=6.0, max_rounds=0)
OCCMAP_FUSE_POINTS_PARAMS = ("prob_hit_log", "prob_miss_log", "min_ray_length", "max_ray_length", "max_rounds")  # the keys of OCCMAP_FUSE_DEFAULTS a point scan has

OCCMAP_BODY = (0.27, 0.0425)  # occ_map/ego_r, ego_h of the reference's launch file
SAFETY_INFLATE_CHECK, SAFETY_INFLATE_SEARCH = 1.2, 1.5  # checkReplanCallback's two ratios (nmpc_manage.cpp:291, :308, :333)

# CHOSEN, not derived: a radius of 20 voxels is 2 m at the reference's 0.1 m resolution -- beyond it a clearance reads +inf
OCCMAP_DIST_DEFAULT_R = 20


def goal_search_table():
    """The candidate offsets of checkReplanCallback's goal search (plan_manage/src/nmpc_manage.cpp:295-305), from its three loops run
    as written: r and nz are accumulated in double (r += dr, nz += dz) against `r <= 5 * dr + 1e-3` and `nz <= 1.6`, and theta
    runs over DEGREES (-90 ... 270 in steps of 30) but is handed to cos / sin as it is, i.e. as RADIANS -- that is the reference's
    behaviour, kept.  Row c is (r * cos(theta), r * sin(theta), nz): the device adds the first two to the goal and takes the third
    as the new z.  Returns (table [n_groups * group_size, 3] float64, n_groups, group_size); a group is one (r, theta) pair's nz
    loop, the loop the reference's `break` leaves.  The counts come from the loops (5 * 13 groups of 4 in IEEE double)."""
    import math
    dr, dtheta, dz = 0.2, 30.0, 0.2                                       # :295
    rows, sizes = [], []
    r = dr
    while r <= 5 * dr + 1e-3:                                             # :299
        theta = -90.0
        while theta <= 270:                                               # :300
            n = 0
            nz = 1.0
            while nz <= 1.6:                                              # :301
                rows.append((r * math.cos(theta), r * math.sin(theta), nz))  # :303-305
                n += 1
                nz += dz
            sizes.append(n)
            theta += dtheta
        r += dr
    assert len(set(sizes)) == 1, sizes
    return np.array(rows, dtype=np.float64).reshape(-1, 3), len(sizes), sizes[0]


def lidar_beams(rings, columns, elevation_min, elevation_max, azimuth_span=2 * np.pi):
    """The beam table of a spinning LiDAR for OccupancyMap.render_scan: [rings * columns, 3] float64 unit vectors in the SENSOR frame
    (x forward, z up) in firing order, column-major -- all rings of azimuth 0, then the next azimuth --, so that the 64 consecutive
    beams of a wavefront point in nearby directions.  az_j = azimuth_span * j / columns, el_i = elevation_min + (elevation_max -
    elevation_min) * i / (rings - 1) (elevation_min when rings == 1), beam = (cos(el) cos(az), cos(el) sin(az), sin(el)).  A
    convenience: frp_nmpc_occmap_render_scan_batch takes any table."""
    rings, columns = int(rings), int(columns)
    if rings < 1 or columns < 1:
        raise ValueError("lidar_beams: at least one ring and one column")
    i, j = np.arange(rings, dtype=np.float64), np.arange(columns, dtype=np.float64)
    el = np.full(rings, float(elevation_min)) if rings == 1 else float(elevation_min) + (float(elevation_max) - float(elevation_min)) * i / (rings - 1)
    az = float(azimuth_span) * j / columns
    out = np.empty((columns, rings, 3), dtype=np.float64)
    out[:, :, 0] = np.cos(el)[None, :] * np.cos(az)[:, None]
    out[:, :, 1] = np.cos(el)[None, :] * np.sin(az)[:, None]
    out[:, :, 2] = np.sin(el)[None, :]
    return out.reshape(rings * columns, 3)


class SafetyCheck:
    """What OccupancyMap.safety_check returns (int32 [B] device tensors): goal_blocked (the goal collided at ratio 1.2), goal_hits (how
    often the search moved it), first_hit (smallest colliding path sample, -1: none) and replan = goal_blocked | (first_hit >= 0),
    the mask DeviceFleet.replan(replan=...) and AstarPlanner.plan(active=...) take."""

    def __init__(self, goal_blocked, goal_hits, first_hit, replan):
        self.goal_blocked, self.goal_hits, self.first_hit, self.replan = goal_blocked, goal_hits, first_hit, replan


class LocalView:
    """What OccupancyMap.local_view returns (device tensors): local_box [B,6] int32 for AstarPlanner.plan / DeviceFleet.replan,
    cloud [B,P,3] f64 + cloud_count [B] int32 for corridor_batch_device / DeviceFleet.full_tick."""

    def __init__(self, local_box, cloud, cloud_count):
        self.local_box, self.cloud, self.cloud_count = local_box, cloud, cloud_count

    def overflowed(self):
        """Planners with more occupied voxels in range than the view stores (their count is minus the true one)."""
        return self.cloud_count < 0


class OccupancyMap:
    """The reference's OccMap (occ_grid/src/occ_map.cpp) in HBM, shared by all planners (frp_nmpc_occmap_*): the log-odds buffer,
    the byte grid the A* searches (.occ) and, per planner, the local box and the local obstacle cloud the corridor takes.
    world: the dict of workloads.astar_world -- its geometry, and its occ as the initial content (occupied voxels at
    clamp_max_log, the others at clamp_min_log); or explicit origin / map_size / resolution for an empty map.  fuse_depth() fuses a
    camera frame by ray casting (projectDepthImage / raycastProcess, include/frp_nmpc_occmap_fuse.h) with the reference's serial
    result to the bit, fuse_points() does the same ray casting for point scans (a LiDAR's cloud and the position it was taken from); a
    caller with another fusion of its own writes .log_odds and calls refresh().  render_depth() is the other
    direction: the depth images cameras at given poses see of this map (a ground-truth world feeding a belief map's fuse_depth_batch),
    and render_scan() the point scans a LiDAR's beam table measures in it (feeding fuse_points)."""

    def __init__(self, world=None, origin=None, map_size=None, resolution=None, local_radius=None, clamp_min_log=None,
                 clamp_max_log=None, min_occupancy_log=None, device="cuda:0"):
        import torch
        lib()
        self.torch = torch
        self.device = torch.device(device)
        d = dict(OCCMAP_DEFAULTS)
        for k, v in (("local_radius", local_radius), ("clamp_min_log", clamp_min_log), ("clamp_max_log", clamp_max_log),
                     ("min_occupancy_log", min_occupancy_log)):
            if v is not None:
                d[k] = v
        if world is not None:
            origin = world["origin"] if origin is None else origin
            map_size = world["map_size"] if map_size is None else map_size
            resolution = world["resolution"] if resolution is None else resolution
        self.origin = tuple(float(v) for v in origin); self.map_size = tuple(float(v) for v in map_size)
        self.resolution = float(resolution)
        self.local_radius = tuple(float(v) for v in d["local_radius"])
        self.clamp_min_log, self.clamp_max_log, self.min_occupancy_log = float(d["clamp_min_log"]), float(d["clamp_max_log"]), float(d["min_occupancy_log"])
        self.grid = tuple(int(np.ceil(m / self.resolution)) for m in self.map_size)  # occ_map.cpp:789
        self.world = world
        self.log_odds = torch.empty(self.grid, dtype=torch.float64, device=self.device)
        self.occ = torch.empty(self.grid, dtype=torch.uint8, device=self.device)
        m = self._map()
        self.ws_bytes = int(lib().frp_nmpc_occmap_workspace_bytes(ctypes.byref(m)))
        if self.ws_bytes == 0:
            raise ValueError("frp_nmpc_occmap refuses this map description (resolution, map_size, grid)")
        self.ws = torch.empty((self.ws_bytes // 4 + 1,), dtype=torch.int32, device=self.device)
        self.fuse_ws = None          # the fusion workspace: allocated by fuse_depth, grown when a larger frame needs it
        self.fuse_batch_ws = None    # the batched fusion's workspace: allocated by fuse_depth_batch, grown when a larger batch needs it
        self.fuse_points_ws = None   # the point scans' fusion workspace: allocated by fuse_points, grown when (S, P, max_ray_length) need more
        self._last_frame = None      # (depth, T_wc) of the previous filtered frame (last_depth_image, last_T_wc: occ_map.cpp:423-424)
        self._fusing_against = None  # the frame the latest filtered call reads on its stream: kept alive until the next call
        self._goal_table = None      # (table, n_groups, group_size) of goal_search_table() on the device: made by the first safety_check
        if world is not None and world.get("occ") is not None:
            o = torch.from_numpy(np.ascontiguousarray(world["occ"], dtype=np.uint8)).to(self.device)
            assert tuple(o.shape) == self.grid, (tuple(o.shape), self.grid)
            self.log_odds.fill_(self.clamp_min_log)
            self.log_odds.masked_fill_(o != 0, self.clamp_max_log)
            self.refresh()
        else:
            self.reset()

    def _map(self):
        return OccMap((ctypes.c_double * 3)(*self.origin), (ctypes.c_double * 3)(*self.map_size), self.resolution, (ctypes.c_int * 3)(*self.grid),
                      self.clamp_min_log, self.clamp_max_log, self.min_occupancy_log, (ctypes.c_double * 3)(*self.local_radius),
                      self.log_odds.data_ptr(), self.occ.data_ptr())

    def _call(self, name, *args, stream=None):
        m = self._map()
        _check(getattr(lib(), name)(ctypes.byref(m), *args, tensor_ptr(self.ws), self.ws_bytes, stream_ptr(stream, self.device)), name)

    def _dev(self, a, dtype):
        return self._upload(a, dtype).to(self.device, dtype=dtype).contiguous()

    def astar_world(self):
        """The constants AstarPlanner reads: the world this map was built from, or the launch-file defaults around its geometry."""
        if self.world is not None:
            return self.world
        from . import workloads
        w = dict(workloads.ASTAR_DEFAULTS)
        w.update(origin=self.origin, map_size=self.map_size, resolution=self.resolution)
        return w

    def reset(self, stream=None):
        """Every voxel back to clamp_min_log (occ_map.cpp:831)."""
        self._call("frp_nmpc_occmap_reset", stream=stream)

    def refresh(self, stream=None):
        """occ and the bit plane from log_odds, after the caller wrote log_odds itself."""
        self._call("frp_nmpc_occmap_refresh", stream=stream)

    def clear_box(self, min_pos, max_pos, stream=None):
        """resetBuffer(min_pos, max_pos) (occ_map.cpp:15-36); host positions."""
        self._call("frp_nmpc_occmap_clear_box", (ctypes.c_double * 3)(*[float(v) for v in min_pos]), (ctypes.c_double * 3)(*[float(v) for v in max_pos]),
                   stream=stream)

    def insert_cloud(self, points, stream=None):
        """globalCloudCallback (occ_map.cpp:600-622): points [P,3] float32 (pcl::PointXYZ; anything else is converted to it first)."""
        pts = self._dev(points, self.torch.float32)
        assert pts.dim() == 2 and pts.shape[1] == 3
        self._call("frp_nmpc_occmap_insert_cloud", tensor_ptr(pts) if pts.shape[0] else None, int(pts.shape[0]), stream=stream)
        self._record(stream, pts)

    # ---- what the sensor routes below share: one argument path ----

    def _upload(self, a, dtype, what=""):
        """An array as a device tensor of `dtype` (uint16: the array `what` has to be uint16 already); a tensor as it is."""
        t = self.torch
        if t.is_tensor(a):
            return a
        if dtype == t.uint16:
            a = np.ascontiguousarray(a)
            if a.dtype != np.uint16:
                raise TypeError(f"{what} must be uint16 (the reference's depth_image.at<uint16_t>)")
            return t.from_numpy(a.view(np.int16)).to(self.device).view(t.uint16)
        return t.from_numpy(np.ascontiguousarray(a, dtype={t.float64: np.float64, t.float32: np.float32, t.int32: np.int32}[dtype])).to(self.device)

    def _tensor(self, a, dtype, shape, message, exc=TypeError, upload=False):
        """The checked device tensor behind an argument: an array is uploaded first (upload), a tensor is used in place.
        shape: a tuple, None for an extent that is free.  Anything but a contiguous tensor of that dtype and shape on the map's
        device: exc(message)."""
        t = self.torch
        if upload:
            a = self._upload(a, dtype)
        if (not t.is_tensor(a) or a.dtype != dtype or a.dim() != len(shape) or any(n is not None and n != m for n, m in zip(shape, a.shape))
                or a.device != self.log_odds.device or not a.is_contiguous()):
            raise exc(message)
        return a

    def _image(self, a, shape, what):
        """depth / last_depth of fuse_depth_batch (uploaded when an array)"""
        return self._tensor(self._upload(a, self.torch.uint16, what), self.torch.uint16, shape, f"{what} must be a contiguous [F, rows, cols] uint16 tensor on the map's device")

    def _fuse_params(self, f, method, params, keys=None):
        """The ray and filter parameters of the description f (`keys`; None: all): OCCMAP_FUSE_DEFAULTS under the caller's params."""
        keys = keys or tuple(OCCMAP_FUSE_DEFAULTS)
        unknown = set(params) - set(keys)
        if unknown:
            raise TypeError(f"{method}: unknown parameters {sorted(unknown)}")
        for k in keys:
            v = params.get(k, OCCMAP_FUSE_DEFAULTS[k])
            setattr(f, k, int(v) if k in ("depth_filter_margin", "skip_pixel", "max_rounds") else float(v))

    def _fuse(self, name, query, ws, f, refused, stream):
        """A fusion call: the workspace description f asks for (`query`; 0: ValueError(refused)), kept in self.<ws> and grown when a
        larger description needs it, then the call on the stream."""
        m = self._map()
        need = int(getattr(lib(), query)(ctypes.byref(m), ctypes.byref(f)))
        if need == 0:
            raise ValueError(refused)
        w = getattr(self, ws)
        if w is None or w.numel() < need:
            w = self.torch.empty((need,), dtype=self.torch.uint8, device=self.device)
            setattr(self, ws, w)
        _check(getattr(lib(), name)(ctypes.byref(m), ctypes.byref(f), tensor_ptr(self.ws), self.ws_bytes, tensor_ptr(w),
                                    int(w.numel()), stream_ptr(stream, self.device)), name)

    def _render(self, name, r, header, stream):
        """A render call on the stream; ValueError for a description the library refuses."""
        m = self._map()
        rc = getattr(lib(), name)(ctypes.byref(m), ctypes.byref(r), tensor_ptr(self.ws), self.ws_bytes,
                                  stream_ptr(stream, self.device))
        if rc == FRP_ERR_ARG:
            raise ValueError(f"{name} refuses this description (see include/{header})")
        _check(rc, name)

    @staticmethod
    def _record(stream, *tensors):
        """The tensors a call on a stream of the caller's reads or writes stay allocated until it has run."""
        if stream is not None:
            for a in tensors:
                if a is not None:
                    a.record_stream(stream)

    def fuse_depth(self, depth, K, T_wc, *, shift_filter=False, status=None, stream=None, **params):
        """One camera frame into the map (OccMap::depthCallback's projectDepthImage + raycastProcess, occ_map.cpp:291-292):
        depth [rows, cols] uint16 (device tensor or array), K 3 x 3 intrinsics, T_wc 4 x 4 camera-to-world pose (host values).
        params: the keys of OCCMAP_FUSE_DEFAULTS.  log_odds, occ and the bit plane follow together -- no refresh().
        Returns the status tensor (int32 [2], device; nothing is synchronised): [0] relaxation rounds used, or minus max_rounds when
        the frame did not converge and the map was left untouched; [1] rays cast.
        shift_filter: the depth filter of :364-419 against the previous filtered frame, which the map keeps (with its pose)
        itself; the first filtered frame fuses nothing (has_first_depth_, :360-361) and returns [0, 0].
        status: a tensor to write into (a captured graph replays into the same buffer)."""
        t = self.torch
        f = OccMapFuse()
        self._fuse_params(f, "fuse_depth", params)
        depth = self._upload(depth, t.uint16, "depth")
        if depth.dtype != t.uint16 or depth.dim() != 2 or depth.device != self.log_odds.device:
            raise TypeError("depth must be a [rows, cols] uint16 tensor on the map's device")
        depth = depth.contiguous()
        T = np.ascontiguousarray(T_wc, dtype=np.float64).reshape(4, 4)
        Kh = np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        if status is None:
            status = t.zeros((2,), dtype=t.int32, device=self.device)
        assert status.dtype == t.int32 and status.numel() >= 2 and status.is_contiguous() and status.device == self.log_odds.device
        last = None
        if shift_filter:
            # The copy kept for the next frame is made on the stream of the call, behind whatever produced `depth` there (the caller
            # may reuse its tensor).  The previous frame stays referenced (_fusing_against) until the next call replaces it, so its
            # memory cannot go back to the allocator while this call's kernels, which read it, are still queued.
            with t.cuda.stream(stream if stream is not None else t.cuda.current_stream(self.device)):
                keep = depth.clone()
            last, self._last_frame = self._last_frame, (keep, T.copy())
            self._fusing_against = last
            if last is None:
                status.zero_()
                return status
            if tuple(last[0].shape) != tuple(depth.shape):
                raise ValueError("shift_filter: the frame size changed")
        f.rows, f.cols = int(depth.shape[0]), int(depth.shape[1])
        f.depth = depth.data_ptr()
        f.last_depth = last[0].data_ptr() if last is not None else None
        if last is not None:
            f.last_T_wc[:] = [float(v) for v in last[1].ravel()]
        f.K[:] = [float(v) for v in Kh.ravel()]
        f.T_wc[:] = [float(v) for v in T.ravel()]
        f.status = status.data_ptr()
        self._fuse("frp_nmpc_occmap_fuse_depth", "frp_nmpc_occmap_fuse_workspace_bytes", "fuse_ws", f,
                   "frp_nmpc_occmap_fuse_depth refuses this frame description (see include/frp_nmpc_occmap_fuse.h)", stream)
        self._record(stream, depth, last[0] if last is not None else None)
        return status

    def fuse_depth_batch(self, depth, K, T_wc, *, last_depth=None, last_T_wc=None, active=None, status=None, stream=None, **params):
        """F camera frames into the map in one call (include/frp_nmpc_occmap_fuse_batch.h): the map afterwards is, to the bit, what
        fuse_depth leaves after frames 0 ... F - 1 in that order; frames that are inactive, refused or not converged are skipped.
        depth [F, rows, cols] uint16, T_wc [F, 4, 4] float64; with the shift filter last_depth and last_T_wc of the same shapes (the
        caller keeps the previous frames; None: the unfiltered loops); active [F] int32 or None, 0 = the frame is not fused.  Each
        may be a numpy array, which is uploaded, or a device tensor, which is used IN PLACE: the poses are read by the kernels, so a
        captured call replays with whatever the caller has written into its tensors since.  K 3 x 3 (host) and params (the keys of
        OCCMAP_FUSE_DEFAULTS) are shared by the frames.
        Returns the status tensor (int32 [F, 2], device; nothing is synchronised): per frame [rounds used, rays cast] as fuse_depth
        reports them, [-max_rounds, rays] for a frame that did not converge (it contributes nothing, the others are fused),
        [0, 0] for an inactive frame, [OCCMAP_FUSE_REFUSED, 0] for a pose fuse_depth would refuse (non-finite, singular last rotation).
        status: a tensor to write into.  ValueError: a description the library refuses."""
        t = self.torch
        f = OccMapFuseBatch()
        self._fuse_params(f, "fuse_depth_batch", params)
        depth = self._image(depth, (None, None, None), "depth")
        F = int(depth.shape[0])
        T = self._tensor(T_wc, t.float64, (F, 4, 4), "T_wc must be a contiguous [F, 4, 4] float64 tensor on the map's device", upload=True)
        if (last_depth is None) != (last_T_wc is None):
            raise ValueError("fuse_depth_batch: last_depth and last_T_wc go together")
        last = lastT = None
        if last_depth is not None:
            last = self._image(last_depth, (None, None, None), "last_depth")
            lastT = self._tensor(last_T_wc, t.float64, (F, 4, 4), "last_T_wc must be a contiguous [F, 4, 4] float64 tensor on the map's device", upload=True)
            if tuple(last.shape) != tuple(depth.shape):
                raise ValueError("fuse_depth_batch: last_depth has another shape than depth")
        if active is not None:
            active = self._tensor(active, t.int32, (F,), "active must be a contiguous [F] int32 tensor on the map's device", upload=True)
        if status is None:
            status = t.zeros((F, 2), dtype=t.int32, device=self.device)
        self._tensor(status, t.int32, (F, 2), "status must be a contiguous [F, 2] int32 tensor on the map's device")
        Kh = np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        f.frames, f.rows, f.cols = F, int(depth.shape[1]), int(depth.shape[2])
        f.depth, f.T_wc, f.status = depth.data_ptr(), T.data_ptr(), status.data_ptr()
        f.last_depth, f.last_T_wc, f.active = tensor_ptr(last), tensor_ptr(lastT), tensor_ptr(active)
        f.K[:] = [float(v) for v in Kh.ravel()]
        self._fuse("frp_nmpc_occmap_fuse_depth_batch", "frp_nmpc_occmap_fuse_batch_workspace_bytes", "fuse_batch_ws", f,
                   "frp_nmpc_occmap_fuse_depth_batch refuses this batch description (see include/frp_nmpc_occmap_fuse_batch.h)", stream)
        self._record(stream, depth, T, last, lastT, active)
        return status

    def fuse_points(self, points, origin, *, count=None, active=None, status=None, stream=None, **params):
        """S point scans into the map in one call (include/frp_nmpc_occmap_fuse_points.h): raycastProcess (occ_map.cpp:441-533) for
        a sensor that delivers a cloud in the world frame and the position it was taken from -- a LiDAR, a stereo rig.  The map
        afterwards is, to the bit, what fusing scans 0 ... S - 1 one after the other leaves; scans that are inactive, refused or not
        converged are skipped.  log_odds, occ and the bit plane follow together -- no refresh().
        points: a contiguous DEVICE tensor [S, P, 3], or [P, 3] for one scan, float64 or float32 (a float is widened exactly), used IN
        PLACE; a point with a NaN or infinite coordinate ("no return") is dropped and keeps its index.  origin [S, 3] or [3]
        float64, count [S] int32 or None (every scan holds P points; storage beyond count[s] is not read) and active [S] int32 or
        None may be numpy arrays, which are uploaded, or device tensors, which are used in place: the kernels read them, so a
        captured call replays with whatever the caller has written into its tensors since.  params: prob_hit_log, prob_miss_log,
        min_ray_length, max_ray_length, max_rounds of OCCMAP_FUSE_DEFAULTS, shared by the scans.
        Returns the status tensor (int32 [S, 2], device; nothing is synchronised) as fuse_depth_batch does: [rounds used, rays cast],
        [-max_rounds, rays] for a scan that did not converge, [0, 0] inactive, [OCCMAP_FUSE_REFUSED, 0] for a non-finite origin.
        status: a tensor to write into.  ValueError: arguments of another kind than described, or a description the library refuses."""
        t = self.torch
        f = OccMapFusePoints()
        self._fuse_params(f, "fuse_points", params, OCCMAP_FUSE_POINTS_PARAMS)
        if not t.is_tensor(points) or points.device != self.log_odds.device:
            raise ValueError("fuse_points: points must be a tensor on the map's device")
        if points.dtype not in (t.float64, t.float32):
            raise ValueError(f"fuse_points: points must be float64 or float32, not {points.dtype}")
        if points.dim() not in (2, 3) or points.shape[-1] != 3:
            raise ValueError(f"fuse_points: points must be [S, P, 3] or [P, 3], not {tuple(points.shape)}")
        if not points.is_contiguous():
            raise ValueError("fuse_points: points must be contiguous")
        S, P = (1, int(points.shape[0])) if points.dim() == 2 else (int(points.shape[0]), int(points.shape[1]))

        def per_scan(a, dtype, shape, what):
            a = self._upload(a, dtype)
            if S == 1 and a.dim() == len(shape) - 1 and a.is_contiguous():
                a = a.reshape(shape)  # one scan given without its leading dimension: a view, still the caller's storage
            return self._tensor(a, dtype, shape, f"fuse_points: {what} must be a contiguous {list(shape)} {dtype} tensor on the map's device "
                                "(or an array of that shape)", ValueError)

        origin = per_scan(origin, t.float64, (S, 3), "origin")
        if count is not None:
            count = per_scan(count, t.int32, (S,), "count")
        if active is not None:
            active = per_scan(active, t.int32, (S,), "active")
        if status is None:
            status = t.zeros((S, 2), dtype=t.int32, device=self.device)
        self._tensor(status, t.int32, (S, 2), "fuse_points: status must be a contiguous [S, 2] int32 tensor on the map's device", ValueError)
        f.scans, f.P = S, P
        f.points = points.data_ptr() if P > 0 and points.dtype == t.float64 else None
        f.points_f32 = points.data_ptr() if P > 0 and points.dtype == t.float32 else None
        f.count, f.active = tensor_ptr(count), tensor_ptr(active)
        f.origin, f.status = origin.data_ptr(), status.data_ptr()
        self._fuse("frp_nmpc_occmap_fuse_points_batch", "frp_nmpc_occmap_fuse_points_workspace_bytes", "fuse_points_ws", f,
                   f"frp_nmpc_occmap_fuse_points_batch refuses this description: {S} scans of {P} points (see include/frp_nmpc_occmap_fuse_points.h)", stream)
        self._record(stream, points, origin, count, active)
        return status

    def render_depth(self, T_wc, K, rows, cols, *, max_range, depth_scale=1000.0, active=None, out=None, voxel=None, status=None, stream=None):
        """What F cameras at the poses T_wc see of THIS map (include/frp_nmpc_occmap_render.h): the depth images
        [F, rows, cols] uint16 that fuse_depth_batch takes, one ray per pixel walked through the bit plane.  T_wc [F, 4, 4] float64
        and active [F] int32 (or None) may be numpy arrays, which are uploaded, or device tensors, which are used IN PLACE: the
        kernels read them, so a captured call replays with whatever the caller has written since.  K 3 x 3 (host), max_range in
        metres along the ray.  out: the depth tensor to write into (an inactive frame's image keeps what it holds; a fresh one is
        zero); voxel: an int32 tensor [F, rows, cols] for the linear voxel index of every return (-1: none), or None; status: an
        int32 tensor [F, 2] for {1, returns} / {0, 0} inactive / {OCCMAP_FUSE_REFUSED, 0} a non-finite pose.  Returns the depth
        tensor; nothing is synchronised.  ValueError: a description the library refuses."""
        t = self.torch
        T_wc = self._tensor(T_wc, t.float64, (None, 4, 4), "T_wc must be a contiguous [F, 4, 4] float64 tensor on the map's device", upload=True)
        F, rows, cols = int(T_wc.shape[0]), int(rows), int(cols)
        if active is not None:
            active = self._tensor(active, t.int32, (F,), "active must be a contiguous [F] int32 tensor on the map's device", upload=True)
        if F < 1 or rows < 1 or cols < 1:
            raise ValueError("render_depth: at least one frame, one row and one column")
        if out is None:
            out = t.zeros((F, rows, cols), dtype=t.int16, device=self.device).view(t.uint16)
        self._tensor(out, t.uint16, (F, rows, cols), "out must be a contiguous [F, rows, cols] uint16 tensor on the map's device")
        if voxel is not None:
            self._tensor(voxel, t.int32, (F, rows, cols), "voxel must be a contiguous [F, rows, cols] int32 tensor on the map's device")
        if status is None:
            status = t.zeros((F, 2), dtype=t.int32, device=self.device)
        self._tensor(status, t.int32, (F, 2), "status must be a contiguous [F, 2] int32 tensor on the map's device")
        r = OccMapRender()
        r.frames, r.rows, r.cols = F, rows, cols
        r.T_wc, r.active = T_wc.data_ptr(), tensor_ptr(active)
        r.K[:] = [float(v) for v in np.ascontiguousarray(K, dtype=np.float64).reshape(9)]
        r.depth_scale, r.max_range = float(depth_scale), float(max_range)
        r.depth, r.voxel, r.status = out.data_ptr(), tensor_ptr(voxel), status.data_ptr()
        self._render("frp_nmpc_occmap_render_depth", r, "frp_nmpc_occmap_render.h", stream)
        self._record(stream, T_wc, active, out, voxel, status)
        return out

    def render_scan(self, T_ws, beams, *, max_range, min_range=0.0, far_range=0.0, dtype=None, active=None, points=None, points_f32=None,
                    origin=None, count=None, range=None, voxel=None, status=None, stream=None):
        """What S range sensors at the poses T_ws measure of THIS map along a table of P beam directions
        (include/frp_nmpc_occmap_render_scan.h): the point scans [S, P, 3] in the world frame that fuse_points takes, in beam order,
        with their origins [S, 3] and counts [S] written on the device -- camera_poses -> render_scan -> fuse_points needs no host.
        T_ws [S, 4, 4] float64 sensor-to-world, beams [P, 3] float64 in the sensor frame (any length; lidar_beams() makes a spinning
        LiDAR's) and active [S] int32 (or None) may be numpy arrays, which are uploaded, or device tensors, which are used IN PLACE: the
        kernels read them, so a captured call replays with whatever the caller has written since.  max_range, min_range: metres along
        the beam.  A beam without a return gives a NaN point (fuse_points drops it), or with far_range >= max_range the point at
        far_range along the beam (fused with max_ray_length < far_range: a miss that carves free space).
        dtype: torch.float64 (the default) or torch.float32, the type of the points returned.  The output tensors are used if given,
        so that a captured call replays into them: points [S, P, 3] (its dtype then decides), points_f32 [S, P, 3] float32 written
        as well as float64 points (each float is the double rounded once), origin [S, 3] float64, count [S] int32, range [S, P]
        float64 (metres along the beam of the return, 0: none), voxel [S, P] int32 (linear voxel index of the return, -1: none),
        status [S, 2] int32 ({1, returns} / {0, 0} inactive, nothing of the scan written but count 0 / {OCCMAP_FUSE_REFUSED, 0} a
        non-finite pose, its points NaN).  Returns (points, origin, count, status); nothing is synchronised.  ValueError: a
        description the library refuses."""
        t = self.torch

        def given(a, dt, shape, what, free=False, upload=False):  # free: the shape was checked by the caller, its message says none
            return self._tensor(a, dt, shape, f"render_scan: {what} must be a contiguous {'' if free else list(shape)} {dt} tensor on the map's device",
                                upload=upload)

        T_ws = self._upload(T_ws, t.float64)
        if T_ws.dim() != 3 or tuple(T_ws.shape[1:]) != (4, 4):
            raise TypeError("render_scan: T_ws must be [S, 4, 4]")
        T_ws = given(T_ws, t.float64, (None, 4, 4), "T_ws", free=True)
        if not t.is_tensor(beams):
            beams = t.from_numpy(np.array(beams, dtype=np.float64, order="C")).to(self.device)  # (a copy: a table kept read-only uploads too)
        if beams.dim() != 2 or beams.shape[1] != 3:
            raise TypeError("render_scan: beams must be [P, 3]")
        beams = given(beams, t.float64, (None, 3), "beams", free=True)
        S, P = int(T_ws.shape[0]), int(beams.shape[0])
        if S < 1 or P < 1:
            raise ValueError("render_scan: at least one scan and one beam")
        if active is not None:
            active = given(active, t.int32, (S,), "active", upload=True)
        if points is None:
            dtype = t.float64 if dtype is None else dtype
            if dtype not in (t.float64, t.float32):
                raise TypeError(f"render_scan: dtype must be float64 or float32, not {dtype}")
            points = t.full((S, P, 3), float("nan"), dtype=dtype, device=self.device)
        elif not t.is_tensor(points) or points.dtype not in (t.float64, t.float32) or (dtype is not None and points.dtype != dtype):
            raise TypeError("render_scan: points must be a float64 or float32 tensor of the dtype asked for")
        points = given(points, points.dtype, (S, P, 3), "points")
        if points_f32 is not None:
            if points.dtype != t.float64:
                raise TypeError("render_scan: points_f32 goes with float64 points")
            points_f32 = given(points_f32, t.float32, (S, P, 3), "points_f32")
        origin = t.zeros((S, 3), dtype=t.float64, device=self.device) if origin is None else given(origin, t.float64, (S, 3), "origin")
        count = t.zeros((S,), dtype=t.int32, device=self.device) if count is None else given(count, t.int32, (S,), "count")
        status = t.zeros((S, 2), dtype=t.int32, device=self.device) if status is None else given(status, t.int32, (S, 2), "status")
        if range is not None:
            range = given(range, t.float64, (S, P), "range")
        if voxel is not None:
            voxel = given(voxel, t.int32, (S, P), "voxel")
        r = OccMapRenderScan()
        r.scans, r.P = S, P
        r.beams, r.T_ws, r.active = beams.data_ptr(), T_ws.data_ptr(), tensor_ptr(active)
        r.min_range, r.max_range, r.far_range = float(min_range), float(max_range), float(far_range)
        r.points = points.data_ptr() if points.dtype == t.float64 else None
        r.points_f32 = points.data_ptr() if points.dtype == t.float32 else tensor_ptr(points_f32)
        r.origin, r.count, r.status = origin.data_ptr(), count.data_ptr(), status.data_ptr()
        r.range, r.voxel = tensor_ptr(range), tensor_ptr(voxel)
        self._render("frp_nmpc_occmap_render_scan_batch", r, "frp_nmpc_occmap_render_scan.h", stream)
        self._record(stream, T_ws, beams, active, points, points_f32, origin, count, range, voxel, status)
        return points, origin, count, status

    def camera_poses(self, state, T_bc, out=None, stream=None):
        """T_wc [B, 4, 4] = T_wb(state) T_bc for planner states [B, 9] (position, velocity, Euler angles; device tensor, used in
        place, or array) and the body-to-camera transform T_bc 4 x 4 (host): what render_depth and fuse_depth_batch take as poses,
        computed where the states are (frp_nmpc_occmap_camera_poses).  out: the tensor to write into."""
        t = self.torch
        st = self._tensor(state, t.float64, (None, 9), "state must be a contiguous [B, 9] float64 tensor on the map's device", upload=True)
        B = int(st.shape[0])
        if out is None:
            out = t.zeros((B, 4, 4), dtype=t.float64, device=self.device)
        self._tensor(out, t.float64, (B, 4, 4), "out must be a contiguous [B, 4, 4] float64 tensor on the map's device")
        Tb = (ctypes.c_double * 16)(*[float(v) for v in np.ascontiguousarray(T_bc, dtype=np.float64).reshape(16)])
        _check(lib().frp_nmpc_occmap_camera_poses(B, tensor_ptr(st) if B else None, Tb, tensor_ptr(out) if B else None,
                                                  stream_ptr(stream, self.device)), "frp_nmpc_occmap_camera_poses")
        self._record(stream, st, out)
        return out


    def local_view(self, centres, P, out=None, stream=None):
        """local_box + localOccVisCallback's cloud (occ_map.cpp:177-215) of every planner: centres [B,3] f64 (device tensor or
        array), P points stored per planner.  centres = None: the whole map as one cloud (globalOccVisCallback, :150-175), B = 1.
        out: a LocalView of the same shapes to write into (a captured graph replays into the same buffers).  Nothing is
        synchronised: cloud_count (negative = overflow, LocalView.overflowed()) is a device tensor.
        P = 0 stores no cloud: local_box alone (cloud_count = minus each planner's count).  That is the per-tick call of the
        shared-cloud route -- shared_view() once per map change, then per tick local_view(centres, 0) and cut(view.local_box)."""
        t = self.torch
        c = None if centres is None else self._dev(centres, t.float64)
        B = 1 if c is None else int(c.shape[0])
        assert c is None or tuple(c.shape) == (B, 3)
        if out is None:
            out = LocalView(t.zeros((B, 6), dtype=t.int32, device=self.device), t.zeros((B, P, 3), dtype=t.float64, device=self.device),
                            t.zeros((B,), dtype=t.int32, device=self.device))
        assert tuple(out.cloud.shape) == (B, P, 3) and out.cloud.is_contiguous() and tuple(out.local_box.shape) == (B, 6)
        v = OccMapView(B, c.data_ptr() if c is not None else None, P, out.local_box.data_ptr(), out.cloud.data_ptr() if P else None,
                       out.cloud_count.data_ptr())
        self._call("frp_nmpc_occmap_local_view", ctypes.byref(v), stream=stream)
        if stream is not None and c is not None and c is not centres:
            c.record_stream(stream)
        return out

    def cut(self, local_box):
        """The visibility cut of frp_nmpc_corridor_batch_cut for local_box [B,6] int32 (device tensor, LocalView.local_box): what
        corridor_batch_device / DeviceFleet.corridor / full_tick take as `cut` beside the shared cloud of shared_view().  Planner b
        then sees the points with origin + min_id * resolution <= q < origin + max_id * resolution per axis -- its local cloud."""
        t = self.torch
        assert t.is_tensor(local_box) and local_box.dtype == t.int32 and local_box.dim() == 2 and local_box.shape[1] == 6 and local_box.is_contiguous()
        assert local_box.device == self.log_odds.device
        c = CorridorCut(local_box.data_ptr(), (ctypes.c_double * 3)(*self.origin), self.resolution)
        c._box = local_box
        return c

    def shared_view(self, cell=0.5, stream=None):
        """The whole-map cloud (local_view(None, .), every occupied voxel's centre in x, y, z order) trimmed to its count, and a
        CloudGrid over it: (cloud [n,3] f64, grid).  The grid is laid over the map itself -- origin = the map's, dims =
        ceil(map_size / cell) -- so nothing is read back to find its bounds.  ONE synchronisation, to read the count: call it
        when the map changes (insert_cloud / clear_box / refresh), not per tick.  A shared cloud holds at most
        FRP_CORRIDOR_MAX_POINTS points; a map with more occupied voxels raises ValueError (use per-planner clouds)."""
        t = self.torch
        s = stream if stream is not None else t.cuda.current_stream(self.device)
        v = self.local_view(None, CORRIDOR_MAX_POINTS, stream=stream)
        with t.cuda.stream(s):
            n = int(v.cloud_count[0].item())   # the one synchronisation
        if n < 0:
            raise ValueError(f"the map holds {-n} occupied voxels, a shared cloud at most FRP_CORRIDOR_MAX_POINTS = {CORRIDOR_MAX_POINTS}: "
                             "use per-planner clouds (local_view(centres, P))")
        with t.cuda.stream(s):
            cloud = v.cloud[0, :n].clone()
        dims = tuple(max(1, int(np.ceil(m / float(cell)))) for m in self.map_size)
        return cloud, CloudGrid(cloud, cell, origin=self.origin, dims=dims, stream=stream)

    def shared_view_device(self, cap=CORRIDOR_MAX_POINTS, cell=0.5, planners=4096):
        """A SharedView of this map: the cloud and grid of shared_view() in persistent buffers of `cap` points, rebuilt by
        SharedView.update() with nothing on the host.  The per-tick form of the shared-cloud route when the map changes every tick.
        cap may exceed CORRIDOR_MAX_POINTS, up to CORRIDOR_LARGE_MAX_POINTS: a LARGE view, for at most `planners` planners per
        corridor call (see SharedView)."""
        return SharedView(self, cap, cell, planners)

    def query(self, pos, local_box=None, planner=None, stream=None):
        """getVoxelState (occ_map.cpp:95-106) of pos [Q,3]: int32 [Q] device tensor, -1 outside the map, 0 free or outside the local
        map, 1 occupied.  local_box [.,6] of a local view with planner [Q] = its row per query (None: row 0)."""
        t = self.torch
        q = self._dev(pos, t.float64)
        Q = int(q.shape[0])
        st = t.zeros((Q,), dtype=t.int32, device=self.device)
        pl = None if planner is None else self._dev(planner, t.int32)
        lb = None if local_box is None else self._dev(local_box, t.int32)
        self._call("frp_nmpc_occmap_query", Q, tensor_ptr(q) if Q else None, pl.data_ptr() if pl is not None else None,
                   lb.data_ptr() if lb is not None else None, tensor_ptr(st), stream=stream)
        self._record(stream, q, pl, lb)
        return st


    def check_surround(self, pos, inflate_ratio, local_box=None, planner=None, body=OCCMAP_BODY, stream=None):
        """checkPosSurround(pos, inflate_ratio) (occ_map.cpp:625-643) of pos [Q,3]: int32 [Q] device tensor, 1 = free (every probe of
        the inflated body is 0), 0 = collision (a probe is occupied or outside the map).  local_box / planner as in query()."""
        t = self.torch
        q = self._dev(pos, t.float64)
        Q = int(q.shape[0])
        assert tuple(q.shape) == (Q, 3)
        out = t.zeros((Q,), dtype=t.int32, device=self.device)
        pl = None if planner is None else self._dev(planner, t.int32)
        lb = None if local_box is None else self._dev(local_box, t.int32)
        bd = OccMapBody(float(body[0]), float(body[1]))
        self._call("frp_nmpc_occmap_check_surround", ctypes.byref(bd), float(inflate_ratio), Q, q.data_ptr() if Q else None,
                   pl.data_ptr() if pl is not None else None, lb.data_ptr() if lb is not None else None, out.data_ptr(), stream=stream)
        self._record(stream, q, pl, lb)
        return out

    def safety_check(self, end_pt, kino_path, kino_size, have_target=None, have_traj=None, local_box=None, stride=5, stream=None,
                     body=OCCMAP_BODY, out=None):
        """One tick of the safety timer (NMPCManage::checkReplanCallback, nmpc_manage.cpp:285-341) for B planners, on the live bit
        plane: the goal test and search (frp_nmpc_occmap_check_goals; end_pt [B,3] f64 device tensor, UPDATED IN PLACE where the
        search moves a blocked goal) and the path walk (frp_nmpc_occmap_check_paths; kino_path [B,K,3] f64 / kino_size [B] int32 as
        AstarPlanner keeps them, every stride-th sample).  have_target / have_traj: int32 [B] or None (all set); local_box [B,6] of
        a local view or None.  Returns a SafetyCheck; nothing is synchronised.  out: a SafetyCheck to write into (a captured
        graph replays into the same buffers).  The FSM transitions stay with the caller."""
        t = self.torch
        dev = self.log_odds.device
        for a, dt in ((end_pt, t.float64), (kino_path, t.float64), (kino_size, t.int32)):
            assert t.is_tensor(a) and a.dtype == dt and a.is_contiguous() and a.device == dev
        B, K = int(kino_path.shape[0]), int(kino_path.shape[1])
        assert tuple(kino_path.shape) == (B, K, 3) and tuple(end_pt.shape) == (B, 3) and tuple(kino_size.shape) == (B,)
        opt = [None if a is None else self._dev(a, t.int32) for a in (have_target, have_traj, local_box)]
        ht, hj, lb = opt
        assert lb is None or tuple(lb.shape) == (B, 6)
        if out is None:
            z = lambda: t.zeros((B,), dtype=t.int32, device=self.device)
            out = SafetyCheck(z(), z(), z(), z())
        if self._goal_table is None:
            tab, ng, gs = goal_search_table()
            self._goal_table = (t.from_numpy(tab).to(self.device), ng, gs)
        tab, ng, gs = self._goal_table
        bd = OccMapBody(float(body[0]), float(body[1]))
        s = stream if stream is not None else t.cuda.current_stream(self.device)
        self._call("frp_nmpc_occmap_check_goals", ctypes.byref(bd), SAFETY_INFLATE_CHECK, SAFETY_INFLATE_SEARCH, B, end_pt.data_ptr(), tensor_ptr(ht), tensor_ptr(lb),
                   ng, gs, tab.data_ptr(), out.goal_blocked.data_ptr(), out.goal_hits.data_ptr(), stream=stream)
        self._call("frp_nmpc_occmap_check_paths", ctypes.byref(bd), SAFETY_INFLATE_CHECK, B, K, int(stride), kino_path.data_ptr(), kino_size.data_ptr(),
                   tensor_ptr(hj), tensor_ptr(lb), out.first_hit.data_ptr(), stream=stream)
        with t.cuda.stream(s):
            t.bitwise_or(out.goal_blocked, (out.first_hit >= 0).to(t.int32), out=out.replan)
        self._record(stream, end_pt, kino_path, kino_size, tab, out.goal_blocked, out.goal_hits, out.first_hit, out.replan, *opt)
        return out

    def distance_field(self, R=OCCMAP_DIST_DEFAULT_R, border=True):
        """A DistanceField of this map (include/frp_nmpc_occmap_distance.h), built once from the bit plane as it is now.  R: the radius in
        voxels, 1 ... OCCMAP_DIST_MAX_R; the default of 20 is 2 m at the reference's 0.1 m resolution -- CHOSEN, not derived.  border:
        voxels outside the map count as occupied (checkPosSurround's reading)."""
        return DistanceField(self, R, border)


class DistanceField:
    """The truncated distance field of an OccupancyMap, on the device (include/frp_nmpc_occmap_distance.h): field [gx, gy, gz] uint16, the
    exact integer squared distance in voxels from each voxel to the nearest occupied one where that is <= R * R, else OCCMAP_DIST_FAR;
    with border=True the voxels outside the map count as occupied.  It has no reference counterpart (the reference's map keeps no
    distance).  Owns `field` and the scratch of the three passes; update() rebuilds from the map's CURRENT bit plane -- the field does
    not follow the map by itself.  clearance(pos) is resolution * sqrt(field) at the positions' voxels: a distance between voxel
    CENTRES (the header says what that bounds), +inf beyond R, 0.0 inside an occupied voxel, outside the map or for a position that is
    not finite."""

    def __init__(self, occmap, R=OCCMAP_DIST_DEFAULT_R, border=True):
        t = occmap.torch
        self.torch, self.occmap, self.R, self.border = t, occmap, int(R), bool(border)
        if not 1 <= self.R <= OCCMAP_DIST_MAX_R:
            raise ValueError(f"DistanceField: R is 1 ... {OCCMAP_DIST_MAX_R} voxels")
        m = occmap._map()
        self.scratch_bytes = int(lib().frp_nmpc_occmap_distance_scratch_bytes(ctypes.byref(m), self.R))
        if self.scratch_bytes == 0:
            raise ValueError("frp_nmpc_occmap_distance refuses this map description")
        self.field = t.empty(occmap.grid, dtype=t.uint16, device=occmap.device)
        self.scratch = t.empty((self.scratch_bytes,), dtype=t.uint8, device=occmap.device)
        self.update()

    def update(self, stream=None):
        """frp_nmpc_occmap_distance_update: field <- the definition on the map's bit plane as the stream finds it (three launches)."""
        o = self.occmap
        m = o._map()
        _check(lib().frp_nmpc_occmap_distance_update(ctypes.byref(m), self.R, int(self.border), tensor_ptr(self.field), tensor_ptr(self.scratch),
                                                     self.scratch_bytes, tensor_ptr(o.ws), o.ws_bytes, stream_ptr(stream, self.field.device)), "frp_nmpc_occmap_distance_update")

    def clearance(self, pos, d2=False, stream=None):
        """frp_nmpc_occmap_clearance of pos [Q,3] (float64 device tensor, or an array that is uploaded): float64 [Q] device tensor; with
        d2=True (clear, d2) with d2 int32 [Q]: the field's integer, OCCMAP_DIST_FAR included, -1 outside the map."""
        t, o = self.torch, self.occmap
        q = o._dev(pos, t.float64)
        Q = int(q.shape[0])
        assert tuple(q.shape) == (Q, 3)
        clear = t.zeros((Q,), dtype=t.float64, device=o.device)
        sq = t.zeros((Q,), dtype=t.int32, device=o.device) if d2 else None
        m = o._map()
        _check(lib().frp_nmpc_occmap_clearance(ctypes.byref(m), tensor_ptr(self.field), self.R, Q, q.data_ptr() if Q else None,
                                               clear.data_ptr() if Q else None, sq.data_ptr() if d2 and Q else None, stream_ptr(stream, self.field.device)),
               "frp_nmpc_occmap_clearance")
        o._record(stream, q, clear, sq)
        return (clear, sq) if d2 else clear


class FlightClearance:
    """How close every vehicle of a Vehicle came to an obstacle, on the device (frp_nmpc_occmap_clearance_trace): min_clear [B] float64
    (+inf until something nearer than the field's radius was seen), hits [B] int32 (samples with clearance 0.0: inside an occupied
    voxel, outside the map or not finite) and samples [B] int32.  It hooks into nothing: the caller launches update() after
    Vehicle.step / FleetFSM.period(..., vehicle=...), inside the same captured graph if they wish.  The positions are the TRUE plant
    states of the vehicle's trace, and the numbers are distances between voxel centres (include/frp_nmpc_occmap_distance.h); the
    body's radius is the caller's to subtract.  Tracking error and the rest of a flight record are flight.FlightRecord's, whose
    summary() folds this object's min_clear and hits in (FlightRecord(vehicle, clearance=this))."""

    def __init__(self, vehicle, field):
        t = vehicle.torch
        dev = vehicle.x.device
        if field.field.device != dev:
            raise ValueError("FlightClearance: the vehicle and the distance field are on different devices")
        self.torch, self.vehicle, self.field, self.B = t, vehicle, field, vehicle.B
        self.min_clear = t.full((self.B,), float("inf"), dtype=t.float64, device=dev)
        self.hits, self.samples = t.zeros((self.B,), dtype=t.int32, device=dev), t.zeros((self.B,), dtype=t.int32, device=dev)

    def update(self, trace=None, active=None, stream=None):
        """The S samples of trace [B,S,stride >= 3] (float64; None: vehicle.trace, or else the attached estimator's meas -- the fallback
        Vehicle.step writes to) taken in order into min_clear, hits and samples; active [B] int32 or None: where it is 0 nothing of
        that vehicle changes."""
        t, v = self.torch, self.vehicle
        if trace is None:
            trace = v.trace if v.trace is not None else v.estimator.meas if v.estimator is not None else None
            if trace is None:
                raise ValueError("FlightClearance.update: this Vehicle keeps no trace (trace=True) and has no ForceEstimator attached; pass trace=")
        assert t.is_tensor(trace) and trace.dim() == 3, "trace is a [B, S, stride] tensor"
        S, stride = int(trace.shape[1]), int(trace.shape[2])
        if S < 1 or stride < 3:
            raise ValueError("FlightClearance.update: trace is [B, S >= 1, stride >= 3]")
        a = optional_ptr(v.x, active, t.int32, (self.B,))
        f = self.field
        m = f.occmap._map()
        _check(lib().frp_nmpc_occmap_clearance_trace(ctypes.byref(m), tensor_ptr(f.field), f.R, self.B, S, stride,
                                                     checked_ptr(v.x, trace, t.float64, (self.B, S, stride)), a, tensor_ptr(self.min_clear),
                                                     tensor_ptr(self.hits), tensor_ptr(self.samples), stream_ptr(stream, v.x)),
               "frp_nmpc_occmap_clearance_trace")

    def reset(self, mask=None, stream=None):
        """frp_nmpc_occmap_clearance_reset: where mask [B] int32 != 0 (None: everywhere) min_clear <- +inf, hits <- 0, samples <- 0."""
        t, v = self.torch, self.vehicle
        m = optional_ptr(v.x, mask, t.int32, (self.B,))
        _check(lib().frp_nmpc_occmap_clearance_reset(self.B, m, tensor_ptr(self.min_clear), tensor_ptr(self.hits),
                                                     tensor_ptr(self.samples), stream_ptr(stream, v.x)), "frp_nmpc_occmap_clearance_reset")


class CloudGrid:
    """Uniform grid over a shared obstacle cloud (frp_nmpc_cloud_grid_build): built once per cloud, handed to
    corridor_batch_device / DeviceFleet.corridor so that a decomposition reads only the cells its local box touches."""

    def __init__(self, cloud, cell=0.5, origin=None, dims=None, stream=None):
        import torch
        assert cloud.dim() == 2 and cloud.shape[1] == 3 and cloud.is_contiguous() and cloud.dtype == torch.float64
        P = cloud.shape[0]
        if origin is None or dims is None:  # bounds of the cloud itself (host round trip; a map normally knows its bounds)
            finite = cloud[torch.isfinite(cloud).all(dim=1)]
            lo = finite.min(dim=0).values.cpu().numpy() if finite.numel() else np.zeros(3)
            hi = finite.max(dim=0).values.cpu().numpy() if finite.numel() else np.ones(3)
            origin = lo - 1e-9
            dims = np.maximum(1, np.ceil((hi - origin) / cell + 1e-9)).astype(int)
        self.origin = tuple(float(v) for v in origin); self.dims = tuple(int(v) for v in dims); self.cell = float(cell)
        cells = self.dims[0] * self.dims[1] * self.dims[2]
        dev = cloud.device
        self.points = torch.empty((max(P, 1), 3), dtype=torch.float64, device=dev)
        self.index = torch.empty((max(P, 1),), dtype=torch.int32, device=dev)
        self.start = torch.empty((cells + 1,), dtype=torch.int32, device=dev)
        scratch = torch.empty((cells,), dtype=torch.int32, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        _check(lib().frp_nmpc_cloud_grid_build(tensor_ptr(cloud) if P else None, P, (ctypes.c_double * 3)(*self.origin), self.cell,
                                               (ctypes.c_int * 3)(*self.dims), tensor_ptr(self.points), tensor_ptr(self.index), tensor_ptr(self.start),
                                               tensor_ptr(scratch), ctypes.c_void_p(s.cuda_stream)), "frp_nmpc_cloud_grid_build")
        s.synchronize()  # scratch may be freed


class SharedViewGrid:
    """The grid of a SharedView: CloudGrid's attributes (origin, dims, cell, points, index, start) over the view's persistent buffers.
    It describes view.cloud[:view.count] as of the last update()."""

    def __init__(self, origin, dims, cell, points, index, start):
        self.origin, self.dims, self.cell, self.points, self.index, self.start = origin, dims, cell, points, index, start


class SharedView:
    """The whole-map obstacle cloud of an OccupancyMap and its uniform grid, resident on the device (frp_nmpc_occmap_shared_view_update):
    cloud [cap,3] f64 whose first count[0] rows are local_view(None, cap).cloud[0, :n] to the bit, count / total [1] int32 (count =
    min(total, cap); total = the map's occupied voxels), grid = a SharedViewGrid laid over the map (origin = the map's, dims =
    ceil(map_size / cell)).  update() enqueues the rebuild -- five launches, no read-back, no allocation, capturable -- and the
    corridor takes the view with the grid ON:  corridor_batch_device(None, ..., view=view, cut=...) / DeviceFleet.corridor /
    full_tick(view=...).  Storage beyond count is never written and never read through the grid.
    cap > CORRIDOR_MAX_POINTS (up to CORRIDOR_LARGE_MAX_POINTS) makes a LARGE view (include/frp_nmpc_corridor_large.h): update() is
    frp_nmpc_occmap_shared_view_update_large, and the corridor entries route to frp_nmpc_corridor_batch_large.  Such a view owns what
    that call needs, allocated here once: the fallback's workspace for min(planners, CORRIDOR_LARGE_GROUPS) lists (256 KB each) and
    overflow, int32 [planners] -- after a corridor call of B <= planners planners overflow[:B] is 1 where a local box held more than
    CORRIDOR_LARGE_LIST points (that planner's result is the refusal marker: poly_count = INT_MIN, poly_nfaces = poly_index = 0) and 0
    elsewhere.  At or below CORRIDOR_MAX_POINTS nothing changes: overflow is None and the existing calls are used."""

    def __init__(self, occmap, cap=CORRIDOR_MAX_POINTS, cell=0.5, planners=4096):
        t = occmap.torch
        self.map, self.cap, self.cell = occmap, int(cap), float(cell)
        if not 1 <= self.cap <= CORRIDOR_LARGE_MAX_POINTS:
            raise ValueError(f"cap = {cap}: a shared cloud holds 1 .. FRP_CORRIDOR_LARGE_MAX_POINTS = {CORRIDOR_LARGE_MAX_POINTS} points")
        self.large = self.cap > CORRIDOR_MAX_POINTS
        self.planners = int(planners)
        if self.large and self.planners < 1:
            raise ValueError(f"planners = {planners}: a large view serves at least one planner")
        dims = (ctypes.c_int * 3)()
        m = occmap._map()
        if lib().frp_nmpc_occmap_shared_view_dims(ctypes.byref(m), self.cell, ctypes.byref(dims)) != 0:
            raise ValueError(f"cell = {cell}: not a positive finite size, or more than FRP_CORRIDOR_MAX_CELLS = {CORRIDOR_MAX_CELLS} cells over this map")
        self.dims = tuple(int(v) for v in dims)
        cells = self.dims[0] * self.dims[1] * self.dims[2]
        dev = occmap.device
        self.cloud = t.zeros((self.cap, 3), dtype=t.float64, device=dev)
        self.count = t.zeros((1,), dtype=t.int32, device=dev)
        self.total = t.zeros((1,), dtype=t.int32, device=dev)
        self.grid = SharedViewGrid(occmap.origin, self.dims, self.cell, t.zeros((self.cap, 3), dtype=t.float64, device=dev),
                                   t.zeros((self.cap,), dtype=t.int32, device=dev), t.zeros((cells + 1,), dtype=t.int32, device=dev))
        self._cursor = t.zeros((cells,), dtype=t.int32, device=dev)
        self._sums = t.zeros((OCCMAP_VIEW_MAX_GROUPS,), dtype=t.int32, device=dev)
        self.overflow = self._workspace = None
        if self.large:
            self._workspace = t.zeros((int(lib().frp_nmpc_corridor_large_workspace_bytes(self.planners)),), dtype=t.uint8, device=dev)
            self.overflow = t.zeros((self.planners,), dtype=t.int32, device=dev)

    def _large_args(self, B):
        """frp_nmpc_corridor_large for a corridor call of B planners through this (large) view."""
        if B > self.planners:
            raise ValueError(f"{B} planners through a large view made for planners = {self.planners}")
        return CorridorLarge(self._workspace.data_ptr(), self._workspace.numel(), self.overflow.data_ptr())

    def _args(self):
        g = self.grid
        return OccMapSharedView(self.cap, self.cell, (ctypes.c_int * 3)(*self.dims), self.cloud.data_ptr(), self.count.data_ptr(),
                                self.total.data_ptr(), g.points.data_ptr(), g.index.data_ptr(), g.start.data_ptr(),
                                self._cursor.data_ptr(), self._sums.data_ptr())

    def update(self, stream=None):
        """Rebuild cloud, count, total and grid from the map as it is on `stream` (torch's current stream when None).  Asynchronous."""
        v = self._args()
        self.map._call("frp_nmpc_occmap_shared_view_update_large" if self.large else "frp_nmpc_occmap_shared_view_update", ctypes.byref(v), stream=stream)

    def overflowed(self):
        """Device bool [1]: the map held more occupied voxels than cap at the last update (the first cap in x, y, z order were kept)."""
        return self.total > self.count
