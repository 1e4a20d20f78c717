"""The depth-image renderer of the device occupancy map (include/frp_nmpc_occmap_render.h), written down: what a camera at a given pose
sees of a given map, pixel by pixel.  Plain Python floats (IEEE doubles), one statement per operation, serial, built on
tests/occmap_oracle.py.  tests/test_gpu_occmap_render.py compares frp_nmpc_occmap_render_depth against it to the bit.

The reference has NO counterpart: it takes its depth images from a simulator outside its tree.  This file is therefore the
SPECIFICATION of the renderer, not a restatement -- the kernel follows the operation order below.  What it shares with the
reference is the camera model of projectDepthImage (occ_grid/src/occ_map.cpp:337-340) and posToIndex (:71-75), so that an image
rendered here and handed to FusionOracle.project lands back in the voxels it came from.

A pixel (u, v):
    d_cam = ((u - cx) / fx, (v - cy) / fy, 1)
    d_w[i] = (R[i][0] * d_cam[0] + R[i][1] * d_cam[1]) + R[i][2]
    the ray t + s * d_w: s is the camera-z depth
is walked cell by cell from the camera's cell (posToIndex of t, clamped to +-2^30 like every index of section (8)) by an exact slab
traversal: per axis k with d_w[k] != 0, s_next[k] = (the next cell face along k - t[k]) / d_w[k] and s_step[k] = resolution / |d_w[k]|;
an axis with d_w[k] == 0 has s_next[k] = +inf and is never chosen (no 0 / 0 anywhere).  A step takes the axis of the smallest s_next
(the comparison tree of RayCaster::step: x before y before z only on strict inequality) and enters the next cell at s_in = that
s_next.  The walk ends
    * without a return when not (s_in * |d_w| <= max_range) -- a NaN ends it too --, or after step_bound() steps;
    * with a return in the first occupied cell inside the map: s_out = the smallest s_next after the step,
      s_mid = (s_in + s_out) / 2, pixel = floor(s_mid * depth_scale + 0.5), kept when 1 <= pixel <= 65535.
A cell outside the map is free; a camera whose own cell is occupied sees nothing.
"""
import math

import numpy as np

from tests.occmap_oracle import _to_int

INF = float("inf")
REFUSED = -256                                                                                        # FRP_OCCMAP_FUSE_REFUSED
MIN_SEGMENT = 0.002                                                                                   # the round-trip tests' 2 mm rule


def step_bound(max_range, resolution):
    return 3 * (int(math.ceil(float(max_range) / float(resolution))) + 2)


class RenderOracle:
    """occ: [gx, gy, gz] array, non-zero = occupied (OccMapOracle.occ() or a world's occ).  origin, resolution: the map's."""

    def __init__(self, occ, origin, resolution):
        self.occ = np.asarray(occ) != 0
        self.g = [int(v) for v in self.occ.shape]
        self.o = [float(v) for v in origin]
        self.res = float(np.float64(resolution))
        self.res_inv = float(np.float64(1) / np.float64(resolution))                                  # resolution_inv_, occ_map.cpp:787

    def _occupied(self, c):
        for k in range(3):
            if c[k] < 0 or c[k] >= self.g[k]:
                return False
        return bool(self.occ[c[0], c[1], c[2]])

    def pixel(self, u, v, K, R, t, max_range, depth_scale, nb):
        """(pixel value, linear voxel index or -1, s_out - s_in of the return or 0.0, cells entered)."""
        dcx = (float(u) - K[2]) / K[0]
        dcy = (float(v) - K[5]) / K[4]
        d = [(R[i][0] * dcx + R[i][1] * dcy) + R[i][2] for i in range(3)]
        length = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        c, step, s_next, s_step = [0] * 3, [0] * 3, [INF] * 3, [INF] * 3
        for k in range(3):
            f = (t[k] - self.o[k]) * self.res_inv
            c[k] = _to_int(float(math.floor(f)) if math.isfinite(f) else f)                           # posToIndex
            if d[k] > 0.0:
                step[k] = 1
                face = self.o[k] + float(c[k] + 1) * self.res
            elif d[k] < 0.0:
                step[k] = -1
                face = self.o[k] + float(c[k]) * self.res
            else:
                continue
            s_next[k] = (face - t[k]) / d[k]
            s_step[k] = self.res / abs(d[k])
        if self._occupied(c):
            return 0, -1, 0.0, 0

        def axis():
            if s_next[0] < s_next[1]:
                return 0 if s_next[0] < s_next[2] else 2
            return 1 if s_next[1] < s_next[2] else 2

        for n in range(nb):
            a = axis()
            s_in = s_next[a]
            if not (s_in * length <= max_range):
                return 0, -1, 0.0, n
            c[a] += step[a]
            s_next[a] = s_next[a] + s_step[a]
            if self._occupied(c):
                s_out = s_next[axis()]
                s_mid = (s_in + s_out) / 2.0
                pix = s_mid * depth_scale + 0.5
                pix = float(math.floor(pix)) if math.isfinite(pix) else pix
                if pix >= 1.0 and pix <= 65535.0:
                    return int(pix), (c[0] * self.g[1] + c[1]) * self.g[2] + c[2], s_out - s_in, n + 1
                return 0, -1, 0.0, n + 1
        return 0, -1, 0.0, nb

    def render(self, T_wc, K, rows, cols, max_range, depth_scale=1000.0):
        """One frame: (depth [rows, cols] uint16, voxel [rows, cols] int32, segment [rows, cols] float64 -- the depth the ray spends
        inside the voxel of the return --, status [2], cells entered in all).  A non-finite T_wc: the zero image, REFUSED."""
        T = [float(v) for v in np.asarray(T_wc, dtype=np.float64).reshape(16)]
        K = [float(v) for v in np.asarray(K, dtype=np.float64).reshape(9)]
        depth = np.zeros((rows, cols), dtype=np.uint16)
        voxel = np.full((rows, cols), -1, dtype=np.int32)
        seg = np.zeros((rows, cols), dtype=np.float64)
        if not all(math.isfinite(v) for v in T):
            return depth, voxel, seg, [REFUSED, 0], 0
        R = [[T[4 * i + j] for j in range(3)] for i in range(3)]
        t = [T[4 * i + 3] for i in range(3)]
        nb = step_bound(max_range, self.res)
        returns = steps = 0
        for v in range(rows):
            for u in range(cols):
                pix, vox, s, n = self.pixel(u, v, K, R, t, float(max_range), float(depth_scale), nb)
                depth[v, u], voxel[v, u], seg[v, u] = pix, vox, s
                returns += 1 if pix != 0 else 0
                steps += n
        return depth, voxel, seg, [1, returns], steps


def camera_poses(state, T_bc):
    """T_wc[b] = T_wb(state[b]) * T_bc, the numpy statement of frp_nmpc_occmap_camera_poses: state [B, 9] = position, velocity,
    Euler angles (roll, pitch, yaw); T_wb = [R p; 0 0 0 1] with R = Rz(yaw) Ry(pitch) Rx(roll) in the operation order of
    workloads._rot; every entry of the product is ((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3.  This is depthOdomCallback's
    arithmetic (occ_map.cpp:218-290) with Euler angles where the reference has a quaternion."""
    st = np.asarray(state, dtype=np.float64).reshape(-1, 9)
    Tb = np.asarray(T_bc, dtype=np.float64).reshape(4, 4)
    r, p, y = st[:, 6], st[:, 7], st[:, 8]
    sr, cr, sp, cp, sy, cy = np.sin(r), np.cos(r), np.sin(p), np.cos(p), np.sin(y), np.cos(y)
    A = np.zeros((len(st), 4, 4))
    A[:, 0, 0] = cy * cp; A[:, 0, 1] = cy * sp * sr - cr * sy; A[:, 0, 2] = cy * sp * cr + sy * sr
    A[:, 1, 0] = cp * sy; A[:, 1, 1] = cy * cr + sy * sp * sr; A[:, 1, 2] = sy * sp * cr - cy * sr
    A[:, 2, 0] = -sp;     A[:, 2, 1] = cp * sr;                A[:, 2, 2] = cp * cr
    A[:, :3, 3] = st[:, 0:3]
    A[:, 3, 3] = 1.0
    out = np.empty((len(st), 4, 4))
    for i in range(4):
        for j in range(4):
            out[:, i, j] = ((A[:, i, 0] * Tb[0, j] + A[:, i, 1] * Tb[1, j]) + A[:, i, 2] * Tb[2, j]) + A[:, i, 3] * Tb[3, j]
    return out
