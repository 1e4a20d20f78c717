"""The point-scan renderer of the device occupancy map (include/frp_nmpc_occmap_render_scan.h), written down: what a range sensor at
a given pose measures of a given map along a table of beam directions, beam by beam.  Plain Python floats (IEEE doubles), one
statement per operation, serial.  tests/test_gpu_occmap_scan.py compares frp_nmpc_occmap_render_scan_batch against it to the bit.

The reference has NO counterpart, as for the depth renderer: this file is the SPECIFICATION, and the kernel follows the operation
order below.  It is tests/occmap_render_oracle.py with the ray and the output changed; tests/test_occmap_scan_cpu.py pins the two to
each other through a table of pinhole directions.

A beam b (sensor frame) of a sensor with rotation R and translation t:
    d_w[i] = (R[i][0] * b[0] + R[i][1] * b[1]) + R[i][2] * b[2]
    length = sqrt((d0 * d0 + d1 * d1) + d2 * d2)
    the ray t + s * d_w: s * length is the distance along the beam in metres
A beam with a non-finite component, or whose length is 0 or not finite, is not fired: its point is NaN whatever far_range is.
The walk is RenderOracle.pixel's: from the sensor's cell (posToIndex of t), per axis k with d_w[k] != 0 the next face crossing
s_next[k] = (face - t[k]) / d_w[k] and the spacing resolution / |d_w[k]|; an axis with d_w[k] == 0 is never chosen.  A step takes the
axis of the smallest s_next (the comparison tree of RayCaster::step) and enters the next cell at s_in.  The walk ends
    * without a return when not (s_in * length <= max_range), or after step_bound() steps, or at once for a sensor whose own cell is
      occupied;
    * in the first occupied cell inside the map: s_out = the smallest s_next after the step, s_mid = (s_in + s_out) / 2,
      rng = s_mid * length; rng < min_range: no return (the walk does not go on behind the hit); otherwise
      point[i] = t[i] + s_mid * d_w[i].
A fired beam without a return: the NaN point with far_range == 0, otherwise s_far = far_range / length and
point[i] = t[i] + s_far * d_w[i]; range 0 and voxel -1 either way.  status[1] counts returns only.
"""
import math

import numpy as np

from tests.occmap_oracle import _to_int
from tests.occmap_render_oracle import REFUSED, RenderOracle, step_bound

INF = float("inf")
NAN = float("nan")


class ScanOracle(RenderOracle):
    """occ, origin, resolution: as RenderOracle."""

    def beam(self, b, R, t, min_range, max_range, far_range, nb):
        """((x, y, z), range, linear voxel index or -1, s_mid of the return or None, cells entered)."""
        none = (NAN, NAN, NAN)
        d = [(R[i][0] * b[0] + R[i][1] * b[1]) + R[i][2] * b[2] for i in range(3)]
        s2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        length = math.sqrt(s2) if s2 >= 0.0 else NAN
        if not all(math.isfinite(v) for v in b) or not (length > 0.0) or not math.isfinite(length):
            return none, 0.0, -1, None, 0

        def far(n):
            if far_range > 0.0:
                s_far = far_range / length
                return tuple(t[i] + s_far * d[i] for i in range(3)), 0.0, -1, None, n
            return none, 0.0, -1, None, n

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
            return far(0)

        def axis():
            if s_next[0] < s_next[1]:
                return 0 if s_next[0] < s_next[2] else 2
            return 1 if s_next[1] < s_next[2] else 2

        for n in range(nb):
            a = axis()
            s_in = s_next[a]
            if not (s_in * length <= max_range):
                return far(n)
            c[a] += step[a]
            s_next[a] = s_next[a] + s_step[a]
            if self._occupied(c):
                s_out = s_next[axis()]
                s_mid = (s_in + s_out) / 2.0
                rng = s_mid * length
                if rng < min_range:
                    return far(n + 1)
                return tuple(t[i] + s_mid * d[i] for i in range(3)), rng, (c[0] * self.g[1] + c[1]) * self.g[2] + c[2], s_mid, n + 1
        return far(nb)

    def scan(self, T_ws, beams, max_range, min_range=0.0, far_range=0.0):
        """One scan: dict(points [P, 3] float64, range [P] float64, voxel [P] int32, s_mid [P] float64 (NaN where no return),
        origin [3], count, status [2], steps).  A non-finite T_ws: all NaN points, count 0, REFUSED, origin as it stands."""
        T = [float(v) for v in np.asarray(T_ws, dtype=np.float64).reshape(16)]
        B = np.asarray(beams, dtype=np.float64).reshape(-1, 3)
        P = len(B)
        out = dict(points=np.full((P, 3), NAN), range=np.zeros(P), voxel=np.full(P, -1, dtype=np.int32), s_mid=np.full(P, NAN),
                   origin=np.array([T[3], T[7], T[11]]), count=0, status=[REFUSED, 0], steps=0)
        if not all(math.isfinite(v) for v in T):
            return out
        R = [[T[4 * i + j] for j in range(3)] for i in range(3)]
        t = [T[4 * i + 3] for i in range(3)]
        nb = step_bound(max_range, self.res)
        returns = 0
        for p in range(P):
            pt, rng, vox, s_mid, n = self.beam([float(v) for v in B[p]], R, t, float(min_range), float(max_range), float(far_range), nb)
            out["points"][p], out["range"][p], out["voxel"][p] = pt, rng, vox
            if s_mid is not None:
                out["s_mid"][p] = s_mid
                returns += 1
            out["steps"] += n
        out["count"], out["status"] = P, [1, returns]
        return out
