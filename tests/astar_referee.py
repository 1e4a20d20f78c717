"""A referee for kinodynamic-A* results, written from the mathematics of the planner -- plain Python, exact rational arithmetic where a
value is judged, NO import of the oracle or of the kernel's host code.  It is applied on the CPU to the oracle's results
(tests/test_astar_paths_cpu.py) and on the GPU to the device's own path_nodes / kino_path (tests/test_gpu_astar_paths.py): what both
sides share by transcription -- a sign in the transit, a primitive off the grid, a collision sample that was not looked at -- does
not show when the two are compared with each other, and does here.

What a result must satisfy (check() raises AssertionError otherwise), u = 2^-53:

DYNAMICS.  Node q >= 1 is the double integrator's state after `duration[q]` under the constant acceleration input[q] + f_ext from
  node q - 1:  p = p0 + v0 tau + (u_ + f)(tau^2 / 2),  v = v0 + (u_ + f) tau, evaluated here in fractions.Fraction of the doubles.
  The implementations form ud = fl(u_ + f), t2 = fl(tau tau), fl(tau v0), fl(p0 + .), fl((t2 / 2) ud), fl(. + .): SIX roundings for a
  position.  The two that feed a product (ud, t2) pass on a relative error u of that product, < 1 ulp of it each; the other four
  are at most half an ulp of their own result.  With L = the largest of |p0|, |v0 tau|, |(u_ + f) tau^2 / 2|, |p0 + v0 tau|, |p|:
  error < 2 + 4 / 2 = 4 ulp(L).  A velocity has three roundings (ud, fl(tau ud), the sum): < 1 + 1/2 + 1/2 ulp; the same 4 ulp of its
  largest term is asserted.
PRIMITIVE SET.  input[q] is on the grid {-a, -a/2, 0, a/2, a}^3 and duration[q] == max_tau; except node 1 of a search that started
  continuous (init) and was not repeated: input == start_acc, duration one of the eight k init_max_tau / 8 (by repeated addition).
BOUNDS.  Nodes q >= 1: |v_i| <= max_vel, origin < p < map_size / 2 in x, y and 0.1 < p_z < map_size_z / 2, all strict.
COLLISION (a necessary condition; only for worlds whose origin is a multiple of the resolution -- otherwise the ray cells of
  checkState are half a voxel off the map's voxels).  At each of the check_num sample times k duration / check_num of every
  primitive on the path, the voxels under both ends of the horizontal arm (+-1.5 ego_r across the horizontal velocity, across (1, 1)
  below 1e-4 m/s) and of the vertical arm (+-1.5 ego_h) are inside the map, and free or outside the planner's local box.  Positions in
  Fraction; an end within 1e-9 voxel of a voxel face is not judged.
SAMPLES.  Consecutive samples of kino_path are at most  sqrt(3) max_vel Ts + (sqrt(3) max_acc + |f_ext|) Ts^2 / 2  apart (node
  velocities are bounded by max_vel, accelerations by the grid), and kino_path[0] is the start to within that same step: the
  reference samples a primitive
  BACKWARDS from its end in steps of Ts down to t >= -1e-5, so the first sample sits at the remainder of duration / Ts, which is not 0
  for six of the eight continuous-start durations.  When the first duration is a multiple of Ts, kino_path[0] is the start to
  1e-5 (sqrt(3) max_vel + 1) m.
SHOT (where coef_shot / t_shot are visible: the oracle).  p(t) = c0 + c1 t + c2 t^2 + c3 t^3 per axis, evaluated in Fraction: p(0),
  p'(0) are the last node's position and velocity exactly (c0, c1 are copies), p(T) = end_pt, p'(T) = end_vel.  Rounding, with
  e = dp - v0 T, E = |dp| + |v0| T, dv = v1 - v0: fl(e) carries 2uE.  c3 = fl(1/6) (fl(-12 / T^3) e + fl(6 / T^2) dv): T^3 two
  roundings, the quotient one, the product one -> (12 / T^3) 6uE; second term four roundings -> (6 / T^2) 4u |dv|; the sum one, the
  constant 1/6 and its product two -> |dc3| T^3 <= 18uE + 7u |dv| T.  c2 = (fl(6 / T^2) e - fl(2 / T) dv) / 2 -> |dc2| T^2 <= 18uE + 4u |dv| T.
  Position at T: 36uE + 11u |dv| T <= 47 u M, M = |p0| + |dp| + (|v0| + |v1|) T, and u M < ulp(M): 47 roundings' worth, asserted at
  64 ulp(M).  Velocity at T: 3 |dc3| T^2 + 2 |dc2| T <= 119 u M / T: asserted at 128 ulp(M / T) (the derived count exceeds 64).
"""
import math
from fractions import Fraction as Fr

import numpy as np

STATUS_NO_PATH = 3
FACE_EPS = Fr(1, 10 ** 9)


def _ulp(x):
    return math.ulp(float(abs(x))) if x != 0 else math.ulp(0.0)


def origin_on_the_voxel_grid(world):
    """True when every origin coordinate is a whole number of voxels (to 1e-9 voxel): the worlds the collision check applies to."""
    return all(abs(o / world["resolution"] - round(o / world["resolution"])) < 1e-9 for o in world["origin"])


def _transit(s0, um, f, tau):
    """Exact state after tau from s0 (Fractions of doubles): ([p], [v], largest terms per axis for p and v)."""
    p, v, Lp, Lv = [], [], [], []
    t = Fr(tau)
    for i in range(3):
        p0, v0, a = Fr(s0[i]), Fr(s0[3 + i]), Fr(um[i]) + Fr(f[i])
        pi = p0 + v0 * t + a * t * t / 2
        vi = v0 + a * t
        p.append(pi); v.append(vi)
        Lp.append(max(abs(p0), abs(v0 * t), abs(a * t * t / 2), abs(p0 + v0 * t), abs(pi)))
        Lv.append(max(abs(v0), abs(a * t), abs(vi)))
    return p, v, Lp, Lv


def _voxel(world, e):
    """Voxel index of the exact point e per axis, or None when e is within FACE_EPS voxels of a face."""
    idx = []
    for i in range(3):
        c = (e[i] - Fr(world["origin"][i])) / Fr(world["resolution"])
        fl = math.floor(c)
        if c - fl < FACE_EPS or fl + 1 - c < FACE_EPS:
            return None
        idx.append(fl)
    return idx


def _free(world, idx, box):
    occ = world["occ"]
    assert all(0 <= idx[i] < occ.shape[i] for i in range(3)), ("arm end outside the map", idx)
    if box is not None and not all(box[i] <= idx[i] <= box[3 + i] for i in range(3)):
        return True
    return occ[idx[0], idx[1], idx[2]] == 0


def init_durations(world):
    out, step = [], 0.125 * world["init_max_tau"]
    tau = step
    while tau <= world["init_max_tau"]:
        out.append(tau); tau += step
    return out


def step_bound(world, f, Ts):
    return math.sqrt(3.0) * world["max_vel"] * Ts + 0.5 * (math.sqrt(3.0) * world["max_acc"] + float(np.linalg.norm(f))) * Ts * Ts


def check(world, start_pt, start_v, start_a, end_pt, end_v, f_ext, init, retried, status, nodes, kino, Ts=0.05, local_box=None,
          shot=None):
    """nodes [n,10+]: state 6, input 3, duration per path node; kino [m,3]: the stored samples (the first m of the path);
    shot: None or (coef [3][4] by power of t, t_shot).  Returns a dict of counters (what was actually judged)."""
    seen = dict(nodes=0, collision_ends=0, samples=0, shot=0)
    if status == STATUS_NO_PATH:
        return seen
    n = len(nodes)
    assert n >= 1
    f = [float(x) for x in f_ext]
    a = world["max_acc"]
    grid = [k * (a * 0.5) for k in (-2, -1, 0, 1, 2)]
    assert np.array_equal(nodes[0][0:3], np.asarray(start_pt, dtype=float)) and np.array_equal(nodes[0][3:6], np.asarray(start_v, dtype=float))
    collide = origin_on_the_voxel_grid(world)
    for q in range(1, n):
        s0, s1, um, tau = nodes[q - 1][0:6], nodes[q][0:6], nodes[q][6:9], float(nodes[q][9])
        # primitive set
        if q == 1 and init and not retried:
            assert np.array_equal(um, np.asarray(start_a, dtype=float)) and tau in init_durations(world), (q, um, tau)
        else:
            assert all(float(x) in grid for x in um) and tau == world["max_tau"], (q, um, tau)
        # dynamics
        p, v, Lp, Lv = _transit(s0, um, f, tau)
        for i in range(3):
            assert abs(Fr(float(s1[i])) - p[i]) <= 4 * Fr(_ulp(Lp[i])), ("position", q, i, float(s1[i]), float(p[i]))
            assert abs(Fr(float(s1[3 + i])) - v[i]) <= 4 * Fr(_ulp(Lv[i])), ("velocity", q, i, float(s1[3 + i]), float(v[i]))
        # bounds
        assert all(abs(float(s1[3 + i])) <= world["max_vel"] for i in range(3)), ("max_vel", q)
        assert world["origin"][0] < s1[0] < world["map_size"][0] * 0.5 and world["origin"][1] < s1[1] < world["map_size"][1] * 0.5 and \
            0.1 < s1[2] < world["map_size"][2] * 0.5, ("range", q, s1[0:3])
        seen["nodes"] += 1
        # collision: both ends of both arms at every sample time
        if collide:
            for k in range(1, world["check_num"] + 1):
                pk, vk, _, _ = _transit(s0, um, f, Fr(tau) * k / world["check_num"])
                vx, vy = float(vk[0]), float(vk[1])
                if math.hypot(vx, vy) < 1e-4:
                    vx, vy = 1.0, 1.0
                nn = math.hypot(vx, vy)
                cw = (Fr(vy / nn * world["ego_r"] * 1.5), Fr(-vx / nn * world["ego_r"] * 1.5))
                h = Fr(world["ego_h"] * 1.5)
                ends = [(pk[0] + cw[0], pk[1] + cw[1], pk[2]), (pk[0] - cw[0], pk[1] - cw[1], pk[2]), (pk[0], pk[1], pk[2] + h), (pk[0], pk[1], pk[2] - h)]
                for e in ends:
                    idx = _voxel(world, e)
                    if idx is None:
                        continue
                    assert _free(world, idx, local_box), ("occupied arm end", q, k, idx)
                    seen["collision_ends"] += 1
    # samples
    m = len(kino)
    assert m >= 1
    bound = step_bound(world, f, Ts)
    d0 = float(np.linalg.norm(kino[0] - np.asarray(start_pt, dtype=float)))
    assert d0 <= bound, ("first sample", d0, bound)
    if n >= 2:
        r = float(nodes[1][9]) / Ts
        if abs(r - round(r)) < 1e-9:
            assert d0 <= 1e-5 * (math.sqrt(3.0) * world["max_vel"] + 1.0), ("first sample is the start", d0)
    if m >= 2:
        step = np.linalg.norm(np.diff(kino, axis=0), axis=1)
        assert float(step.max()) <= bound * (1.0 + 1e-12), ("sample step", int(step.argmax()), float(step.max()), bound)
    seen["samples"] = m
    # shot
    if shot is not None:
        coef, T = shot
        last = nodes[n - 1]
        for i in range(3):
            c = [Fr(float(coef[i][j])) for j in range(4)]
            t = Fr(float(T))
            p0, v0, p1, v1 = float(last[i]), float(last[3 + i]), float(end_pt[i]), float(end_v[i])
            assert c[0] == Fr(p0) and c[1] == Fr(v0), ("shot start", i)
            M = abs(p0) + abs(p1 - p0) + (abs(v0) + abs(v1)) * float(T)
            pT = c[0] + c[1] * t + c[2] * t * t + c[3] * t * t * t
            vT = c[1] + 2 * c[2] * t + 3 * c[3] * t * t
            assert abs(pT - Fr(p1)) <= 64 * Fr(_ulp(M)), ("shot end position", i, float(pT), p1)
            assert abs(vT - Fr(v1)) <= 128 * Fr(_ulp(M / float(T))), ("shot end velocity", i, float(vT), v1)
        seen["shot"] = 1
    return seen
