#!/usr/bin/env python3
"""Multiprecision reference of the corridor where no obstacle lies inside a seed ellipsoid
-> tests/golden/corridor_mp.npz.

    python tests/tools/gen_corridor_mp.py [--jobs J] [--out FILE]

When no in-box cloud point lies inside the seed ellipsoid, find_ellipsoid leaves the seed as it is and the decomposition is a closed
geometric procedure.  This script evaluates it with mpmath at DPS digits FROM THE GEOMETRY -- it neither imports nor follows
oracle/corridor_oracle.py, and needs no rotation matrix, quaternion or 3x3 inverse.  Every float64 input is taken as an exact value.

  heading, centre   h = (cos yaw, sin yaw, 0), p2 = p1 + seed_len h, d = (p1 + p2) / 2, f = seed_len / 2, r = f / (f + offset_x)
  seed metric       the ellipsoid is axially symmetric about h: for w = q - d, t = w.h,  dist^2(q) = t^2 / f^2 + (|w|^2 - t^2) / (f r)^2
  local box         dir_h = (h_y, -h_x, 0), dir_v = h x dir_h; the six planes of line_segment.h:47-85 with half-widths bbox; a point is
                    in the box when its signed distance to every plane is <= 1e-10 (the double, taken exactly)
  precondition      no in-box point has dist <= 1; otherwise the planner is `undecided` from that stage on and nothing of it is compared
  polyhedron        (Liu et al.) among the remaining in-box points take the one with the smallest dist^2, cut with the plane through it
                    whose normal is the metric's gradient  n ~ h t / f^2 + (w - t h) / (f r)^2, drop every q with (q - p).n >= 0,
                    repeat until none is left; then the six box planes
  rows              (n, n.p), flipped so that n.d <= c
  selection         stage i reuses the last polytope iff every row has  a.ref_i - (b - inflation |E_i a|) <= 0, else decomposes there

Every discrete decision leaves a margin, in the units of the quantity compared: the pick (gap between the smallest and the second
smallest dist^2, relative), each keep/drop (|(q - p).n|), each box-membership test (distance of the deciding signed distance from
1e-10), the in-seed test (dist - 1) and each reuse test (the row value; for a refusal, the most violated row's).  A planner is
DECISIVE when all of them exceed corridor_mp_cases.MARGIN = 1e-7: rounding of these double expressions is ~1e-13 and the project's row
tolerance 1e-9, so nothing an implementation rounds differently can flip a decision of a decisive planner.

A float pre-filter discards, before any mp arithmetic, the points more than 1e-6 outside a box (their margin is 1e-6, beyond the
threshold).  The file holds DATA only; the clouds are not stored but regenerated from their seeds, with a SHA-256 of their bytes.  The
archive is written with fixed time stamps, so a second run reproduces the committed file bit for bit.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import corridor_mp_cases as CM          # noqa: E402
from tests.tools.gen_tube_mp import write_npz      # noqa: E402

DPS = 50
PREFILTER = 1e-6
BOX_EPS = 1e-10      # decomp_basis/data_type.h:129


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


class Margins:
    def __init__(self):
        self.m = {k: float("inf") for k in CM.MARGIN_KINDS}

    def see(self, kind, value):
        v = float(value)
        if v < self.m[kind]:
            self.m[kind] = v

    def row(self):
        return np.array([self.m[k] for k in CM.MARGIN_KINDS])


def decompose_mp(p1f, yawf, cloud, c, mg):
    """The decomposition seeded at p1 with heading yaw.  Returns the rows [(n, c)] in mp, or None when a point is inside the seed."""
    mp = _mp()
    F = mp.mpf
    p1 = [F(float(x)) for x in p1f]
    yaw = F(float(yawf))
    L, off = F(c["seed_len"]), F(c["offset_x"])
    bb = [F(x) for x in c["bbox"]]
    h = [mp.cos(yaw), mp.sin(yaw), F(0)]
    p2 = [p1[k] + L * h[k] for k in range(3)]
    d = [(p1[k] + p2[k]) / 2 for k in range(3)]
    f = L / 2
    r = f / (f + off)
    fa2, fb2 = f * f, (f * r) * (f * r)
    dh = [h[1], -h[0], F(0)]
    dv = [h[1] * dh[2] - h[2] * dh[1], h[2] * dh[0] - h[0] * dh[2], h[0] * dh[1] - h[1] * dh[0]]
    neg = lambda v: [-x for x in v]
    along = lambda p, v, s: [p[k] + v[k] * s for k in range(3)]
    box = [(along(p1, dh, bb[1]), dh), (along(p1, dh, -bb[1]), neg(dh)), (along(p2, h, bb[0]), h), (along(p1, h, -bb[0]), neg(h)),
           (along(p1, dv, bb[2]), dv), (along(p1, dv, -bb[2]), neg(dv))]
    # float pre-filter: a point whose float signed distance to some plane exceeds PREFILTER is outside (float error ~1e-15)
    sd = np.stack([(cloud - np.array([float(x) for x in pp])) @ np.array([float(x) for x in n]) for pp, n in box], 1)
    cand = np.nonzero(sd.max(axis=1) <= PREFILTER)[0]
    eps = F(BOX_EPS)
    pts = []        # (cloud index, q, dist^2, w, t)
    for idx in cand:
        q = [F(float(x)) for x in cloud[idx]]
        s = [_dot([q[k] - pp[k] for k in range(3)], n) for pp, n in box]
        worst = max(s)
        inside = worst <= eps
        mg.see("box", abs(worst - eps))       # all six must hold, so the largest decides either way
        if not inside:
            continue
        w = [q[k] - d[k] for k in range(3)]
        t = _dot(w, h)
        d2 = t * t / fa2 + (_dot(w, w) - t * t) / fb2
        pts.append((int(idx), q, d2, w, t))
    if pts:
        dmin = mp.sqrt(min(p[2] for p in pts))
        mg.see("in_seed", abs(dmin - 1))
        if dmin <= 1:
            return None
    planes = []
    remain = pts
    while remain:
        order = sorted(range(len(remain)), key=lambda j: remain[j][2])
        best = remain[order[0]]
        if len(order) > 1:
            mg.see("pick", (remain[order[1]][2] - best[2]) / best[2])
        _, p, _, w, t = best
        g = [h[k] * t / fa2 + (w[k] - t * h[k]) / fb2 for k in range(3)]
        gn = mp.sqrt(_dot(g, g))
        n = [x / gn for x in g]
        planes.append((p, n))
        keep = []
        for it in remain:
            if it is best:
                continue
            s = _dot([it[1][k] - p[k] for k in range(3)], n)
            mg.see("keep_drop", abs(s))
            if s < 0:
                keep.append(it)
        remain = keep
    rows = []
    for p, n in planes + box:
        cc = _dot(n, p)
        if _dot(n, d) - cc > 0:
            n, cc = neg(n), -cc
        rows.append((n, cc))
    return rows


def planner_mp(ref, yaw, E, cloud, c):
    """One planner.  Returns (poly_index [N], polytopes as float64 [m,4] arrays, margins [5], undecided)."""
    mp = _mp()
    F = mp.mpf
    mg = Margins()
    infl = F(c["inflation"])
    polys, index = [], []
    for i in range(len(ref)):
        reuse = False
        if polys:
            x = [F(float(v)) for v in ref[i]]
            Ei = [[F(float(E[i][a][b])) for b in range(3)] for a in range(3)]
            vals = []
            for n, cc in polys[-1]:
                Ea = [_dot(Ei[a], n) for a in range(3)]
                vals.append(_dot(n, x) - (cc - infl * mp.sqrt(_dot(Ea, Ea))))
            reuse = all(v <= 0 for v in vals)
            mg.see("reuse", min(abs(v) for v in vals) if reuse else max(vals))
        if not reuse:
            rows = decompose_mp(ref[i], yaw[i], cloud, c, mg)
            if rows is None:
                return np.zeros(len(ref), dtype=np.int32), [], mg.row(), True
            polys.append(rows)
        index.append(len(polys) - 1)
    out = [np.array([[float(n[0]), float(n[1]), float(n[2]), float(cc)] for n, cc in rows]) for rows in polys]
    return np.array(index, dtype=np.int32), out, mg.row(), False


def run_job(job):
    name, p = job
    off, sl, rot, tunnel, seed, P = CM.CASES[name]
    cloud, ref, yaw, E, cs = CM.world(seed, P=P, tunnel=tunnel, rot_deg=rot)
    return planner_mp(ref[p], yaw[p], E[p], cloud, CM.consts_of(name))


def main(argv):
    import multiprocessing as mpc
    jobs, out = 8, CM.FIXTURE
    for i, a in enumerate(argv):
        if a == "--jobs":
            jobs = int(argv[i + 1])
        if a == "--out":
            out = argv[i + 1]
    names = list(CM.CASES)
    work = [(n, p) for n in names for p in range(CM.B)]
    with mpc.Pool(min(jobs, len(work))) as pool:
        res = pool.map(run_job, work, chunksize=1)
    C, B, N = len(names), CM.B, CM.N
    arr = dict(case_name=np.array(names), const_keys=np.array(CM.CONST_KEYS), margin_kinds=np.array(CM.MARGIN_KINDS),
               dps=np.array(DPS, dtype=np.int32), margin_threshold=np.array(CM.MARGIN),
               consts=np.zeros((C, len(CM.CONST_KEYS))), seed=np.zeros(C, dtype=np.int64), P=np.zeros(C, dtype=np.int64), tunnel=np.zeros(C),
               rot_deg=np.zeros(C), rot_cs=np.zeros((C, 2)), ref=np.zeros((C, B, N, 3)), yaw=np.zeros((C, B, N)), E=np.zeros((C, B, N, 3, 3)),
               cloud_len=np.zeros(C, dtype=np.int64), poly_index=np.zeros((C, B, N), dtype=np.int32), poly_count=np.zeros((C, B), dtype=np.int32),
               nfaces=np.zeros((C, B, N), dtype=np.int32), row_start=np.zeros((C, B, N), dtype=np.int64), decisive=np.zeros((C, B), dtype=bool),
               undecided=np.zeros((C, B), dtype=bool), margins=np.zeros((C, B, len(CM.MARGIN_KINDS))), min_margin=np.zeros(C))
    sha, rows, at, ok = [], [], 0, True
    for k, name in enumerate(names):
        off, sl, rot, tunnel, seed, P = CM.CASES[name]
        cloud, ref, yaw, E, cs = CM.world(seed, P=P, tunnel=tunnel, rot_deg=rot)
        arr["consts"][k] = CM.consts_row(CM.consts_of(name))
        arr["seed"][k], arr["P"][k], arr["tunnel"][k], arr["rot_deg"][k], arr["rot_cs"][k] = seed, P, tunnel, rot, cs
        arr["ref"][k], arr["yaw"][k], arr["E"][k], arr["cloud_len"][k] = ref, yaw, E, len(cloud)
        sha.append(CM.cloud_sha256(cloud))
        for p in range(B):
            index, polys, margins, undecided = res[k * B + p]
            arr["poly_index"][k, p], arr["poly_count"][k, p] = index, len(polys)
            arr["margins"][k, p], arr["undecided"][k, p] = margins, undecided
            arr["decisive"][k, p] = (not undecided) and bool((margins > CM.MARGIN).all())
            for j, R in enumerate(polys):
                arr["nfaces"][k, p, j], arr["row_start"][k, p, j] = len(R), at
                rows.append(R); at += len(R)
        arr["min_margin"][k] = arr["margins"][k].min()
        weak = int((~arr["decisive"][k]).sum())
        cap = 0 if name.startswith("a_") else 1
        ok &= weak <= cap
        print(f"{name}: cloud {len(cloud)}, polytopes {arr['poly_count'][k].tolist()}, decisive {arr['decisive'][k].tolist()}, undecided "
              f"{arr['undecided'][k].tolist()}, smallest margin {arr['min_margin'][k]:.3g} "
              f"({', '.join(f'{n} {v:.3g}' for n, v in zip(CM.MARGIN_KINDS, arr['margins'][k].min(axis=0)))})" + ("" if weak <= cap else "  <-- CAP EXCEEDED"))
    arr["cloud_sha256"] = np.array(sha)
    arr["rows"] = np.concatenate(rows) if rows else np.zeros((0, 4))
    if not ok:
        raise SystemExit("a case has more non-decisive or undecided planners than its cap allows: change that case's seed")
    write_npz(out, arr)
    print(f"{out}: {C} cases, {len(arr['rows'])} rows, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
