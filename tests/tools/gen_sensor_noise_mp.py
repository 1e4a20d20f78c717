#!/usr/bin/env python3
"""Multiprecision reference of the sensor noise (include/frp_nmpc.h section 16) -> tests/golden/sensor_noise_mp.npz.

    python tests/tools/gen_sensor_noise_mp.py [--out FILE]

Written from the header's statement of the scheme; tests/sensor_noise_oracle.py is imported for ONE purpose, at the end of each channel: to
measure its error against what is computed here (`*_tol_case`).  Every float64 input is taken as an exact value.

WHAT IS EVALUATED, for the case set of tests/sensor_noise_cases.py, in DPS = 50 digits with mpmath and NOTHING rounded on the way:
  * The generator's integers, restated here with % and // (the oracle masks and shifts): the sample keys with their tags, the words of every
    normal and uniform; u1, u2 and u are exact doubles; n = sqrt(-2 ln u1) cos(tp u2) with tp the double 6.283185307179586.
  * States: bias <- a bias + c n_i, meas = x + bias + sigma n for the finite components, the others as they are.  Stored as (hi, lo) pairs of
    doubles: states_meas [B][S][9][2], states_bias [B][3][2] (after the call); states_tick [B] uint64 (mod 2^64).
  * Depth: v = pix + depth_scale (sigma0 + sigma2 z z) n with z = pix / depth_scale, the pixel floor(v + 1/2) where that lies in 1 ... 65535 and
    0 elsewhere; u < p_drop is a comparison of exact doubles.  depth_out [DEPTH_CALLS][F][rows][cols] uint16: the images after each of two
    calls (the inactive frame as it was).  depth_margin: the smallest distance of a kept pixel's v + 1/2 from an integer, depth_u_margin: the
    smallest |u - p_drop| -- the GPU test may demand equal images because these are far above any rounding error.
  * Scan: d = p - o, r = sqrt(d.d), p' = o + d (1 + (sigma0 + sigma1 r) n / r); scan_out [S][P][3][2] as pairs, NaN where the oracle's scheme
    leaves or writes a NaN (lo = 0 there, and for infinities); scan_u_margin as above.
  * states_tol_case [B], scan_tol_case [S]: the largest absolute error of tests/sensor_noise_oracle.py over a case's finite values against
    these, and never below 2^-52 times the largest magnitude among them and 1 (gen_disturbance_mp.py's rule).
    tests/test_gpu_sensor_noise.py allows the device tol_factor = 8 times that.
DATA only, fixed time stamps: a second run reproduces the file bit for bit.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.tools.gen_tube_mp import write_npz      # noqa: E402
from tests.tools.gen_disturbance_mp import finalise, M64  # noqa: E402
from tests import sensor_noise_cases as NC         # noqa: E402

DPS = 50
OUT = os.path.join(ROOT, "tests", "golden", "sensor_noise_mp.npz")
TOL_FACTOR = 8.0
TAGS = dict(state=1398030676, depth=1145393236, scan=1396916558)      # "STAT", "DEPT", "SCAN" as big-endian ASCII


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


def key(seed, ident, k, tag):
    return finalise((finalise((finalise((finalise(seed % M64) + ident % M64) % M64) + k % M64) % M64) + tag) % M64)


def normal_mp(h, j):
    mp = _mp()
    r0, r1 = finalise((h + 2 * j) % M64), finalise((h + 2 * j + 1) % M64)
    u1 = mp.mpf(r0 // 2048 + 1) / mp.mpf(2) ** 53
    u2 = mp.mpf(r1 // 2048) / mp.mpf(2) ** 53
    return mp.sqrt(-2 * mp.log(u1)) * mp.cos(mp.mpf(6.283185307179586) * u2)


def uniform_exact(h, j):
    return float(finalise((h + j) % M64) // 2048) / 2.0 ** 53             # exact: 53 bits over a power of two


def split(x):
    if not isinstance(x, _mp().mpf):
        return float(x), 0.0
    if not _mp().isfinite(x):
        return float(x), 0.0
    hi = float(x)
    return hi, float(x - _mp().mpf(hi))


def tol(pairs):
    """max(|oracle - mp| over the finite values, 2^-52 max(1, |mp|))."""
    mp = _mp()
    fin = [(o, w) for o, w in pairs if isinstance(w, mp.mpf) and mp.isfinite(w)]
    err = max([abs(float(mp.mpf(o) - w)) for o, w in fin] + [0.0])
    return max(err, 2.0 ** -52 * max([1.0] + [abs(float(w)) for _, w in fin]))


def states_mp(par):
    mp = _mp()
    x, bias0, tick0 = NC.states_case()
    meas, bias_out = [], []
    for b in range(NC.B):
        bias = [mp.mpf(float(v)) for v in bias0[b]]
        rows = []
        for s in range(NC.S):
            h = key(par["seed"], par["id0"] + b, int(tick0[b]) + s, TAGS["state"])
            row = [float(v) for v in x[b, s]]
            m = list(row)
            for i in range(3):
                if math.isfinite(row[i]):
                    bias[i] = mp.mpf(par["bias_a"][i]) * bias[i] + mp.mpf(par["bias_c"][i]) * normal_mp(h, i)
                    m[i] = mp.mpf(row[i]) + bias[i] + mp.mpf(par["sigma_p"][i]) * normal_mp(h, 3 + i)
                if math.isfinite(row[3 + i]):
                    m[3 + i] = mp.mpf(row[3 + i]) + mp.mpf(par["sigma_v"][i]) * normal_mp(h, 6 + i)
                if math.isfinite(row[6 + i]):
                    m[6 + i] = mp.mpf(row[6 + i]) + mp.mpf(par["sigma_a"][i]) * normal_mp(h, 9 + i)
            rows.append(m)
        meas.append(rows); bias_out.append(list(bias))
    return x, bias0, tick0, meas, bias_out


def depth_mp(par):
    mp = _mp()
    img = NC.depth_case()
    scale, s0, s2, p_drop = (mp.mpf(par[n]) for n in ("depth_scale", "depth_sigma0", "depth_sigma2", "depth_p_drop"))
    cur = img.copy()
    outs, margin, u_margin = [], 1.0, 1.0
    tick = [0] * NC.F
    for _ in range(NC.DEPTH_CALLS):
        nxt = cur.copy()
        for f in range(NC.F):
            if not NC.DEPTH_ACTIVE[f]:
                continue
            hs = key(par["seed"], par["id0"] + f, tick[f], TAGS["depth"])
            for r in range(NC.ROWS):
                for c in range(NC.COLS):
                    pix = int(cur[f, r, c])
                    if pix == 0:
                        continue
                    h = finalise((hs + r * NC.COLS + c) % M64)
                    u = uniform_exact(h, 2)
                    u_margin = min(u_margin, abs(u - par["depth_p_drop"]))
                    if u < par["depth_p_drop"]:
                        nxt[f, r, c] = 0
                        continue
                    z = mp.mpf(pix) / scale
                    v = mp.mpf(pix) + scale * (s0 + s2 * z * z) * normal_mp(h, 0) + mp.mpf(0.5)
                    w = int(mp.floor(v))
                    margin = min(margin, float(min(v - w, w + 1 - v)))
                    nxt[f, r, c] = w if 1 <= w <= 65535 else 0
            tick[f] += 1
        outs.append(nxt)
        cur = nxt
    return img, np.array(outs, dtype=np.uint16), margin, u_margin


def scan_mp(par):
    mp = _mp()
    pts, origin, count = NC.scan_case()
    out = [[[float(v) for v in p] for p in sc] for sc in pts]
    u_margin = 1.0
    for s in range(NC.SCANS):
        hs = key(par["seed"], par["id0"] + s, 0, TAGS["scan"])
        o = [mp.mpf(float(v)) for v in origin[s]]
        for idx in range(int(count[s])):
            p = [float(v) for v in pts[s, idx]]
            if not all(math.isfinite(v) for v in p):
                continue
            d = [mp.mpf(p[i]) - o[i] for i in range(3)]
            r = mp.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            if r == 0:
                continue
            h = finalise((hs + idx) % M64)
            u = uniform_exact(h, 2)
            u_margin = min(u_margin, abs(u - par["scan_p_drop"]))
            if u < par["scan_p_drop"]:
                out[s][idx] = [float("nan")] * 3
                continue
            e = (mp.mpf(par["scan_sigma0"]) + mp.mpf(par["scan_sigma1"]) * r) * normal_mp(h, 0)
            out[s][idx] = [o[i] + d[i] * (1 + e / r) for i in range(3)]
    return pts, origin, count, out, u_margin


def main(argv):
    out = OUT
    for i, a in enumerate(argv):
        if a == "--out":
            out = argv[i + 1]
    from tests import sensor_noise_oracle as NO
    assert (NO.TAG_STATE, NO.TAG_DEPTH, NO.TAG_SCAN) == (TAGS["state"], TAGS["depth"], TAGS["scan"])
    par = NC.params()
    store = {}
    # ---- states ----
    x, bias0, tick0, meas, bias = states_mp(par)
    tol_case, tick = [], []
    for b in range(NC.B):
        om, oy, ob, ot = NO.states(x[b], bias0[b], int(tick0[b]), b, par)
        assert oy == om[-1]
        pairs = [(om[s][j], meas[b][s][j]) for s in range(NC.S) for j in range(9)] + [(ob[i], bias[b][i]) for i in range(3)]
        for o, w in pairs:                                  # what passes through passes through to the bit
            if not isinstance(w, _mp().mpf):
                assert np.array_equal(np.array(o).view(np.uint64), np.array(w).view(np.uint64))
        tol_case.append(tol(pairs))
        tick.append(ot % M64)
    store.update(states_x=x, states_bias0=bias0, states_tick0=tick0, states_tol_case=np.array(tol_case), states_tick=np.array(tick, dtype=np.uint64),
                 states_meas=np.array([[[split(v) for v in r] for r in rows] for rows in meas]), states_bias=np.array([[split(v) for v in r] for r in bias]))
    print("states  %3d vehicles; oracle error: worst %.3e, smallest %.3e" % (NC.B, max(tol_case), min(tol_case)))
    # ---- depth ----
    img, outs, margin, u_margin = depth_mp(par)
    cur, ticks = img, [0] * NC.F
    for call in range(NC.DEPTH_CALLS):
        got = []
        for f in range(NC.F):
            o, ticks[f] = NO.depth(cur[f].tolist(), f, ticks[f], par, active=NC.DEPTH_ACTIVE[f])
            got.append(o)
        cur = np.array(got, dtype=np.uint16)
        assert np.array_equal(cur, outs[call]), call        # the oracle's images are the 50-digit images
    store.update(depth_in=img, depth_out=outs, depth_margin=np.array(margin), depth_u_margin=np.array(u_margin))
    print("depth   %d x %d x %d, %d calls; v + 1/2 at least %.3e from an integer, u at least %.3e from p_drop; the oracle's images are equal" % (NC.F, NC.ROWS, NC.COLS, NC.DEPTH_CALLS, margin, u_margin))
    # ---- scan ----
    pts, origin, count, want, u_margin = scan_mp(par)
    tol_case = []
    for s in range(NC.SCANS):
        o, _ = NO.scan(pts[s], origin[s], int(count[s]), s, 0, par)
        flat_o, flat_w = [v for p in o for v in p], [v for p in want[s] for v in p]
        assert [math.isnan(v) for v in flat_o] == [(not isinstance(v, _mp().mpf)) and math.isnan(v) for v in flat_w], s
        for a_, w_ in zip(flat_o, flat_w):                 # what stays (not finite, at the origin, beyond count) and what is lost: to the bit
            if not isinstance(w_, _mp().mpf):
                assert np.array_equal(np.array(a_).view(np.uint64), np.array(w_).view(np.uint64)), s
        tol_case.append(tol(list(zip(flat_o, flat_w))))
    store.update(scan_in=pts, scan_origin=origin, scan_count=count, scan_out=np.array([[[split(v) for v in p] for p in sc] for sc in want]),
                 scan_tol_case=np.array(tol_case), scan_u_margin=np.array(u_margin))
    print("scan    %d x %d points; oracle error: %s; u at least %.3e from p_drop" % (NC.SCANS, NC.P, ", ".join("%.3e" % v for v in tol_case), u_margin))
    a, c = NC.coefficients()
    store["scalars"] = np.array(list(a) + list(c))
    store["ints"] = np.array([NC.SEED, NC.ID0], dtype=np.int64)
    store["dps"] = np.array(DPS, dtype=np.int32)
    store["tol_factor"] = np.array(TOL_FACTOR)
    write_npz(out, store)
    print("-> %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1:])
