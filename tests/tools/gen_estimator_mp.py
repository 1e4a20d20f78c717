#!/usr/bin/env python3
"""Multiprecision reference of the force estimator (include/frp_nmpc_estimator.h) -> tests/golden/estimator_mp.npz.

    python tests/tools/gen_estimator_mp.py [--out FILE]

Written from the header's statement of the scheme; tests/estimator_oracle.py is imported for ONE purpose, at the end: to measure its error
against what is computed here (`tol_case` below) and to check that it took the same branches.  Every float64 input is taken as an exact
value, mpmath works at DPS digits.

WHAT IS EVALUATED, per case of tests/estimator_cases.py: mp_cases (one estimator, one call of S samples): the SAME DISCRETE SCHEME in 50
digits -- per sample the branch (not finite / first / update), and in an update  a0 = accel(v_prev, e_prev, T, 0), a1 = accel(v, e, T, 0)
of  zB T / m - g e3 - d (I - zB zB') v,  dv = (v - v_prev) / dt, m = (a0 + a1) / 2, r = dv - m, f_hat <- f_hat + alpha (r - f_hat).
Stored: f_hat, force, residual [5][3] as (hi, lo) pairs of doubles (residual rows beyond S are 0); y_prev [9] (a copy of a measurement or
of y_prev0: exact); count, fresh, status [5] (rows beyond S are -1).  Every label's status sequence, final count and fresh flag are
asserted against estimator_cases.EXPECT, so every branch the case list names is taken; an empty one fails here.

Also stored, and printed: tol_case [C], the largest absolute error of tests/estimator_oracle.py over a case's f_hat, force and residual
against these values, and never below FLOOR = 2^-52 times the largest magnitude among the case's residuals, estimates and 1: one unit
in the last place of the quantities compared, so that a case the oracle happens to hit exactly (a first call: copies alone) still states
a precision.  tests/test_gpu_estimator.py allows the device tol_factor = 8 times that (the margin of tests/golden/vehicle_mp.npz).  DATA
only, fixed time stamps: a second run reproduces the file bit for bit.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.tools.gen_tube_mp import write_npz      # noqa: E402
from tests import estimator_cases as EC            # noqa: E402

DPS = 50
OUT = os.path.join(ROOT, "tests", "golden", "estimator_mp.npz")
TOL_FACTOR = 8.0
MASS, GRAV, DRAG = 0.745319, 9.81, 0.33            # the model's constants (nonlinear_dynamics.m, setup.m), as doubles
SKIPPED, FIRST, ABSORBED = 0, 1, 2


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


def F(v):
    return _mp().mpf(float(v))


def accel0(v, e, T):
    """The model's acceleration without an external force."""
    mp = _mp()
    sr, cr, sp, cp, sy, cy = mp.sin(e[0]), mp.cos(e[0]), mp.sin(e[1]), mp.cos(e[1]), mp.sin(e[2]), mp.cos(e[2])
    zb = [cy * sp * cr + sy * sr, sy * sp * cr - cy * sr, cp * cr]
    zv = sum(zb[i] * v[i] for i in range(3))
    a = T / F(MASS) + F(DRAG) * zv
    out = [a * zb[i] - F(DRAG) * v[i] for i in range(3)]
    out[2] -= F(GRAV)
    return out


def run_case(meas, thrust, S, f_hat0, y_prev0, count0, alpha, min_samples, dt=EC.DT):
    mp = _mp()
    fh = [F(v) for v in f_hat0]
    yp = [float(v) for v in y_prev0]
    count = int(count0)
    res, stat = [], []
    for s in range(int(S)):
        y, T = [float(v) for v in meas[s]], float(thrust[s])
        r = [mp.mpf(0)] * 3
        if not (math.isfinite(T) and all(math.isfinite(v) for v in y)):
            count, st = -1, SKIPPED
        elif count == -1:
            yp, count, st = list(y), 0, FIRST
        else:
            a0 = accel0([F(v) for v in yp[3:6]], [F(v) for v in yp[6:9]], F(T))
            a1 = accel0([F(v) for v in y[3:6]], [F(v) for v in y[6:9]], F(T))
            r = [(F(y[3 + i]) - F(yp[3 + i])) / F(dt) - (a0[i] + a1[i]) / 2 for i in range(3)]
            fh = [fh[i] + F(alpha) * (r[i] - fh[i]) for i in range(3)]
            count = min(count + 1, EC.INT_MAX)
            yp, st = list(y), ABSORBED
        res.append(r); stat.append(st)
    return fh, yp, count, int(count >= int(min_samples)), res, stat


def split(x):
    hi = float(x)
    return hi, float(x - _mp().mpf(hi))


def main(argv):
    out = OUT
    for i, a in enumerate(argv):
        if a == "--out":
            out = argv[i + 1]
    from tests import estimator_oracle as EO
    mp = _mp()
    cases, labels = EC.mp_cases()
    C = len(labels)
    assert C == 2 * EC.PER_ALPHA and set(labels) == set(EC.EXPECT)                     # every named branch has a case
    err = lambda got, want: max(abs(float(mp.mpf(float(g)) - w)) for g, w in zip(got, want))
    FH, RES, YP, CNT, FR, ST, tol_case = [], [], [], [], [], [], []
    seen = set()
    for c in range(C):
        a = {k: v[c] for k, v in cases.items()}
        S = int(a["S"])
        fh, yp, count, fresh, res, stat = run_case(**a)
        exp = EC.EXPECT[labels[c]]
        assert (S, int(a["count0"])) == exp[0:2] and tuple(stat) == exp[2] and (count, fresh) == exp[3:5], (c, labels[c], stat, count, fresh)
        seen.update(stat)
        o = EO.update(a["meas"][:S], a["thrust"][:S], a["f_hat0"], a["y_prev0"], int(a["count0"]), EC.DT, float(a["alpha"]), int(a["min_samples"]))
        assert (o[1], o[2], o[4], o[6]) == (yp, count, fresh, stat), (c, labels[c])
        flat = [v for row in res for v in row]
        oflat = [v for row in o[5] for v in row]
        tol = max(err(o[0], fh), err(o[3], fh), err(oflat, flat))
        floor = 2.0 ** -52 * max([1.0] + [abs(float(v)) for v in flat + fh])
        tol_case.append(max(tol, floor))
        if labels[c] == "zero_residual":
            assert max(abs(float(v)) for v in flat) < 1e-14, [float(v) for v in flat]
        if labels[c] in ("thrust_lo", "thrust_hi"):
            assert all(float(t) == (EC.THRUST_LO if labels[c] == "thrust_lo" else EC.THRUST_HI) for t in a["thrust"][:S])
        pad = [[mp.mpf(0)] * 3] * (EC.S_MAX - S)
        FH.append(fh); RES.append([v for row in res + pad for v in row]); YP.append(yp); CNT.append(count); FR.append(fresh)
        ST.append(stat + [-1] * (EC.S_MAX - S))
    assert seen == {SKIPPED, FIRST, ABSORBED}
    assert set(cases["alpha"].tolist()) == set(EC.ALPHAS) and set(cases["S"].tolist()) == {1, 5}
    pair = lambda rows: np.array([[split(v) for v in r] for r in rows])
    arrays = dict(cases, dt=np.array(EC.DT), f_hat=pair(FH), force=pair(FH), residual=pair(RES).reshape(C, EC.S_MAX, 3, 2), y_prev=np.array(YP),
                  count=np.array(CNT, dtype=np.int32), fresh=np.array(FR, dtype=np.int32), status=np.array(ST, dtype=np.int32),
                  dps=np.array(DPS, dtype=np.int32), tol_factor=np.array(TOL_FACTOR), tol_case=np.array(tol_case))
    write_npz(out, arrays)
    worst = int(np.argmax(tol_case))
    print("%d cases; oracle error: worst %.3e (case %d, %s), smallest %.3e -> %s (%d bytes)"
          % (C, max(tol_case), worst, labels[worst], min(tol_case), out, os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1:])
