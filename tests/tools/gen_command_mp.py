#!/usr/bin/env python3
"""Multiprecision reference of the command timer's arithmetic (include/frp_nmpc_command.h) -> tests/golden/command_mp.npz.

    python tests/tools/gen_command_mp.py [--out FILE]

Written from the mathematics; tests/command_oracle.py is imported for ONE purpose, at the end: to measure its error against what is
computed here (`tol_*` below).  Every float64 input is taken as an exact value, mpmath works at DPS digits.

WHAT IS EVALUATED, per case (a plan of MP_N rows of 17, a time t, Ts = 0.05, mass, g -- tests/command_cases.py: mp_cases):
  pose   the plan, piecewise linear in time through its rows at 0, Ts, 2 Ts, ...:  i = floor(t / Ts),  lam = (t - i Ts) / Ts,
         row = (1 - lam) row_i + lam row_{i+1}, all exact rational arithmetic of the doubles.  (t on a row boundary k * Ts is the row k
         from either side; the float k * 0.05 is not the real k * 0.05, and the difference is carried exactly.)
  quat   the unit quaternion of the rotation  R_x(roll) R_y(pitch) R_z(yaw)  of the interpolated angles, as the Hamilton product
         q_x(roll) q_y(pitch) q_z(yaw), q_a(phi) = cos(phi / 2) + sin(phi / 2) e_a, multiplied out:
             w = cr cp cy - sr sp sy      x = sr cp cy + cr sp sy      y = cr sp cy - sr cp sy      z = cr cp sy + sr sp cy
         (c., s. of the HALF angles).  verify() checks it against the matrices: unit norm, and v -> q v q* equals R_x R_y R_z v for
         the three basis vectors, to 1e-45.
  acc    R_z(yaw) R_y(pitch) R_x(roll) e_3 * thrust / mass - g e_3, from the three elementary rotation matrices multiplied in mp.
and per yaw of mp_yaws(): (sin(yaw / 2), cos(yaw / 2)), the z and w of the quaternion of a rotation about z.

Stored as (hi, lo) pairs of doubles, hi + lo exact to ~32 digits.  Also stored, and printed: tol_pose, tol_quat, tol_acc, tol_yaw -- the
largest absolute error of tests/command_oracle.py over all cases against these values; tests/test_gpu_command.py allows the device
tol_factor = 8 times that (the margin of tests/golden/astar_mp.npz).  DATA only, fixed time stamps: a second run reproduces the
file bit for bit.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.tools.gen_tube_mp import write_npz      # noqa: E402
from tests import command_cases as CC              # noqa: E402

DPS = 50
OUT = os.path.join(ROOT, "tests", "golden", "command_mp.npz")
TOL_FACTOR = 8.0
MASS, G = 0.74, 9.81


def _mp():
    import mpmath
    mpmath.mp.dps = DPS + 10
    return mpmath


def rot(axis, phi):
    mp = _mp()
    c, s = mp.cos(phi), mp.sin(phi)
    if axis == 0:
        return mp.matrix([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == 1:
        return mp.matrix([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return mp.matrix([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def pose(plan, t, Ts):
    mp = _mp()
    F = mp.mpf
    t, Ts = F(float(t)), F(float(Ts))
    i = int(mp.floor(t / Ts))
    lam = (t - i * Ts) / Ts
    return [(1 - lam) * F(float(plan[i][j])) + lam * F(float(plan[i + 1][j])) for j in range(17)]


def quat_xyz(roll, pitch, yaw):
    """(x, y, z, w) of q_x(roll) q_y(pitch) q_z(yaw)."""
    mp = _mp()
    cr, sr, cp, sp, cy, sy = mp.cos(roll / 2), mp.sin(roll / 2), mp.cos(pitch / 2), mp.sin(pitch / 2), mp.cos(yaw / 2), mp.sin(yaw / 2)
    return [sr * cp * cy + cr * sp * sy, cr * sp * cy - sr * cp * sy, cr * cp * sy + sr * sp * cy, cr * cp * cy - sr * sp * sy]


def rotate(q, v):
    """q v q* for q = (x, y, z, w): v + 2 w (u x v) + 2 u x (u x v)."""
    mp = _mp()
    u, w = mp.matrix(q[:3]), q[3]
    cross = lambda a, b: mp.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    uv = cross(u, v)
    return v + 2 * w * uv + 2 * cross(u, uv)


def verify(q, roll, pitch, yaw):
    mp = _mp()
    eps = mp.mpf(10) ** -45
    assert abs(sum(c * c for c in q) - 1) < eps
    R = rot(0, roll) * rot(1, pitch) * rot(2, yaw)
    for k in range(3):
        e = mp.matrix([1 if j == k else 0 for j in range(3)])
        d = rotate(q, e) - R * e
        assert max(abs(d[j]) for j in range(3)) < eps, (k, d)


def acc(row, mass, g):
    mp = _mp()
    F = mp.mpf
    z = rot(2, row[16]) * rot(1, row[15]) * rot(0, row[14]) * mp.matrix([0, 0, 1])
    a = [z[k] * row[3] / F(float(mass)) for k in range(3)]
    a[2] -= F(float(g))
    return a


def split(x):
    hi = float(x)
    return hi, float(x - _mp().mpf(hi))


def evaluate():
    plan, t = CC.mp_cases()
    P, Q, A = [], [], []
    for c in range(len(t)):
        row = pose(plan[c], t[c], CC.TS)
        q = quat_xyz(row[14], row[15], row[16])
        verify(q, row[14], row[15], row[16])
        P.append(row); Q.append(q); A.append(acc(row, MASS, G))
    mp = _mp()
    yaws = CC.mp_yaws()
    Y = [[mp.sin(mp.mpf(float(y)) / 2), mp.cos(mp.mpf(float(y)) / 2)] for y in yaws]
    return plan, t, yaws, P, Q, A, Y


def oracle_errors(plan, t, yaws, P, Q, A, Y):
    """The float64 restatement against the values above: largest absolute errors."""
    import math
    from tests import command_oracle as CO
    mp = _mp()
    worst = dict(pose=0.0, quat=0.0, acc=0.0, yaw=0.0)
    slots = list(range(0, 4)) + list(range(8, 17))
    for c in range(len(t)):
        idx = int(t[c] / CC.TS)
        mpcq = CO.interpolate(plan[c], idx, float(t[c]), CC.TS)
        o = CO.trajectory_point(mpcq, MASS, G)
        worst["pose"] = max(worst["pose"], max(abs(float(mp.mpf(mpcq[j]) - P[c][j])) for j in slots))
        worst["quat"] = max(worst["quat"], max(abs(float(mp.mpf(o[3 + k]) - Q[c][k])) for k in range(4)))
        worst["acc"] = max(worst["acc"], max(abs(float(mp.mpf(o[13 + k]) - A[c][k])) for k in range(3)))
    for y, (s, cc) in zip(yaws, Y):
        worst["yaw"] = max(worst["yaw"], abs(float(mp.mpf(math.sin(0.5 * float(y))) - s)), abs(float(mp.mpf(math.cos(0.5 * float(y))) - cc)))
    return worst


def main(argv):
    out = OUT
    for i, a in enumerate(argv):
        if a == "--out":
            out = argv[i + 1]
    plan, t, yaws, P, Q, A, Y = evaluate()
    worst = oracle_errors(plan, t, yaws, P, Q, A, Y)
    pair = lambda rows: np.array([[split(v) for v in r] for r in rows])      # [C][k][2]
    arrays = dict(plan=plan, t=t, Ts=np.array(CC.TS), mass=np.array(MASS), g=np.array(G), pose=pair(P), quat=pair(Q), acc=pair(A),
                  yaws=yaws, yaw_sc=pair(Y), dps=np.array(DPS, dtype=np.int32), tol_factor=np.array(TOL_FACTOR),
                  tol_pose=np.array(worst["pose"]), tol_quat=np.array(worst["quat"]), tol_acc=np.array(worst["acc"]), tol_yaw=np.array(worst["yaw"]))
    write_npz(out, arrays)
    print("%d cases + %d yaws; oracle error: pose %.3e, quat %.3e, acc %.3e, yaw quaternion %.3e -> %s (%d bytes)"
          % (len(t), len(yaws), worst["pose"], worst["quat"], worst["acc"], worst["yaw"], out, os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1:])
