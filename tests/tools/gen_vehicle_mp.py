#!/usr/bin/env python3
"""Multiprecision reference of the vehicle (include/frp_nmpc_vehicle.h) -> tests/golden/vehicle_mp.npz.

    python tests/tools/gen_vehicle_mp.py [--out FILE]

Written from the header's statement of the scheme; tests/vehicle_oracle.py is imported for ONE purpose, at the end: to measure its error
against what is computed here (`tol_*` below) and to check that it took the same branches.  Every float64 input is taken as an exact
value, mpmath works at DPS digits.

WHAT IS EVALUATED, per case of tests/vehicle_cases.py: mp_cases (one vehicle, S samples, n_sub):
  trace   the SAME DISCRETE SCHEME in 50 digits: per sample the setpoint, the controller (thrust, desired roll / pitch, wrapped yaw
          error, clamped rates), then n_sub Heun steps of h = dt_cmd / n_sub of  p' = v, v' = zB T / m + f - g e3 - d (I - zB zB') v,
          e' = w  with (w, T) held.  The state after every sample; `sat` the clamps that engaged; `hold` the setpoint kept.
  msg     the message of the final state for both types: the quaternion of R_z(yaw) R_y(pitch) R_x(roll) as the Hamilton product
          q_z q_y q_x, and the body-frame velocity R' v;
  odo     what the callback's formulas return on that message: the angles of mav_msgs::getEulerAnglesFromQuaternion and R(q) v_B.
and for the order test (vehicle_cases.order_case) the ODE itself, integrated over one sample of DT_ORDER seconds with the first
sample's (w, T) held, by mpmath's Taylor-series odefun at the same precision: `ode_x`.

Stored as (hi, lo) pairs of doubles.  Also stored, and printed: tol_case [C], the largest absolute error of tests/vehicle_oracle.py over a
case's trace against these values; tol_hold, tol_msg, tol_odo the same over all cases for the kept yaw, the message and the callback.  tests/test_gpu_vehicle.py
allows the device tol_factor = 8 times that (the margin of tests/golden/astar_mp.npz).  DATA only, fixed time stamps: a second run
reproduces the file bit for bit.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.tools.gen_tube_mp import write_npz      # noqa: E402
from tests import vehicle_cases as VC              # noqa: E402

DPS = 50
OUT = os.path.join(ROOT, "tests", "golden", "vehicle_mp.npz")
TOL_FACTOR = 8.0
# the model's constants (nonlinear_dynamics.m, setup.m) and the planner's stage bounds (mpc_generator_normal.m:33-46), as doubles
MASS, GRAV, DRAG = 0.745319, 9.81, 0.33
NONE, TRAJ, END, YAW = 0, 1, 2, 3


def _mp():
    import mpmath
    if mpmath.mp.dps < DPS + 10:      # (never lowered: odefun raises the working precision around its calls of the right-hand side)
        mpmath.mp.dps = DPS + 10
    return mpmath


def F(v):
    return _mp().mpf(float(v))


def bounds():
    mp = _mp()
    half_pi, pi = F(1.5707963267948966), F(3.14159265358979323846)        # the model's doubles, taken as exact
    return dict(thrust=(F(0.5 * GRAV * MASS), F(2.0 * GRAV * MASS)), rate=(-half_pi, half_pi), att=(F(-0.4 * 3.14159265358979323846), F(0.4 * 3.14159265358979323846)), pi=pi, mp=mp)


def accel(v, e, T, f):
    mp = _mp()
    sr, cr, sp, cp, sy, cy = mp.sin(e[0]), mp.cos(e[0]), mp.sin(e[1]), mp.cos(e[1]), mp.sin(e[2]), mp.cos(e[2])
    zb = [cy * sp * cr + sy * sr, sy * sp * cr - cy * sr, cp * cr]
    zv = sum(zb[i] * v[i] for i in range(3))
    a = T / F(MASS) + F(DRAG) * zv
    out = [a * zb[i] - F(DRAG) * v[i] + f[i] for i in range(3)]
    out[2] -= F(GRAV)
    return out


def heun(x, w, T, f, h):
    v, e = x[3:6], x[6:9]
    a1 = accel(v, e, T, f)
    vt = [v[i] + h * a1[i] for i in range(3)]
    et = [e[i] + h * w[i] for i in range(3)]
    a2 = accel(vt, et, T, f)
    return [x[i] + h * (v[i] + vt[i]) / 2 for i in range(3)] + [v[i] + h * (a1[i] + a2[i]) / 2 for i in range(3)] + et


MARGIN = []   # how far every clamped quantity of the last run_case stood from the edges of its branch


def clamp(v, lo, hi):
    MARGIN.append(min(abs(v - lo), abs(v - hi)))
    return (lo, -1) if v < lo else (hi, 1) if v > hi else (v, 0)


def setpoint(cmd, kind, hold):
    mp = _mp()
    zero = [mp.mpf(0)] * 3
    if kind in (TRAJ, END):
        x, y, z, w = cmd[3:7]
        yaw = mp.atan2(-(2 * x * y - 2 * w * z), 1 - 2 * (y * y + z * z))
        p, v, wf, a = cmd[0:3], cmd[7:10], cmd[10:13], cmd[13:16]
    elif kind == YAW:
        p, v, wf, a, yaw = cmd[0:3], zero, zero, zero, cmd[12]
    else:
        return hold[0:3], zero, zero, zero, hold[3]
    hold[0:3] = p
    hold[3] = yaw
    return p, v, wf, a, yaw


def control(x, sp, mass, g, gains, B):
    mp = B["mp"]
    p_ref, v_ref, w_ff, a_ff, yaw = sp
    kp, kv, ka = ([F(k) for k in gains[n]] for n in ("kp", "kv", "ka"))
    sat = 0
    a = [a_ff[i] + kp[i] * (p_ref[i] - x[i]) + kv[i] * (v_ref[i] - x[3 + i]) for i in range(3)]
    a[2] += g
    na = mp.sqrt(sum(c * c for c in a))
    T, c = clamp(mass * na, *B["thrust"])
    sat |= 1 if c < 0 else 2 if c > 0 else 0
    if na == 0:
        zb = [mp.mpf(0), mp.mpf(0), mp.mpf(1)]
        sat |= 128
    else:
        zb = [c / na for c in a]
    cx = mp.cos(yaw) * zb[0] + mp.sin(yaw) * zb[1]
    cy = mp.cos(yaw) * zb[1] - mp.sin(yaw) * zb[0]
    s, _ = clamp(-cy, mp.mpf(-1), mp.mpf(1))
    roll, c = clamp(mp.asin(s), *B["att"])
    sat |= 4 if c else 0
    pitch, c = clamp(mp.atan2(cx, zb[2]), *B["att"])
    sat |= 8 if c else 0
    d = yaw - x[8]
    k = mp.ceil((d - B["pi"]) / (2 * B["pi"]))
    MARGIN.append(abs((d - B["pi"]) / (2 * B["pi"]) - mp.nint((d - B["pi"]) / (2 * B["pi"]))))
    sat |= 256 if k != 0 else 0
    err = [roll - x[6], pitch - x[7], d - 2 * B["pi"] * k]
    w = []
    for i in range(3):
        wi, c = clamp(w_ff[i] + ka[i] * err[i], *B["rate"])
        sat |= (16 << i) if c else 0
        w.append(wi)
    return w, T, sat


def run_case(x0, hold0, f_true, cmd, kind, n_sub, dt_cmd=VC.DT_CMD):
    B = bounds()
    x, hold, f = [F(v) for v in x0], [F(v) for v in hold0], [F(v) for v in f_true]
    h = F(dt_cmd) / int(n_sub)
    trace, sats = [], []
    for s in range(len(kind)):
        sp = setpoint([F(v) for v in cmd[s]], int(kind[s]), hold)
        w, T, sat = control(x, sp, F(VC.MASS), F(VC.G), VC.GAINS, B)
        for _ in range(int(n_sub)):
            x = heun(x, w, T, f, h)
        trace.append(list(x)); sats.append(sat)
    return trace, sats, hold


def quat_zyx(e):
    """(w, x, y, z) of q_z(yaw) q_y(pitch) q_x(roll)."""
    mp = _mp()
    cr, sr, cp, sp, cy, sy = mp.cos(e[0] / 2), mp.sin(e[0] / 2), mp.cos(e[1] / 2), mp.sin(e[1] / 2), mp.cos(e[2] / 2), mp.sin(e[2] / 2)
    return [cy * cp * cr + sy * sp * sr, cy * cp * sr - sy * sp * cr, cy * sp * cr + sy * cp * sr, sy * cp * cr - cy * sp * sr]


def rot_of_quat(q):
    mp = _mp()
    w, x, y, z = q
    return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def verify_quat(q, e):
    """q_z q_y q_x against the matrices R_z R_y R_x, to 1e-45."""
    mp = _mp()
    c, s = mp.cos, mp.sin
    Rx = mp.matrix([[1, 0, 0], [0, c(e[0]), -s(e[0])], [0, s(e[0]), c(e[0])]])
    Ry = mp.matrix([[c(e[1]), 0, s(e[1])], [0, 1, 0], [-s(e[1]), 0, c(e[1])]])
    Rz = mp.matrix([[c(e[2]), -s(e[2]), 0], [s(e[2]), c(e[2]), 0], [0, 0, 1]])
    D = rot_of_quat(q) - Rz * Ry * Rx
    assert max(abs(D[i, j]) for i in range(3) for j in range(3)) < mp.mpf(10) ** -45


def link(x):
    """x (a float64 state taken as exact) -> (msg1 [13], msg2 [13], odo [9])."""
    mp = _mp()
    x = [F(v) for v in x]
    q = quat_zyx(x[6:9])
    verify_quat(q, x[6:9])
    R = rot_of_quat(q)
    v = mp.matrix(x[3:6])
    vb = R.T * v
    zero = [mp.mpf(0)] * 3
    head = x[0:3] + [q[1], q[2], q[3], q[0]]
    w, qx, qy, qz = q
    ang = [mp.atan2(2 * (w * qx + qy * qz), 1 - 2 * (qx * qx + qy * qy)), mp.asin(2 * (w * qy - qz * qx)), mp.atan2(2 * (w * qz + qx * qy), 1 - 2 * (qy * qy + qz * qz))]
    return head + list(v) + zero, head + list(vb) + zero, x[0:3] + list(R * vb) + ang


def ode_reference():
    """The ODE of the order case over DT_ORDER with the first sample's (w, T) held."""
    mp = _mp()
    c = VC.order_case()
    B = bounds()
    x = [F(v) for v in c["x0"]]
    hold = [F(v) for v in c["hold0"]]
    sp = setpoint([F(v) for v in c["cmd"][0]], TRAJ, hold)
    w, T, sat = control(x, sp, F(VC.MASS), F(VC.G), VC.GAINS, B)
    assert sat == 0
    f = [F(v) for v in c["f_true"]]
    e0 = x[6:9]

    def rhs(t, y):
        e = [e0[i] + w[i] * t for i in range(3)]
        return list(y[3:6]) + accel(y[3:6], e, T, f)
    sol = mp.odefun(rhs, 0, x[0:6])
    y = sol(F(VC.DT_ORDER))
    return list(y) + [e0[i] + w[i] * F(VC.DT_ORDER) for i in range(3)]


def split(x):
    hi = float(x)
    return hi, float(x - _mp().mpf(hi))


def main(argv):
    out = OUT
    for i, a in enumerate(argv):
        if a == "--out":
            out = argv[i + 1]
    from tests import vehicle_oracle as VO
    mp = _mp()
    cases, labels = VC.mp_cases()
    C = len(labels)
    pair = lambda rows: np.array([[split(v) for v in r] for r in rows])
    err = lambda got, want: max(abs(float(mp.mpf(float(g)) - w)) for g, w in zip(got, want))
    T, SAT, H, M1, M2, OD, tol_case = [], [], [], [], [], [], []
    tol_msg = tol_odo = tol_hold = 0.0
    for c in range(C):
        a = {k: v[c] for k, v in cases.items()}
        del MARGIN[:]
        trace, sats, hold = run_case(a["x0"], a["hold0"], a["f_true"], a["cmd"], a["kind"], a["n_sub"])
        assert min(MARGIN) > 1e-3, (c, labels[c], float(min(MARGIN)))   # no case next to the edge of a branch
        x, oh, otrace, osats = VO.step(a["x0"], a["hold0"], a["f_true"], a["cmd"], a["kind"], mass=VC.MASS, g=VC.G, dt_cmd=VC.DT_CMD, n_sub=int(a["n_sub"]), **VC.GAINS)
        assert osats == sats, (c, labels[c], osats, sats)
        assert [float(v) for v in hold[0:3]] == oh[0:3], (c, labels[c])
        tol = max(err(o, t) for o, t in zip(otrace, trace))
        assert tol > 0.0, (c, labels[c])
        tol_case.append(tol)
        tol_hold = max(tol_hold, err(oh[3:4], hold[3:4]))
        T.append([v for row in trace for v in row]); SAT.append(sats); H.append(hold)
        # the link, from the oracle's final state (a float64 state both sides take as exact)
        m1, m2, od = link(x)
        M1.append(m1); M2.append(m2); OD.append(od)
        for t, m in ((VO.ODOM_WORLD, m1), (VO.ODOM_BODY, m2)):
            om = VO.message(x, t)
            tol_msg = max(tol_msg, err(om, m))
            st, _, _ = VO.odometry(om, 1, t, [0.0] * 9, [0.0] * 9, 0)
            tol_odo = max(tol_odo, err(st, od))
    S = cases["kind"].shape[1]
    arrays = dict(cases, mass=np.array(VC.MASS), g=np.array(VC.G), dt_cmd=np.array(VC.DT_CMD), kp=np.array(VC.GAINS["kp"]), kv=np.array(VC.GAINS["kv"]),
                  ka=np.array(VC.GAINS["ka"]), trace=pair(T).reshape(C, S, 9, 2), sat=np.array(SAT, dtype=np.int32), hold=pair(H),
                  x_link=np.array([VO.step(*(cases[k][c] for k in ("x0", "hold0", "f_true", "cmd", "kind")), mass=VC.MASS, g=VC.G, dt_cmd=VC.DT_CMD,
                                           n_sub=int(cases["n_sub"][c]), **VC.GAINS)[0] for c in range(C)]),
                  msg_world=pair(M1), msg_body=pair(M2), odo=pair(OD), ode_x=pair([ode_reference()])[0], dt_order=np.array(VC.DT_ORDER),
                  dps=np.array(DPS, dtype=np.int32), tol_factor=np.array(TOL_FACTOR), tol_case=np.array(tol_case), tol_hold=np.array(tol_hold),
                  tol_msg=np.array(tol_msg), tol_odo=np.array(tol_odo))
    write_npz(out, arrays)
    worst = int(np.argmax(tol_case))
    print("%d cases; oracle error: trace worst %.3e (case %d, %s), smallest %.3e; kept yaw %.3e, message %.3e, callback %.3e -> %s (%d bytes)"
          % (C, max(tol_case), worst, labels[worst], min(tol_case), tol_hold, tol_msg, tol_odo, out, os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1:])
