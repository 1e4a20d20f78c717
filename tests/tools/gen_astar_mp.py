#!/usr/bin/env python3
"""Multiprecision reference of the kinodynamic A*'s heuristic (second half) -> tests/golden/astar_mp.npz.

    python tests/tools/gen_astar_mp.py [--out FILE]

Written from the mathematics; it neither imports nor follows oracle/astar_oracle.c.  Every float64 input is taken as an exact value,
mpmath works at DPS digits.

THE PROBLEM.  A double integrator p'' = u in three dimensions goes from (p0, v0) to (p1, v1) in a free time T; the cost is
    J = int_0^T (|u|^2 + w) dt.
For a fixed T the Hamiltonian |u|^2 + l_p.v + l_v.u gives l_p' = 0, l_v' = -l_p and u = -l_v / 2: the optimal u is LINEAR in t,
    u(t) = alpha + beta t.
The two end conditions, with dv = v1 - v0 and e = (p1 - p0) - v0 T:
    alpha T + beta T^2 / 2 = dv,      alpha T^2 / 2 + beta T^3 / 6 = e
    =>  beta = -12 e / T^3 + 6 dv / T^2,     alpha = 6 e / T^2 - 2 dv / T.
The energy is  int |u|^2 = |alpha|^2 T + alpha.beta T^2 + |beta|^2 T^3 / 3  -- j_of_T() below evaluates J EXACTLY THIS WAY, from alpha
and beta.  Substituting and collecting powers of T (dp = p1 - p0) gives the closed form
    J(T) = w T + 12 |dp|^2 / T^3 - 12 (v0 + v1).dp / T^2 + 4 (|v0|^2 + v0.v1 + |v1|^2) / T,
which verify() checks against the boundary-value evaluation, and
    T^4 J'(T) = w T^4 - 4 (|v0|^2 + v0.v1 + |v1|^2) T^2 + 24 (v0 + v1).dp T - 36 |dp|^2.
The planner may not be faster than max_vel on any axis: T >= t_bar = max_i |dp_i| / max_vel.  Stored per case: the constrained
minimum J_min = min_{T >= t_bar} J(T) and its minimiser.  J -> +inf at both ends of (0, inf) (for dp != 0), so the minimum is at a real
root of the quartic T^4 J' that is >= t_bar, or at t_bar: the roots come from mpmath.polyroots at DPS digits, J is evaluated at the
real part of every root >= t_bar (a point that is no stationary point is still feasible: it cannot lower the minimum) and at t_bar.
verify() re-checks the result against the equation: J'(T_min) = 0 to 1e-40 of its largest term or T_min = t_bar with J'(t_bar) >= 0,
and J(T_min) <= J(T) on 4000 log-spaced T >= t_bar.

CASES (SETTINGS = (w_time, max_vel): the launch defaults and two others), x1 = (p0, v0), x2 = (p1, v1):
  generic      random pairs in the map, |v| <= max_vel, half of them with v1 = 0 (the planner's goal), half with v1 != 0
  far          8 .. 18 m apart: t_bar is the minimiser
  rest         v0 = v1 = 0
  aligned      dp within 1e-3 .. 1e-9 rad of +-(v0 + v1)
  disc         Ferrari's resolvent cubic  y^3 - a2 y^2 - 4 a0 y + (4 a2 a0 - a1^2)  of the monic quartic t^4 + a2 t^2 + a1 t + a0 has
               discriminant-like D = Q^3 + R^2 (Q = (3 b1 - b2^2) / 9, R = (9 b1 b2 - 27 b0 - 2 b2^3) / 54 for y^3 + b2 y^2 + b1 y + b0);
               the speed along dp is bisected in mp until D = 0, and the case is stored at that speed times (1 +- 1e-3, 1e-6, 1e-9):
               both signs of D, where a closed-form solver switches between its one-real-root and three-real-root branches

Also stored: `tol_measured`, the worst relative cost error of an INDEPENDENT float64 solve (numpy.roots on the quartic above, J in
float64 at the real parts >= t_bar and at t_bar) against J_min, and `tol_factor` = 8: tests/test_oracle_astar_mp.py allows the
oracle 8 x the measured value (Ferrari's closed formulas are less stable than companion-matrix roots).  The file holds DATA only and
is written with fixed time stamps: a second run reproduces it bit for bit.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.tools.gen_tube_mp import write_npz      # noqa: E402

DPS = 60
OUT = os.path.join(ROOT, "tests", "golden", "astar_mp.npz")
SETTINGS = ((10.0, 2.0), (1.0, 3.0), (50.0, 1.0))
TOL_FACTOR = 8.0


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


def _vec(x):
    F = _mp().mpf
    return [F(float(v)) for v in x]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def t_bar_of(x1, x2, max_vel):
    F = _mp().mpf
    return max(abs(F(float(x2[i])) - F(float(x1[i]))) for i in range(3)) / F(float(max_vel))


def j_of_T(x1, x2, w, T):
    """J(T) from the boundary-value problem: alpha, beta of the linear optimal control, then its energy + w T."""
    F = _mp().mpf
    p0, v0, p1, v1 = _vec(x1[:3]), _vec(x1[3:]), _vec(x2[:3]), _vec(x2[3:])
    dv = [v1[i] - v0[i] for i in range(3)]
    e = [p1[i] - p0[i] - v0[i] * T for i in range(3)]
    beta = [-12 * e[i] / T ** 3 + 6 * dv[i] / T ** 2 for i in range(3)]
    alpha = [6 * e[i] / T ** 2 - 2 * dv[i] / T for i in range(3)]
    return _dot(alpha, alpha) * T + _dot(alpha, beta) * T ** 2 + _dot(beta, beta) * T ** 3 / 3 + F(float(w)) * T


def coefficients(x1, x2):
    """(d, s, c) = (|dp|^2, (v0 + v1).dp, |v0|^2 + v0.v1 + |v1|^2) in mp."""
    p0, v0, p1, v1 = _vec(x1[:3]), _vec(x1[3:]), _vec(x2[:3]), _vec(x2[3:])
    dp = [p1[i] - p0[i] for i in range(3)]
    vs = [v0[i] + v1[i] for i in range(3)]
    return _dot(dp, dp), _dot(vs, dp), _dot(v0, v0) + _dot(v0, v1) + _dot(v1, v1)


def j_closed(x1, x2, w, T):
    F = _mp().mpf
    d, s, c = coefficients(x1, x2)
    return F(float(w)) * T + 12 * d / T ** 3 - 12 * s / T ** 2 + 4 * c / T


def dj_T4(x1, x2, w, T):
    """T^4 J'(T) and the largest of its terms."""
    F = _mp().mpf
    d, s, c = coefficients(x1, x2)
    terms = [F(float(w)) * T ** 4, -4 * c * T ** 2, 24 * s * T, -36 * d]
    return sum(terms), max(abs(t) for t in terms)


def solve(x1, x2, w, max_vel):
    """(t_bar, T_min, J_min) in mp."""
    mp = _mp()
    F = mp.mpf
    d, s, c = coefficients(x1, x2)
    tb = t_bar_of(x1, x2, max_vel)
    roots = mp.polyroots([F(float(w)), F(0), -4 * c, 24 * s, -36 * d], maxsteps=2000, extraprec=4 * DPS)
    cand = [tb] + [mp.re(r) for r in roots if mp.re(r) >= tb]
    best = min(cand, key=lambda T: j_of_T(x1, x2, w, T))
    return tb, best, j_of_T(x1, x2, w, best)


def verify(x1, x2, w, max_vel, T_min, J_min):
    """The stored minimum against the equation it claims to solve; returns the residuals it asserts on."""
    mp = _mp()
    F = mp.mpf
    tb = t_bar_of(x1, x2, max_vel)
    assert T_min >= tb
    closed = abs(j_closed(x1, x2, w, T_min) - J_min) / abs(J_min)
    assert closed < F(10) ** (-DPS + 12), closed
    r, big = dj_T4(x1, x2, w, T_min)
    if T_min == tb:
        assert r >= -big * F(10) ** -40, (r, big)
        stat = F(0)
    else:
        stat = abs(r) / big
        assert stat < F(10) ** -40, stat
    hi = max(4 * T_min, tb * 64, F(64))
    grid = [tb * (hi / tb) ** (F(k) / 3999) for k in range(4000)] if tb > 0 else [hi * F(k + 1) / 4000 for k in range(4000)]
    worst = min(j_closed(x1, x2, w, T) for T in grid)
    assert worst >= J_min * (1 - F(10) ** -40), (worst, J_min)
    return dict(closed=float(closed), stationary=float(stat))


def resolvent_D(x1, x2, w):
    """D = Q^3 + R^2 of Ferrari's resolvent cubic of the monic quartic T^4 J' / w."""
    F = _mp().mpf
    d, s, c = coefficients(x1, x2)
    a2, a1, a0 = -4 * c / F(float(w)), 24 * s / F(float(w)), -36 * d / F(float(w))
    b2, b1, b0 = -a2, -4 * a0, 4 * a2 * a0 - a1 * a1
    Q = (3 * b1 - b2 * b2) / 9
    R = (9 * b1 * b2 - 27 * b0 - 2 * b2 ** 3) / 54
    return Q ** 3 + R * R


def _disc_cases(rng, w, n):
    """Pairs whose D is 0 at some speed lam along dp (v0 = lam dir + small cross part, v1 = 0): lam bisected in mp, cases at lam (1 +- eps)."""
    out = []
    tries = 0
    while len(out) < n and tries < 200:
        tries += 1
        p0 = rng.uniform(-6, 6, 3) * np.array([1, 1, 0.1]); dp = rng.uniform(-5, 5, 3) * np.array([1, 1, 0.2])
        dirn = dp / np.linalg.norm(dp)
        cross = rng.uniform(-0.2, 0.2, 3)
        mk = lambda lam: (np.r_[p0, lam * dirn + cross], np.r_[p0 + dp, 0.0, 0.0, 0.0])
        lams = np.linspace(0.05, 4.0, 80)
        Ds = [resolvent_D(*mk(float(l)), w) for l in lams]
        for k in range(len(lams) - 1):
            if (Ds[k] > 0) != (Ds[k + 1] > 0):
                lo, hi, flo = float(lams[k]), float(lams[k + 1]), Ds[k] > 0
                for _ in range(60):
                    mid = 0.5 * (lo + hi)
                    if (resolvent_D(*mk(mid), w) > 0) == flo:
                        lo = mid
                    else:
                        hi = mid
                for eps in (1e-3, 1e-6, 1e-9):
                    for sg in (-1.0, 1.0):
                        out.append(mk(lo * (1.0 + sg * eps)))
                break
    return out[:n]


def case_list():
    """[(kind, x1 [6], x2 [6], w_time, max_vel)] -- seeded, the same list on every run."""
    cases = []
    for si, (w, vm) in enumerate(SETTINGS):
        rng = np.random.default_rng(4100 + si)
        pos = lambda: rng.uniform(-9, 9, 3) * np.array([1, 1, 0.1]) + np.array([0, 0, 1.0])
        vel = lambda: rng.uniform(-vm, vm, 3)
        for k in range(40):
            cases.append(("generic", np.r_[pos(), vel()], np.r_[pos(), vel() if k % 2 else np.zeros(3)], w, vm))
        for k in range(12):
            p0 = pos() * np.array([0.2, 0.2, 1.0]); ang = rng.uniform(0, 2 * np.pi); L = rng.uniform(8, 18)
            cases.append(("far", np.r_[p0, vel() * 0.3], np.r_[p0 + L * np.array([np.cos(ang), np.sin(ang), 0.02]), vel() * (k % 2)], w, vm))
        for k in range(8):
            cases.append(("rest", np.r_[pos(), np.zeros(3)], np.r_[pos(), np.zeros(3)], w, vm))
        for k in range(12):
            p0, dp = pos(), rng.uniform(-5, 5, 3) * np.array([1, 1, 0.1])
            vs = dp / np.linalg.norm(dp) * rng.uniform(0.3, vm) * (1 if k % 2 else -1)
            tilt = np.cross(dp, rng.uniform(-1, 1, 3)); tilt /= np.linalg.norm(tilt)
            vs = vs + tilt * np.linalg.norm(vs) * 10.0 ** -(3 + 2 * (k % 4))
            split = rng.uniform(0, 1) if k % 3 else 1.0
            cases.append(("aligned", np.r_[p0, vs * split], np.r_[p0 + dp, vs * (1 - split)], w, vm))
        for x1, x2 in _disc_cases(rng, w, 18):
            cases.append(("disc", x1, x2, w, vm))
    return cases


def float64_solve(x1, x2, w, max_vel):
    """The independent float64 solve the tolerance is measured with: numpy.roots on T^4 J', J in float64 at the candidates."""
    x1 = np.asarray(x1, dtype=np.float64); x2 = np.asarray(x2, dtype=np.float64)
    dp = x2[:3] - x1[:3]; v0, v1 = x1[3:], x2[3:]
    d, s, c = float(dp @ dp), float((v0 + v1) @ dp), float(v0 @ v0 + v0 @ v1 + v1 @ v1)
    tb = float(np.max(np.abs(dp))) / max_vel
    cand = [tb] + [float(r.real) for r in np.roots([w, 0.0, -4.0 * c, 24.0 * s, -36.0 * d]) if r.real >= tb]
    J = [w * T + 12.0 * d / T ** 3 - 12.0 * s / T ** 2 + 4.0 * c / T for T in cand if T > 0.0]
    return min(J)


def split_double(x):
    """An mp value as (hi, lo) doubles, hi + lo exact to ~32 digits."""
    hi = float(x)
    return hi, float(x - _mp().mpf(hi))


def main(argv):
    out = OUT
    for i, a in enumerate(argv):
        if a == "--out":
            out = argv[i + 1]
    mp = _mp()
    cases = case_list()
    rows = []
    worst = 0.0
    for kind, x1, x2, w, vm in cases:
        tb, T, J = solve(x1, x2, w, vm)
        verify(x1, x2, w, vm, T, J)
        Jh, Jl = split_double(J)
        Th, Tl = split_double(T)
        rows.append((float(tb), Th, Tl, Jh, Jl, 1.0 if T == tb else 0.0, float(mp.sign(resolvent_D(x1, x2, w)))))
        worst = max(worst, abs(float((mp.mpf(float64_solve(x1, x2, w, vm)) - J) / J)))
    arrays = dict(kind=np.array([c[0] for c in cases]), x1=np.stack([c[1] for c in cases]), x2=np.stack([c[2] for c in cases]),
                  w_time=np.array([c[3] for c in cases]), max_vel=np.array([c[4] for c in cases]),
                  result=np.array(rows), result_keys=np.array(["t_bar", "T_hi", "T_lo", "J_hi", "J_lo", "at_t_bar", "sign_D"]),
                  dps=np.array(DPS, dtype=np.int32), tol_measured=np.array(worst), tol_factor=np.array(TOL_FACTOR))
    write_npz(out, arrays)
    print("%d cases, worst float64-solve error %.3e -> %s (%d bytes)" % (len(cases), worst, out, os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1:])
