#!/usr/bin/env python3
"""Exact and multiprecision reference of the disturbance model (include/frp_nmpc.h section 15) -> tests/golden/disturbance_mp.npz.

    python tests/tools/gen_disturbance_mp.py [--out FILE]

Written from the header's statement of the scheme; tests/disturbance_oracle.py is imported for ONE purpose, at the end of each case: to
measure its error against what is computed here (`tol_case`) and to check that it took the same branches.  Every float64 input is taken
as an exact value.

WHAT IS EVALUATED, per scene and case of tests/disturbance_cases.py:
  * Times, zones and events in EXACT RATIONAL arithmetic (fractions.Fraction): every product, quotient and sum the header names is formed
    exactly and rounded to the nearest double once (float(Fraction) rounds to nearest even) -- the header's "each product and each sum is
    rounded on its own", restated without a floating-point unit.  Comparisons are of doubles and need no rounding.  An operation with a
    NaN or an infinity among its operands is IEEE's own rule (no rounding is in question).  Stored as `det` [C][5][3]: the force without
    the gust term, which the oracle and the device must reproduce to the bit.
  * The branch every zone and event takes in every sample, asserted against the case's `expect`: what it was built to take.
  * Gusts in DPS = 50 digits with mpmath: the generator's integers (restated here), u1 and u2 (exact doubles), n = sqrt(-2 ln u1) cos(tp u2)
    with tp the double 6.283185307179586, g <- a g + c n and force = det + g, none of them rounded.  Stored as (hi, lo) pairs of doubles:
    `gust` [C][5][3][2] (g after each sample) and `force` [C][5][3][2].
  * tol_case [C]: the largest absolute error of tests/disturbance_oracle.py over a case's gust and force against these values, and never
    below FLOOR = 2^-52 times the largest magnitude among them and 1: one unit in the last place of the quantities compared
    (gen_estimator_mp.py's rule).  tests/test_gpu_disturbance.py allows the device tol_factor = 8 times that.  0 in a scene without gusts.
DATA only, fixed time stamps: a second run reproduces the file bit for bit.
"""
import math
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.tools.gen_tube_mp import write_npz      # noqa: E402
from tests import disturbance_cases as DC          # noqa: E402

DPS = 50
OUT = os.path.join(ROOT, "tests", "golden", "disturbance_mp.npz")
TOL_FACTOR = 8.0
M64 = 2 ** 64


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


def rop(op, a, b):
    """One IEEE operation on two doubles: exact in rationals, rounded once; IEEE's special values where an operand is not finite."""
    if math.isfinite(a) and math.isfinite(b) and not (op == "/" and b == 0.0):
        fa, fb = Fraction(a), Fraction(b)
        return float(fa + fb if op == "+" else fa - fb if op == "-" else fa * fb if op == "*" else fa / fb)
    return a + b if op == "+" else a - b if op == "-" else a * b if op == "*" else a / b


def finalise(x):
    """SplitMix64's finaliser on an integer mod 2^64, written with % (the oracle masks)."""
    x = (x + 11400714819323198485) % M64
    x = ((x ^ (x // 2 ** 30)) * 13787848793156543929) % M64
    x = ((x ^ (x // 2 ** 27)) * 10723151780598845931) % M64
    return x ^ (x // 2 ** 31)


def normal_mp(seed, ident, k, axis):
    mp = _mp()
    h = finalise((finalise((finalise(seed % M64) + ident) % M64) + k) % M64)
    r0, r1 = finalise((h + 2 * axis) % M64), finalise((h + 2 * axis + 1) % M64)
    u1 = mp.mpf(r0 // 2048 + 1) / mp.mpf(2) ** 53        # the double 9007199254740993.0 is 2^53
    u2 = mp.mpf(r1 // 2048) / mp.mpf(2) ** 53
    return mp.sqrt(-2 * mp.log(u1)) * mp.cos(mp.mpf(6.283185307179586) * u2)


def deterministic(pos, k, base, zones, events, t_epoch):
    """(force without gusts [3] as doubles, the branches) of one sample."""
    t = rop("+", t_epoch, rop("*", float(k), DC.DT))
    acc = [float(v) for v in base]
    br = []
    for row in zones:
        if not (row[10] <= t < row[11]):
            w = 0.0; br.append(DC.OFF)
        else:
            d = [rop("-", pos[i], row[i]) for i in range(3)] + [rop("-", row[3 + i], pos[i]) for i in range(3)]
            if not all(v >= 0.0 for v in d):
                w = 0.0; br.append(DC.OUT)
            else:
                m = min(d)                               # (all six are numbers here; equal values are the same double)
                if m >= row[9]:
                    w = 1.0; br.append(DC.FULL)
                else:
                    w = rop("/", m, row[9]); br.append(DC.RAMP)
        acc = [rop("+", acc[i], rop("*", w, row[6 + i])) for i in range(3)]
    for row in events:
        if row[0] <= t < row[1]:
            br.append(DC.EV_ON)
            acc = [rop("+", acc[i], row[2 + i]) for i in range(3)]
        else:
            br.append(DC.EV_OFF)
    return acc, tuple(br)


def split(x):
    hi = float(x)
    return hi, float(x - _mp().mpf(hi))


def main(argv):
    out = OUT
    for i, a in enumerate(argv):
        if a == "--out":
            out = argv[i + 1]
    from tests import disturbance_oracle as DO
    mp = _mp()
    store = {}
    names = []
    for sc in DC.scenes():
        name, E = sc["name"], sc["E"]
        names.append(name)
        arr = DC.arrays(sc)
        zones = [[float(v) for v in r] for r in sc["zones"]]
        gust = sc["gust"]
        a, c = DC.gust_coefficients(gust["sigma"], gust["tau"]) if gust else ([0.0] * 3, [0.0] * 3)
        det_all, G, Fo, tol_case = [], [], [], []
        for case in sc["cases"]:
            b, k0 = int(case["lane"]), int(case["tick0"])
            ev = [[float(v) for v in r] for r in case["events"]]
            g = [mp.mpf(float(v)) for v in case["g0"]]
            det, gs, fs, taken = [], [], [], []
            for s in range(DC.S_MAX):
                f, br = deterministic([float(v) for v in case["pos"][s]], k0 + s, case["base"], zones, ev, sc["t_epoch"])
                assert br == tuple(case["expect"][s]), (name, b, s, br, case["expect"][s])
                det.append(f)
                if gust:
                    n = [normal_mp(sc["seed"], (sc["id0"] + b) % M64, (k0 + s) % M64, i) for i in range(3)]
                    g = [mp.mpf(a[i]) * g[i] + mp.mpf(c[i]) * n[i] for i in range(3)]
                gs.append(list(g)); fs.append([mp.mpf(f[i]) + g[i] for i in range(3)])
            # the oracle: the same branches, the deterministic part to the bit, its error on the rest
            taken = []
            of, og, ot = DO.evaluate(case["pos"], k0, b, case["base"], zones, ev, list(case["g0"]) if gust else None, a, c, sc["seed"], sc["id0"], sc["t_epoch"], DC.DT, taken)
            assert ot == k0 + DC.S_MAX
            per = len(zones) + E + (1 if gust else 0)
            for s in range(DC.S_MAX):
                assert tuple(x for x in taken[s * per:(s + 1) * per] if x != DO.GUST) == tuple(case["expect"][s]), (name, b, s)
            if not gust:
                assert np.array_equal(np.array(of).view(np.uint64), np.array(det).view(np.uint64)), (name, b, of, det)
                tol_case.append(0.0)
            else:
                # g after every sample: the oracle's, replayed
                og_s, gg = [], list(case["g0"])
                for s in range(DC.S_MAX):
                    _, gg = DO.sample(case["pos"][s], k0 + s, b, case["base"], zones, ev, gg, a, c, sc["seed"], sc["id0"], sc["t_epoch"], DC.DT)
                    og_s.append(list(gg))
                assert og_s[-1] == og
                flat = lambda rows: [v for r in rows for v in r]
                fin = list(zip(flat(of) + flat(og_s), flat(fs) + flat(gs)))
                assert all(math.isfinite(o) for o, _ in fin)         # (a position that is not finite feels no zone: the force stays finite)
                err = max(abs(float(mp.mpf(o) - w)) for o, w in fin)
                floor = 2.0 ** -52 * max([1.0] + [abs(float(w)) for _, w in fin])
                tol_case.append(max(err, floor))
            det_all.append(det); G.append(gs); Fo.append(fs)
        pair = lambda rows: np.array([[[split(v) for v in r] for r in case] for case in rows])
        for k_, v_ in arr.items():
            store[f"{name}_{k_}"] = v_
        store[f"{name}_det"] = np.array(det_all, dtype=np.float64)
        store[f"{name}_tol_case"] = np.array(tol_case)
        store[f"{name}_scalars"] = np.array([sc["t_epoch"], DC.DT] + list(a) + list(c))
        store[f"{name}_ints"] = np.array([E, 1 if gust else 0, sc["seed"], sc["id0"]], dtype=np.int64)
        if gust:
            store[f"{name}_gust"] = pair(G)
            store[f"{name}_force"] = pair(Fo)
            print("%-10s %2d cases; oracle error: worst %.3e, smallest %.3e" % (name, len(tol_case), max(tol_case), min(tol_case)))
        else:
            print("%-10s %2d cases; the oracle reproduces the exact scheme to the bit" % (name, len(tol_case)))
    store["names"] = np.array(names)
    store["dps"] = np.array(DPS, dtype=np.int32)
    store["tol_factor"] = np.array(TOL_FACTOR)
    write_npz(out, store)
    print("-> %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1:])
