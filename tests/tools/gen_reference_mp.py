#!/usr/bin/env python3
"""Multiprecision reference of the stage references (getCurTraj + calculate_yaw) -> tests/golden/reference_mp.npz.

    python tests/tools/gen_reference_mp.py [--out FILE]

Written from the mathematics over the cases of tests/reference_cases.py; oracle/reference_oracle.py is not imported.  Every float64
input is taken as an exact rational, mpmath works at DPS digits.

PER STAGE i of a case (path [K,3], size, offset `off`, Ts, plan row 1 = position and seed yaw):
  discrete decisions, in exact arithmetic with fractions.Fraction, each IEEE operation rounded once (float(Fraction) rounds correctly):
    t   = fl(fl(i Ts) + off)                     the stage time
    q   = fl(t / Ts)          ki = trunc(q)      the sample;  q <= -1, q >= 2**31 - 1 or q not finite: the kernel's documented rule,
                                                 the END OF THE PATH for position and look-ahead (a "hostile" stage)
    w   = fl(fmod(t, Ts) / Ts)                   fmod is exact: t - trunc(t / Ts) Ts with the EXACT quotient, the sign of t
    interpolate when ki + 1 < size, look ahead to sample ki + 5 when ki + 5 < size, else the last sample (size clamped to [1, K])
  then in DPS digits, with w the double above:
    pos  = a + w (b - a)                         (exact rational, no rounding)
    far  = |fwd - pos| > 0.1                     0.1, 0.2, 0.8, PI = 3.1415926: the doubles the kernel holds, as exact rationals
    yaw_temp = atan2(dy, dx) if far else last;   D = yaw_temp - last
    unwrap: D > PI -> yaw_temp - 2 PI  (yaw_temp > 0),  D < -PI -> yaw_temp + 2 PI
    yaw  = 0.2 last + 0.8 yaw_temp';             last = yaw                 last starts from the seed yaw
  replan = |pos_0 - plan position| > 1.
Every threshold decision carries its margin: | |d| / 0.1 - 1 | and | dist / 1 - 1 |, relative to the threshold (the sqrt's error is
relative), and | |D| - PI | in radians (the atan2's error is absolute at these magnitudes).  The generator REFUSES a case with a margin
below MARGIN = 1e-9 (less one part in 1e6, so that a case placed AT 1e-9 stays), so that neither a faithfully rounded sqrt nor an
atan2 a few ulp off can take another branch.  One family is exempt, 'direction_exact': its look-ahead distance is the double 0.1 itself
(margin exactly 0, decided by the strict '>'), which is what tells '>' from '>='.

Stored: the inputs (paths, per case: path, size, offset, Ts, N, plan row 1), per stage ki, w, branch bits, margins, ref_pos and ref_yaw
as (hi float64, lo float32) pairs (hi + lo good to ~1e-23 relative), per case the replan flag and its margin.  DATA only, fixed time
stamps: a second run reproduces the file bit for bit.
"""
import io
import os
import sys
import zipfile
from fractions import Fraction as F

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import reference_cases as RC     # noqa: E402

DPS = 50
MARGIN = 1e-9
REFUSE = MARGIN * (1 - 1e-6)
OUT = os.path.join(ROOT, "tests", "golden", "reference_mp.npz")
B_INTERP, B_AHEAD, B_FAR, B_MINUS, B_PLUS, B_HOSTILE = 1, 2, 4, 8, 16, 32


def _mp():
    import mpmath
    mpmath.mp.dps = DPS + 10
    return mpmath


def fl(x):
    """A rational rounded to the nearest double, ties to even (int / int true division in CPython is correctly rounded)."""
    return x.numerator / x.denominator


def trunc(x):
    return int(x) if x >= 0 else -int(-x)      # Fraction.__int__ truncates towards zero already; spelled out


def decisions(c):
    """Per stage (ki or None, w, interp, ahead), exactly."""
    out = []
    Ts = F(c.Ts)
    size = c.eff_size
    for i in range(c.N):
        if c.off != c.off or c.off in (float("inf"), float("-inf")):
            out.append((None, 0.0, False, False))
            continue
        t = fl(F(fl(F(i) * Ts)) + F(c.off))
        q = fl(F(t) / Ts)
        if not (-1.0 < q < 2.0 ** 31 - 1.0):
            out.append((None, 0.0, False, False))
            continue
        ki = trunc(F(q))
        fm = F(t) - trunc(F(t) / Ts) * Ts
        w = fl(fm / Ts)
        out.append((ki, w, ki + 1 < size, ki + 5 < size))
    return out


def to_mp(mp, x):
    return mp.mpf(x.numerator) / mp.mpf(x.denominator)


def run_case(c):
    mp = _mp()
    size = c.eff_size
    path = [[F(float(v)) for v in row] for row in c.path]
    last_sample = path[size - 1]
    c01, c02, c08, PI = F(0.1), F(0.2), F(0.8), F(RC.PI)
    last = to_mp(mp, F(c.yaw0))
    rows = []
    replan = None
    for i, (ki, w, interp, ahead) in enumerate(decisions(c)):
        bits = 0
        if ki is None:
            bits |= B_HOSTILE
        if interp:
            a, b = path[ki], path[ki + 1]
            pos = [a[k] + F(w) * (b[k] - a[k]) for k in range(3)]
            bits |= B_INTERP
        else:
            pos = last_sample
        fwd = path[ki + 5] if ahead else last_sample
        bits |= B_AHEAD if ahead else 0
        d = [fwd[k] - pos[k] for k in range(3)]
        dist = mp.sqrt(to_mp(mp, d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
        m_far = abs(dist / to_mp(mp, c01) - 1)
        far = dist > to_mp(mp, c01)
        yaw_temp = mp.atan2(to_mp(mp, d[1]), to_mp(mp, d[0])) if far else last
        bits |= B_FAR if far else 0
        D = yaw_temp - last
        m_unwrap = abs(abs(D) - to_mp(mp, PI))
        yaw = yaw_temp
        if abs(D) > to_mp(mp, PI):
            if yaw_temp > 0:
                yaw, bits = yaw_temp - 2 * to_mp(mp, PI), bits | B_MINUS
            else:
                yaw, bits = yaw_temp + 2 * to_mp(mp, PI), bits | B_PLUS
        yaw = to_mp(mp, c02) * last + to_mp(mp, c08) * yaw
        last = yaw
        if i == 0:
            e = [pos[k] - F(float(c.pos1[k])) for k in range(3)]
            de = mp.sqrt(to_mp(mp, e[0] * e[0] + e[1] * e[1] + e[2] * e[2]))
            replan = (bool(de > 1), float(abs(de - 1)))
        for what, m in (("direction", m_far), ("unwrap", m_unwrap)):
            if m < REFUSE and not (c.family == "direction_exact" and what == "direction" and m == 0):
                raise SystemExit("case %s stage %d: %s margin %s below %g -- move the case" % (c.name, i, what, mp.nstr(m, 5), MARGIN))
        rows.append((-1 if ki is None else min(ki, 2 ** 31 - 1), w, bits, float(m_far), float(m_unwrap), [to_mp(mp, p) for p in pos], yaw))
    if replan[1] < REFUSE:
        raise SystemExit("case %s: replan margin %g below %g -- move the case" % (c.name, replan[1], MARGIN))

    def split(x):
        hi = float(x)
        return hi, float(x - mp.mpf(hi))
    ki = np.array([r[0] for r in rows], dtype=np.int32)
    w = np.array([r[1] for r in rows])
    bits = np.array([r[2] for r in rows], dtype=np.uint8)
    margins = np.array([[r[3], r[4]] for r in rows], dtype=np.float32)
    pos = np.array([[split(p) for p in r[5]] for r in rows])           # [N,3,2]
    yaw = np.array([split(r[6]) for r in rows])                        # [N,2]
    return ki, w, bits, margins, pos, yaw, replan


def write_npz(path, arrays):
    """np.savez_compressed with fixed member time stamps (zip members carry the wall clock otherwise)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main(argv):
    out = OUT
    for i, a in enumerate(argv):
        if a == "--out":
            out = argv[i + 1]
    cs = RC.cases()
    res = [run_case(c) for c in cs]
    N = np.array([c.N for c in cs], dtype=np.int32)
    pids = sorted(RC.PATHS)
    pK = np.array([len(RC.PATHS[p]) for p in pids], dtype=np.int32)
    cat = lambda j: np.concatenate([r[j] for r in res])
    pos, yaw = cat(4), cat(5)
    arrays = dict(
        dps=np.array(DPS, dtype=np.int32), margin=np.array(MARGIN),
        path_id=np.array(pids), path_K=pK, path_start=np.concatenate([[0], np.cumsum(pK)[:-1]]).astype(np.int32),
        paths=np.concatenate([RC.PATHS[p] for p in pids]),
        case_name=np.array([c.name for c in cs]), case_family=np.array([c.family for c in cs]), case_N=N,
        case_start=np.concatenate([[0], np.cumsum(N)[:-1]]).astype(np.int32), case_Ts=np.array([c.Ts for c in cs]),
        case_path=np.array([pids.index(c.path_id) for c in cs], dtype=np.int32),
        case_size=np.array([RC.NO_SIZE if c.size is None else c.size for c in cs], dtype=np.int32),
        case_off=np.array([c.off for c in cs]), case_pos1=np.stack([c.pos1 for c in cs]), case_yaw0=np.array([c.yaw0 for c in cs]),
        case_replan=np.array([r[6][0] for r in res], dtype=np.uint8), case_replan_margin=np.array([r[6][1] for r in res], dtype=np.float32),
        ki=cat(0), w=cat(1), branch=cat(2), margins=cat(3),
        pos_hi=pos[:, :, 0].copy(), pos_lo=pos[:, :, 1].astype(np.float32), yaw_hi=yaw[:, 0].copy(), yaw_lo=yaw[:, 1].astype(np.float32))
    write_npz(out, arrays)
    m = arrays["margins"]
    print("%d cases, %d stages, %d bytes; smallest margins: direction %.3g, unwrap %.3g, replan %.3g" % (
        len(cs), len(m), os.path.getsize(out), m[:, 0].min(), m[:, 1].min(), arrays["case_replan_margin"].min()))


if __name__ == "__main__":
    main(sys.argv[1:])
