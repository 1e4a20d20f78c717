"""The flight record (include/frp_nmpc.h section 14, csrc/frp_flight_record.hip) restated in plain NumPy and Python floats: the three update
rules and the fleet summary with its addition order.  It has no reference counterpart: this file is the specification the device is held
to, bit for bit -- every product, sum, quotient and square root below is one IEEE double operation, in the order the header writes it.

A record is a dict of arrays named as the fields of frp_nmpc_flight_record.  `census`, where given, is a collections.Counter that counts
the branches taken (tests/flight_record_cases.py asserts that none stays empty).  `broken` names a deliberately wrong variant (BROKEN):
tests/test_flight_record_cpu.py shows that each is caught by a named case."""
import math

import numpy as np

TRAJ, END = 1, 2                      # FRP_COMMAND_TRAJ, FRP_COMMAND_END
TICK_RUN = 0                          # FRP_TICK_RUN
SAT_MASK = 1 | 2 | 4 | 8 | 16 | 32 | 64   # THRUST_LO, THRUST_HI, ROLL, PITCH, RATE0 << 0, 1, 2
RESULT_BINS, STATE_BINS, GROUP, MAX_EDGES = 6, 6, 256, 64
SUM_INTS, SUM_F64 = 19, 6
(I_SELECTED, I_ARRIVED, I_WITH_BAD, I_WITH_HITS, I_SAMPLES, I_FLOWN, I_TRACK_N, I_BAD, I_SAT_SAMPLES, I_PERIODS, I_TICKS_RUN, I_TICKS_CONVERGED,
 I_RESULT) = range(13)
I_ARRIVAL_SUM = 18
F_TRACK_MAX2, F_SPEED_MAX2, F_PATH_MAX, F_MIN_CLEAR, F_TRACK_SUM2, F_PATH_SUM = range(6)
BROKEN = ("error_after_the_sample", "edge_greater_than", "bad_sample_enters_the_sums", "tree_left_to_right")

I32 = ("have_prev", "track_n", "samples", "flown", "bad", "sat_samples", "sat_bits", "periods", "ticks_run", "ticks_converged", "first_arrival")
F64 = ("track_max2", "track_sum2", "path_len", "speed_max2")
FIELDS = ("p_prev", "have_prev", "track_max2", "track_sum2", "track_n", "path_len", "speed_max2", "samples", "flown", "bad", "sat_samples", "sat_bits",
          "periods", "ticks_run", "ticks_converged", "result_hist", "state_hist", "first_arrival")


def new(B):
    r = {n: np.zeros(B, dtype=np.int32) for n in I32}
    r.update({n: np.zeros(B, dtype=np.float64) for n in F64})
    r["p_prev"] = np.zeros((B, 3))
    r["result_hist"], r["state_hist"] = np.zeros((B, RESULT_BINS), dtype=np.int32), np.zeros((B, STATE_BINS), dtype=np.int32)
    r["first_arrival"][:] = -1
    return r


def copy(r):
    return {n: a.copy() for n, a in r.items()}


def _count(census, what):
    if census is not None:
        census[what] += 1


def _finite3(v):
    return all(math.isfinite(c) for c in v)


def _sq3(x, y, z):
    return (x * x + y * y) + z * z


def reset(r, mask=None, x=None, census=None):
    for b in range(len(r["samples"])):
        if mask is not None and mask[b] == 0:
            _count(census, "reset: masked out")
            continue
        for n in I32 + F64:
            r[n][b] = 0
        r["result_hist"][b] = 0
        r["state_hist"][b] = 0
        r["first_arrival"][b] = -1
        if x is not None:
            r["p_prev"][b] = x[b][0:3]
            r["have_prev"][b] = 1
            _count(census, "reset: with x")
        else:
            _count(census, "reset: without x")


def samples(r, trace, cmd, kind, sat=None, active=None, broken=None, census=None):
    """trace [B,S,>=6], cmd [B,S,16], kind [B,S], sat [B,S] or None, active [B] or None."""
    B, S = kind.shape
    for b in range(B):
        if active is not None and active[b] == 0:
            _count(census, "samples: inactive")
            continue
        p0 = [float(v) for v in r["p_prev"][b]]
        have = int(r["have_prev"][b])
        tmax, tsum, plen, vmax = (float(r[n][b]) for n in ("track_max2", "track_sum2", "path_len", "speed_max2"))
        tn, n, flown, bad, satn, bits = (int(r[k][b]) for k in ("track_n", "samples", "flown", "bad", "sat_samples", "sat_bits"))
        for s in range(S):
            p1 = [float(v) for v in trace[b, s, 0:3]]
            v1 = [float(v) for v in trace[b, s, 3:6]]
            c = [float(v) for v in cmd[b, s, 0:3]]
            k = int(kind[b, s])
            tracked = k in (TRAJ, END)
            _count(census, "samples: kind %d" % k)
            n += 1
            if sat is not None:
                w = int(sat[b, s])
                bits |= w
                if w & SAT_MASK:
                    satn += 1
                    _count(census, "samples: a counted sat bit")
                else:
                    _count(census, "samples: no counted sat bit")
                for i in range(32):
                    if w >> i & 1:
                        _count(census, "samples: sat bit %d" % i)
            else:
                _count(census, "samples: sat NULL")
            is_bad = False
            if have:
                for name, vec, applies in (("p0", p0, True), ("p1", p1, True), ("v1", v1, True), ("cmd", c, tracked)):
                    if applies and not _finite3(vec):
                        is_bad = True
                        _count(census, "samples: bad by " + name + (" nan" if any(math.isnan(q) for q in vec) else " inf"))
            elif not (_finite3(p1) and _finite3(v1)):
                _count(census, "samples: not finite without have_prev")
            if not tracked and not _finite3(c):
                _count(census, "samples: cmd not finite, not tracked")
            if is_bad:
                bad += 1
            if not is_bad or broken == "bad_sample_enters_the_sums":
                if have:
                    plen += math.sqrt(_sq3(p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]))
                    if tracked:
                        q = p1 if broken == "error_after_the_sample" else p0
                        e2 = _sq3(q[0] - c[0], q[1] - c[1], q[2] - c[2])
                        tsum += e2
                        tmax = e2 if e2 > tmax else tmax
                        tn += 1
                        _count(census, "samples: tracked")
                    else:
                        _count(census, "samples: path only")
                else:
                    _count(census, "samples: first sample without p_prev")
                v2 = _sq3(v1[0], v1[1], v1[2])
                vmax = v2 if v2 > vmax else vmax
            if tracked:
                flown += 1
            if have and s == 0 and int(r["samples"][b]) == 0:
                _count(census, "samples: first sample with p_prev from reset")
            p0, have = p1, 1
        r["p_prev"][b] = p0
        r["have_prev"][b] = have
        for name, v in (("track_max2", tmax), ("track_sum2", tsum), ("path_len", plen), ("speed_max2", vmax), ("track_n", tn), ("samples", n), ("flown", flown),
                        ("bad", bad), ("sat_samples", satn), ("sat_bits", bits)):
            r[name][b] = v


def result_bin(result):
    return 1 - result if -3 <= result <= 1 else RESULT_BINS - 1


def period(r, fsm_state, gate, result, exit_code, active=None, census=None):
    for b in range(len(r["periods"])):
        if active is not None and active[b] == 0:
            _count(census, "period: inactive")
            continue
        r["periods"][b] += 1
        _count(census, "period: gate %d" % gate[b])
        if gate[b] == TICK_RUN:
            r["ticks_run"][b] += 1
            if exit_code[b] == 1:
                r["ticks_converged"][b] += 1
                _count(census, "period: ran and converged")
            else:
                _count(census, "period: ran, not converged")
        res, st = int(result[b]), int(fsm_state[b])
        r["result_hist"][b, result_bin(res)] += 1
        _count(census, "period: result %d" % res)
        if 0 <= st < STATE_BINS:
            r["state_hist"][b, st] += 1
            _count(census, "period: state %d" % st)
        else:
            _count(census, "period: state out of range")
        if res == 0:
            if r["first_arrival"][b] < 0:
                r["first_arrival"][b] = r["periods"][b] - 1
                _count(census, "period: first arrival")
            else:
                _count(census, "period: a later arrival")


def tree_sum(v, broken=None):
    """The header's order over one workgroup's GROUP values."""
    v = [float(x) for x in v]
    assert len(v) == GROUP
    if broken == "tree_left_to_right":
        s = 0.0
        for x in v:
            s += x
        return s
    stride = GROUP // 2
    while stride >= 1:
        for i in range(stride):
            v[i] += v[i + stride]
        stride //= 2
    return v[0]


def mean_bin(m, edges, broken=None):
    if broken == "edge_greater_than":
        return sum(1 for e in edges if e < m)
    return sum(1 for e in edges if e <= m)


def summary(r, min_clear=None, hits=None, mask=None, edges=(), broken=None, census=None):
    """-> (ints [SUM_INTS] int64, floats [SUM_F64] float64, hist [len(edges) + 1] int64)"""
    B = len(r["samples"])
    edges = [float(e) for e in edges]
    assert len(edges) <= MAX_EDGES and (min_clear is None) == (hits is None)
    ints, hist = [0] * SUM_INTS, [0] * (len(edges) + 1)
    fmax, cmin, sums = [0.0, 0.0, 0.0], math.inf, [0.0, 0.0]
    for g in range((B + GROUP - 1) // GROUP):
        lanes = [[0.0] * GROUP, [0.0] * GROUP]
        for t in range(GROUP):
            b = g * GROUP + t
            if b >= B:
                _count(census, "summary: lane out of range")
                continue
            if mask is not None and mask[b] == 0:
                _count(census, "summary: unselected")
                continue
            fa, tn = int(r["first_arrival"][b]), int(r["track_n"][b])
            ints[I_SELECTED] += 1
            ints[I_ARRIVED] += fa >= 0
            ints[I_WITH_BAD] += int(r["bad"][b]) > 0
            ints[I_WITH_HITS] += hits is not None and int(hits[b]) > 0
            for i, n in ((I_SAMPLES, "samples"), (I_FLOWN, "flown"), (I_TRACK_N, "track_n"), (I_BAD, "bad"), (I_SAT_SAMPLES, "sat_samples"), (I_PERIODS, "periods"),
                         (I_TICKS_RUN, "ticks_run"), (I_TICKS_CONVERGED, "ticks_converged")):
                ints[i] += int(r[n][b])
            for k in range(RESULT_BINS):
                ints[I_RESULT + k] += int(r["result_hist"][b, k])
            ints[I_ARRIVAL_SUM] += fa if fa >= 0 else 0
            for i, n in enumerate(("track_max2", "speed_max2", "path_len")):
                v = float(r[n][b])
                fmax[i] = v if v > fmax[i] else fmax[i]
            if min_clear is not None:
                v = float(min_clear[b])
                cmin = v if v < cmin else cmin
            lanes[0][t], lanes[1][t] = float(r["track_sum2"][b]), float(r["path_len"][b])
            if tn > 0:
                m = float(r["track_sum2"][b]) / float(tn)
                hist[mean_bin(m, edges, broken)] += 1
                _count(census, "summary: on an edge" if m in edges else "summary: inside a bin")
            else:
                _count(census, "summary: track_n == 0")
        for i in range(2):                      # the second launch: the partials in workgroup order, from 0.0
            sums[i] = sums[i] + tree_sum(lanes[i], broken)
    floats = fmax + [cmin] + sums
    return np.array(ints, dtype=np.int64), np.array(floats, dtype=np.float64), np.array(hist, dtype=np.int64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Whether two records are equal, the doubles bit for bit; p_prev only where have_prev says it is valid."""
    for n in FIELDS:
        if n == "p_prev":
            v = np.asarray(a["have_prev"]) != 0
            if not np.array_equal(bits(a[n])[v], bits(b[n])[v]):
                return False
        elif a[n].dtype == np.float64:
            if not np.array_equal(bits(a[n]), bits(b[n])):
                return False
        elif not np.array_equal(a[n], b[n]):
            return False
    return True
