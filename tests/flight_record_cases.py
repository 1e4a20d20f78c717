"""Synthetic cases of the flight record (tests/flight_record_oracle.py, include/frp_nmpc.h section 14) that take every branch of its rules:
a script of NV base vehicles over T samples and P period ends, played through any implementation of reset / samples / period (the oracle on
the CPU, the device in tests/test_gpu_flight_record.py) for B vehicles (the base tiled) in calls of S samples, and records for the
summary.  census() plays everything through the oracle and counts the branches; REQUIRED lists every branch, and none may stay empty."""
import collections

import numpy as np

from . import flight_record_oracle as FO

NAN, INF = float("nan"), float("inf")
T, P, NV = 10, 8, 48
S_VALUES = (1, 5)
KIND_NONE, KIND_TRAJ, KIND_END, KIND_YAW, KIND_NO_YAW_INPUT = 0, 1, 2, 3, -1
NAMES = ["clean_all_kinds", "no_x", "nan_p1", "inf_p1", "nan_v1", "inf_v1", "nan_cmd_tracked", "inf_cmd_tracked", "nan_cmd_untracked", "nan_x0", "inf_x0",
         "nan_first_no_x", "inactive_poisoned_a", "left_of_b", "inactive_poisoned_b", "never_tracked", "arrives_twice", "arrives_at_once", "never_arrives",
         "every_result", "every_gate", "every_state", "reset_again"] + ["sat_bit_%d" % i for i in range(10)]
NAMED = {n: i for i, n in enumerate(NAMES)}
assert len(NAMES) < NV


def script(seed=7):
    """The base vehicles: x0 [NV,9], with_x [NV], trace [NV,T,9], cmd [NV,T,16], kind / sat [NV,T], active [NV], the four period arrays [P,NV],
    again [NV] (who is reset once more at the end) and `poison`, the record's contents before the first reset."""
    rng = np.random.default_rng(seed)
    x0 = rng.normal(0.0, 2.0, (NV, 9))
    trace = rng.normal(0.0, 1.0, (NV, T, 9))
    trace[:, :, 0:3] = x0[:, None, 0:3] + np.cumsum(rng.normal(0.0, 0.02, (NV, T, 3)), axis=1)
    cmd = rng.normal(0.0, 1.0, (NV, T, 16))
    cmd[:, :, 0:3] = trace[:, :, 0:3] + rng.normal(0.0, 0.05, (NV, T, 3))
    kind = rng.choice([0, 1, 1, 1, 2, 3, -1], (NV, T)).astype(np.int32)
    sat = rng.choice([0, 0, 0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 3, 384, 512], (NV, T)).astype(np.int32)
    with_x = rng.integers(0, 2, NV).astype(np.int32)
    active = np.ones(NV, dtype=np.int32)
    state = rng.integers(0, 6, (P, NV)).astype(np.int32)
    gate = rng.choice([0, 0, 0, 1, 2, 3], (P, NV)).astype(np.int32)
    result = rng.choice([1, 1, 1, 0, -1, -2, -3, -4], (P, NV)).astype(np.int32)
    exit_code = rng.choice([1, 1, 0, -7, 2], (P, NV)).astype(np.int32)
    again = np.zeros(NV, dtype=np.int32)
    v = NAMED
    for n in NAMES[:12]:
        kind[v[n]] = KIND_TRAJ
        with_x[v[n]] = 1
    kind[v["clean_all_kinds"]] = [0, 1, 2, 3, -1, 1, 1, 2, 0, 1]
    with_x[v["no_x"]] = 0
    trace[v["nan_p1"], 3, 0] = NAN            # sample 3 is bad by p1, sample 4 by p0
    trace[v["inf_p1"], 4, 1] = INF
    trace[v["nan_v1"], 2, 4] = NAN
    trace[v["inf_v1"], 6, 5] = -INF
    cmd[v["nan_cmd_tracked"], 5, 1] = NAN
    cmd[v["inf_cmd_tracked"], 2, 2] = INF; kind[v["inf_cmd_tracked"], 2] = KIND_END
    cmd[v["nan_cmd_untracked"], 3, 0] = NAN; kind[v["nan_cmd_untracked"], 3] = KIND_NONE
    x0[v["nan_x0"], 1] = NAN                   # the first sample is bad by p0
    x0[v["inf_x0"], 2] = INF
    with_x[v["nan_first_no_x"]] = 0; trace[v["nan_first_no_x"], 0, 0] = NAN   # not bad: nothing to compare with; sample 1 is, by p0
    for n in ("inactive_poisoned_a", "inactive_poisoned_b"):
        active[v[n]] = 0
        trace[v[n]] = NAN; cmd[v[n]] = NAN; x0[v[n]] = NAN
    kind[v["never_tracked"]] = [0, 3, -1, 0, 3, -1, 0, 3, -1, 0]
    result[:, v["arrives_twice"]] = [1, 1, 0, 1, 1, 0, 1, 1]
    result[:, v["arrives_at_once"]] = [0, 1, 1, 1, 1, 1, 1, 1]
    result[:, v["never_arrives"]] = 1
    result[:, v["every_result"]] = [1, 0, -1, -2, -3, -4, 7, 1]
    gate[:, v["every_gate"]] = [0, 1, 2, 3, 0, 0, 1, 2]; exit_code[:, v["every_gate"]] = [1, 1, 1, 1, 0, -5, 0, 1]
    state[:, v["every_state"]] = [0, 1, 2, 3, 4, 5, 6, -1]
    again[v["reset_again"]] = 1
    for i in range(10):
        sat[v["sat_bit_%d" % i]] = 0
        sat[v["sat_bit_%d" % i], i % 5] = 1 << i          # (within the first half: the second is played with sat NULL)
    poison = FO.new(NV)
    for n in FO.FIELDS:
        a = poison[n]
        a[...] = rng.integers(1, 1000, a.shape) if a.dtype == np.int32 else rng.normal(0.0, 1e3, a.shape)
    poison["p_prev"][::5] = NAN
    return dict(x0=x0, with_x=with_x, trace=trace, cmd=cmd, kind=kind, sat=sat, active=active, state=state, gate=gate, result=result, exit_code=exit_code,
                again=again, poison=poison)


def tiled(sc, B):
    """The script for B vehicles: vehicle b is base vehicle b % NV."""
    idx = np.arange(B) % NV
    out = {n: np.ascontiguousarray(a[:, idx] if n in ("state", "gate", "result", "exit_code") else a[idx]) for n, a in sc.items() if n != "poison"}
    out["poison"] = {n: np.ascontiguousarray(a[idx]) for n, a in sc["poison"].items()}
    return out


class OracleApi:
    """The oracle behind the interface play() drives."""

    def __init__(self, broken=None, census=None):
        self.broken, self.census, self.rec = broken, census, None

    def load(self, rec):
        self.rec = FO.copy(rec)

    def reset(self, mask, x):
        FO.reset(self.rec, mask, x, census=self.census)

    def samples(self, trace, cmd, kind, sat, active):
        FO.samples(self.rec, trace, cmd, kind, sat, active, broken=self.broken, census=self.census)

    def period(self, state, gate, result, exit_code, active):
        FO.period(self.rec, state, gate, result, exit_code, active, census=self.census)

    def result(self):
        return self.rec


def play(api, sc, S):
    """The script through an implementation, in calls of S samples: the record starts as `poison`; those with with_x are reset to x0, the
    others without x; T samples, the first half with the sat words and the second with sat NULL; P period ends; `again` reset once more."""
    assert T % S == 0 and (T // 2) % S == 0
    api.load(sc["poison"])
    api.reset(sc["with_x"], sc["x0"])
    api.reset(1 - sc["with_x"], None)
    for c in range(T // S):
        w = slice(c * S, (c + 1) * S)
        sat = np.ascontiguousarray(sc["sat"][:, w]) if c * S < T // 2 else None
        api.samples(np.ascontiguousarray(sc["trace"][:, w]), np.ascontiguousarray(sc["cmd"][:, w]), np.ascontiguousarray(sc["kind"][:, w]), sat, sc["active"])
    for p in range(P):
        api.period(sc["state"][p], sc["gate"][p], sc["result"][p], sc["exit_code"][p], sc["active"])
    api.reset(sc["again"], None)
    return api.result()


# ---- records for the summary ----
SUMMARY_B = (1, 256, 257, 700)
SUMMARY_EDGES = (0, 1, 64)


def summary_record(B, seed=11):
    """(record, min_clear, hits): plausible accumulators of B vehicles, the float ones over eight decades so that the order of a sum shows."""
    rng = np.random.default_rng(seed + B)
    r = FO.new(B)
    r["track_n"][:] = np.where(rng.random(B) < 0.12, 0, rng.integers(1, 60, B))
    r["track_n"][0] = 7
    r["track_sum2"][:] = np.where(r["track_n"] > 0, 10.0 ** rng.uniform(-6, 2, B), 0.0)
    r["track_max2"][:] = r["track_sum2"] * rng.uniform(0.1, 1.0, B)
    r["path_len"][:] = 10.0 ** rng.uniform(-4, 3, B)
    r["speed_max2"][:] = rng.uniform(0.0, 9.0, B)
    for n in ("samples", "flown", "sat_samples", "periods", "ticks_run", "ticks_converged"):
        r[n][:] = rng.integers(0, 2000, B)
    r["bad"][:] = np.where(rng.random(B) < 0.2, rng.integers(1, 9, B), 0)
    r["result_hist"][:] = rng.integers(0, 300, (B, 6))
    r["state_hist"][:] = rng.integers(0, 300, (B, 6))
    r["first_arrival"][:] = np.where(rng.random(B) < 0.4, -1, rng.integers(0, 400, B))
    r["have_prev"][:] = 1
    min_clear = np.where(rng.random(B) < 0.3, INF, rng.uniform(0.1, 2.0, B))
    hits = np.where(rng.random(B) < 0.25, rng.integers(1, 5, B), 0).astype(np.int32)
    return r, min_clear, hits


def summary_mask(B, seed=13):
    """Vehicle 0 selected, the whole second workgroup (256 ... 511) not, the rest at random."""
    m = (np.random.default_rng(seed + B).random(B) < 0.7).astype(np.int32)
    m[256:512] = 0
    m[0] = 1
    return m


def summary_edges(r, n):
    """n ascending edges; from the first on, edges are the mean squared errors of vehicles with track_n > 0, exactly, so that those
    vehicles sit ON an edge (vehicle 0 always does for n >= 1)."""
    if n == 0:
        return np.zeros(0)
    tracked = np.nonzero(r["track_n"] > 0)[0]
    exact = sorted({float(r["track_sum2"][b]) / float(r["track_n"][b]) for b in tracked[:max(1, n // 8)]})
    fill = [e for e in (10.0 ** np.linspace(-7, 2, n)).tolist() if e not in exact]
    edges = np.array(sorted(exact + fill[:n - len(exact)]))
    assert len(edges) == n and np.all(np.diff(edges) > 0)
    return edges


REQUIRED = (["samples: inactive", "samples: a counted sat bit", "samples: no counted sat bit", "samples: sat NULL", "samples: not finite without have_prev",
             "samples: cmd not finite, not tracked", "samples: tracked", "samples: path only", "samples: first sample without p_prev",
             "samples: first sample with p_prev from reset", "reset: masked out", "reset: with x", "reset: without x", "period: inactive",
             "period: ran and converged", "period: ran, not converged", "period: state out of range", "period: first arrival", "period: a later arrival",
             "summary: lane out of range", "summary: unselected", "summary: on an edge", "summary: inside a bin", "summary: track_n == 0"]
            + ["samples: kind %d" % k for k in (-1, 0, 1, 2, 3)] + ["samples: sat bit %d" % i for i in range(10)]
            + ["samples: bad by %s %s" % (a, b) for a in ("p0", "p1", "v1", "cmd") for b in ("nan", "inf")]
            + ["period: gate %d" % g for g in range(4)] + ["period: result %d" % v for v in (1, 0, -1, -2, -3, -4, 7)] + ["period: state %d" % s for s in range(6)])


def census():
    """Every case of this file through the oracle: the branch counts."""
    c = collections.Counter()
    sc = script()
    for S in S_VALUES:
        play(OracleApi(census=c), sc, S)
    for B in SUMMARY_B:
        r, min_clear, hits = summary_record(B)
        for n in SUMMARY_EDGES:
            FO.summary(r, min_clear, hits, summary_mask(B), summary_edges(r, n), census=c)
    return c
