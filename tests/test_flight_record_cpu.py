"""CPU tests of the flight record (include/frp_nmpc.h section 14): the restatement tests/flight_record_oracle.py against hand-worked answers, the
census of tests/flight_record_cases.py (no branch stays empty), deliberately broken variants of the oracle each caught by a named case, and
the boundary of the built library without a device: the symbols, the struct, every FRP_ERR_ARG rule before any device call.
The record has no reference counterpart: the oracle is its specification."""
import ctypes
import os
import re

import numpy as np

from forces_resilient_planner_amd import capi, solver

from . import flight_record_cases as FC
from . import flight_record_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
NAMES = ["frp_nmpc_flight_record_samples", "frp_nmpc_flight_record_period", "frp_nmpc_flight_record_reset", "frp_nmpc_flight_summary_workspace_bytes",
         "frp_nmpc_flight_summary"]


# ---- hand-worked answers ----
def _one(trace, cmd, kind, sat=None, x=None):
    r = FO.new(1)
    FO.reset(r, None, None if x is None else np.array([list(x) + [0.0] * 6]))
    c = np.zeros((1, len(kind), 16)); c[0, :, 0:3] = cmd
    FO.samples(r, np.array([trace], dtype=np.float64), c, np.array([kind], dtype=np.int32), None if sat is None else np.array([sat], dtype=np.int32))
    return {n: a[0] for n, a in r.items()}


def test_the_sample_rule_against_hand_worked_numbers():
    trace = [(3, 4, 0, 1, 2, 2), (3, 4, 12, 0, 0, 0), (3, 4, 12, 0, 3, 4), (4, 4, 12, 0, 0, 0)]
    cmd = [(0, 0, 12), (9, 9, 9), (3, 0, 12), (3, 4, 10)]
    kind = [FC.KIND_TRAJ, FC.KIND_NONE, FC.KIND_END, FC.KIND_YAW]
    r = _one(trace, cmd, kind, sat=[0, 1 | 128, 256, 64], x=(0, 0, 0))
    # the error is the state BEFORE the sample against its setpoint: (0,0,0) - (0,0,12) and (3,4,12) - (3,0,12); the YAW sample tracks nothing
    assert r["track_sum2"] == 144.0 + 16.0 and r["track_max2"] == 144.0 and r["track_n"] == 2 and r["flown"] == 2
    assert r["path_len"] == 5.0 + 12.0 + 0.0 + 1.0 and r["speed_max2"] == 25.0 and r["samples"] == 4 and r["bad"] == 0
    assert r["sat_bits"] == (1 | 128 | 256 | 64) and r["sat_samples"] == 2          # ZERO_ACC and YAW_WRAP are not saturations
    assert r["p_prev"].tolist() == [4.0, 4.0, 12.0] and r["have_prev"] == 1
    # without x the first sample has nothing to compare with: no path, no error, but its speed counts and it was flown
    r = _one(trace, cmd, kind)
    assert r["track_sum2"] == 16.0 and r["track_n"] == 1 and r["flown"] == 2 and r["path_len"] == 12.0 + 0.0 + 1.0 and r["speed_max2"] == 25.0
    assert r["sat_bits"] == 0 and r["sat_samples"] == 0 and r["samples"] == 4
    # a NaN position: that sample and the next are bad, they are flown all the same, and nothing of them enters a sum
    bad = [trace[0], (NAN, 4, 12, 9, 9, 9), trace[2], trace[3]]
    r = _one(bad, cmd, [FC.KIND_TRAJ] * 4, x=(0, 0, 0))
    assert r["bad"] == 2 and r["flown"] == 4 and r["samples"] == 4 and r["track_n"] == 2 and r["track_sum2"] == 144.0 + 4.0 and r["path_len"] == 5.0 + 1.0
    assert r["speed_max2"] == 9.0                                                  # (1, 2, 2) and (0, 0, 0): the bad samples' speeds are not looked at
    # every product is rounded on its own: 1 + 2^-53 squared is 1 + 2^-52 + 2^-106, and the sum with the tiny square rounds it away
    e = 1.0 + 2.0 ** -52
    r = _one([(e, 2.0 ** -30, 0, 0, 0, 0)], [(0, 0, 0)], [FC.KIND_TRAJ], x=(e, 2.0 ** -30, 0))
    assert r["track_sum2"] == (e * e + 2.0 ** -60) + 0.0 and r["path_len"] == 0.0


def test_the_period_rule_against_hand_worked_numbers():
    r = FO.new(2)
    seq = [(5, 0, 1, 1), (4, 0, -2, -7), (1, 2, 0, 1), (1, 1, -4, 1), (9, 0, 0, 1), (3, 3, -1, 0)]   # state, gate, result, exit_code
    for st, g, res, ex in seq:
        FO.period(r, [st, st], [g, g], [res, res], [ex, ex], active=[1, 0])
    a = {n: v[0] for n, v in r.items()}
    assert a["periods"] == 6 and a["ticks_run"] == 3 and a["ticks_converged"] == 2 and a["first_arrival"] == 2
    assert a["result_hist"].tolist() == [1, 2, 1, 1, 0, 1] and a["state_hist"].tolist() == [0, 2, 0, 1, 1, 1]
    assert FO.same({n: v[1:] for n, v in r.items()}, {n: v[1:] for n, v in FO.new(2).items()})     # the inactive one is untouched
    x = np.arange(18.0).reshape(2, 9)
    FO.reset(r, [1, 0], x)
    assert r["periods"].tolist() == [0, 0] and r["first_arrival"].tolist() == [-1, -1] and r["have_prev"].tolist() == [1, 0] and r["p_prev"][0].tolist() == [0.0, 1.0, 2.0]


def test_the_summary_against_hand_worked_numbers():
    r = FO.new(3)
    u = 2.0 ** -53
    r["track_sum2"][:] = [u, u, 1.0]; r["track_n"][:] = [1, 2, 0]; r["path_len"][:] = [1.0, 2.0, 4.0]; r["track_max2"][:] = [u, u, 0.0]
    r["speed_max2"][:] = [4.0, 9.0, 1.0]; r["samples"][:] = [5, 6, 7]; r["bad"][:] = [0, 3, 0]; r["first_arrival"][:] = [4, -1, 6]
    r["result_hist"][:] = [[1, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0], [0, 0, 0, 0, 0, 3]]
    ints, floats, hist = FO.summary(r, edges=[u / 2, u])
    # the tree: lane 0 + lane 2 first (stride 2: u + 1 rounds to 1), then + lane 1 (1 + u rounds to 1); left to right it is 2u + 1 > 1
    assert floats[FO.F_TRACK_SUM2] == 1.0 and FO.tree_sum([u, u, 1.0] + [0.0] * 253, broken="tree_left_to_right") == 1.0 + 2 * u
    assert floats[FO.F_PATH_SUM] == 7.0 and floats[FO.F_PATH_MAX] == 4.0 and floats[FO.F_SPEED_MAX2] == 9.0 and floats[FO.F_TRACK_MAX2] == u
    assert floats[FO.F_MIN_CLEAR] == INF
    assert hist.tolist() == [0, 1, 1]                  # means u (ON the upper edge: the bin above it) and u / 2 (on the lower: the middle bin)
    assert ints[FO.I_SELECTED] == 3 and ints[FO.I_ARRIVED] == 2 and ints[FO.I_WITH_BAD] == 1 and ints[FO.I_WITH_HITS] == 0 and ints[FO.I_SAMPLES] == 18
    assert ints[FO.I_BAD] == 3 and ints[FO.I_ARRIVAL_SUM] == 10 and ints[FO.I_RESULT:FO.I_RESULT + 6].tolist() == [1, 2, 0, 0, 0, 3]
    ints, floats, hist = FO.summary(r, min_clear=[0.5, 0.25, INF], hits=[0, 2, 0], mask=[1, 0, 1])
    assert ints[FO.I_SELECTED] == 2 and ints[FO.I_WITH_HITS] == 0 and floats[FO.F_MIN_CLEAR] == 0.5 and floats[FO.F_PATH_SUM] == 5.0 and hist.tolist() == [1]
    # partials of workgroups are added in their order
    big = FO.new(513)
    big["path_len"][[0, 256, 512]] = [1.0, u, u]
    assert FO.summary(big)[1][FO.F_PATH_SUM] == 1.0 and FO.summary(big, mask=(np.arange(513) > 0).astype(int))[1][FO.F_PATH_SUM] == 2 * u


# ---- the cases ----
def test_no_branch_of_the_rules_stays_empty():
    c = FC.census()
    empty = [n for n in FC.REQUIRED if c[n] == 0]
    assert not empty, empty
    assert set(c) >= set(FC.REQUIRED) and len(set(FC.REQUIRED)) == len(FC.REQUIRED)


def test_one_call_of_five_samples_is_five_calls_of_one_and_the_named_cases_do_what_they_are_named_for():
    sc = FC.script()
    r1, r5 = (FC.play(FC.OracleApi(), sc, S) for S in (1, 5))
    assert FO.same(r1, r5)
    v = FC.NAMED
    row = lambda n: {k: a[v[n]] for k, a in r5.items()}
    assert row("nan_p1")["bad"] == 2 and row("inf_p1")["bad"] == 2 and row("nan_v1")["bad"] == 1 and row("inf_v1")["bad"] == 1
    assert row("nan_cmd_tracked")["bad"] == 1 and row("inf_cmd_tracked")["bad"] == 1 and row("nan_cmd_untracked")["bad"] == 0
    assert row("nan_x0")["bad"] == 1 and row("inf_x0")["bad"] == 1 and row("nan_first_no_x")["bad"] == 1
    for n in FC.NAMES[:12]:
        a = row(n)
        untracked = int(np.sum((sc["kind"][v[n]] != FC.KIND_TRAJ) & (sc["kind"][v[n]] != FC.KIND_END)))
        assert np.isfinite([a["track_sum2"], a["track_max2"], a["path_len"], a["speed_max2"]]).all() and a["samples"] == FC.T == a["flown"] + untracked, n
        assert a["track_n"] == FC.T - untracked - a["bad"] - (n in ("no_x", "nan_first_no_x")), n
    for n in ("inactive_poisoned_a", "inactive_poisoned_b"):
        a = row(n)
        assert a["samples"] == 0 and a["periods"] == 0 and a["first_arrival"] == -1 and a["track_sum2"] == 0.0 and a["bad"] == 0
    assert row("never_tracked")["track_n"] == 0 and row("never_tracked")["flown"] == 0 and row("never_tracked")["path_len"] > 0.0
    assert row("arrives_twice")["first_arrival"] == 2 and row("arrives_at_once")["first_arrival"] == 0 and row("never_arrives")["first_arrival"] == -1
    assert row("every_result")["result_hist"].tolist() == [2, 1, 1, 1, 1, 2] and row("every_state")["state_hist"].tolist() == [1] * 6
    assert row("every_gate")["ticks_run"] == 3 and row("every_gate")["ticks_converged"] == 1
    assert row("reset_again")["samples"] == 0 and row("reset_again")["have_prev"] == 0
    for i in range(10):
        a = row("sat_bit_%d" % i)
        assert a["sat_bits"] == 1 << i and a["sat_samples"] == (1 if i < 7 else 0), i


def test_deliberately_broken_variants_are_each_caught_by_a_named_case():
    assert set(FO.BROKEN) == {"error_after_the_sample", "edge_greater_than", "bad_sample_enters_the_sums", "tree_left_to_right"}
    sc = FC.script()
    good = FC.play(FC.OracleApi(), sc, 5)
    v = FC.NAMED
    after = FC.play(FC.OracleApi(broken="error_after_the_sample"), sc, 5)
    assert after["track_sum2"][v["clean_all_kinds"]] != good["track_sum2"][v["clean_all_kinds"]] and after["track_n"][v["clean_all_kinds"]] == good["track_n"][v["clean_all_kinds"]]
    enters = FC.play(FC.OracleApi(broken="bad_sample_enters_the_sums"), sc, 5)
    assert np.isnan(enters["track_sum2"][v["nan_p1"]]) and np.isnan(enters["path_len"][v["nan_p1"]]) and np.isfinite(good["track_sum2"][v["nan_p1"]])
    assert enters["track_n"][v["nan_p1"]] == good["track_n"][v["nan_p1"]] + 2
    for b in ("error_after_the_sample", "bad_sample_enters_the_sums"):      # ... and both leave every other rule alone
        w = FC.play(FC.OracleApi(broken=b), sc, 5)
        assert all(np.array_equal(w[n], good[n]) for n in ("samples", "flown", "bad", "sat_bits", "periods", "result_hist", "first_arrival"))
    # summary, B = 257, one edge: vehicle 0 sits on it
    r, min_clear, hits = FC.summary_record(257)
    edges = FC.summary_edges(r, 1)
    assert edges[0] == r["track_sum2"][0] / r["track_n"][0]
    want, got = FO.summary(r, min_clear, hits, None, edges), FO.summary(r, min_clear, hits, None, edges, broken="edge_greater_than")
    assert got[2][0] == want[2][0] + 1 and got[2][1] == want[2][1] - 1 and np.array_equal(got[0], want[0]) and np.array_equal(FO.bits(got[1]), FO.bits(want[1]))
    # summary, B = 256, one full workgroup: the order of the sum shows in its last bits
    r, min_clear, hits = FC.summary_record(256)
    want, got = FO.summary(r, min_clear, hits), FO.summary(r, min_clear, hits, broken="tree_left_to_right")
    assert not np.array_equal(FO.bits(got[1][4:]), FO.bits(want[1][4:])) and np.array_equal(FO.bits(got[1][:4]), FO.bits(want[1][:4])) and np.array_equal(got[0], want[0])
    assert np.allclose(got[1][4:], want[1][4:], rtol=1e-12, atol=0.0)


# ---- the boundary, without a device ----
def _has_gpu():
    try:
        return solver.lib().frp_nmpc_device_count() > 0
    except Exception:
        return False


def test_the_five_calls_are_declared_where_the_issue_puts_them():
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    assert solver.EXPORTS[-len(NAMES):] == NAMES and all(hasattr(solver.lib(), n) for n in NAMES)
    assert "#define FRP_NMPC_ABI_VERSION 7" in hdr and solver.ABI_VERSION == 7 and "(14)" in hdr and hdr.rindex('#include "frp_nmpc_') < hdr.index("(14)")
    assert re.findall(r"^(?:int|size_t) (frp_nmpc_flight_\w+)\(", hdr, flags=re.M) == NAMES
    assert not os.path.exists(os.path.join(ROOT, "include", "frp_nmpc_flight.h"))
    assert capi.C_TYPES[capi.FlightRecordArgs] == ("frp_nmpc_flight_record", "frp_nmpc.h") and [f for f, _ in capi.FlightRecordArgs._fields_[1:]] == list(FO.FIELDS)
    for n in ("GROUP", "RESULT_BINS", "STATE_BINS", "MAX_EDGES", "SAT_MASK", "SUM_INTS", "SUM_F64", "I_SELECTED", "I_ARRIVED", "I_WITH_BAD", "I_WITH_HITS", "I_SAMPLES",
              "I_FLOWN", "I_TRACK_N", "I_BAD", "I_SAT_SAMPLES", "I_PERIODS", "I_TICKS_RUN", "I_TICKS_CONVERGED", "I_RESULT", "I_ARRIVAL_SUM", "F_TRACK_MAX2",
              "F_SPEED_MAX2", "F_PATH_MAX", "F_MIN_CLEAR", "F_TRACK_SUM2", "F_PATH_SUM"):
        assert getattr(FO, n) == getattr(solver, "FLIGHT_" + n) and capi.MACROS["FLIGHT_" + n] == "FRP_FLIGHT_" + n, n
    assert FO.SAT_MASK == (solver.VEHICLE_SAT_THRUST_LO | solver.VEHICLE_SAT_THRUST_HI | solver.VEHICLE_SAT_ROLL | solver.VEHICLE_SAT_PITCH | solver.VEHICLE_SAT_RATE0 * 7)
    assert (FO.TRAJ, FO.END, FO.TICK_RUN) == (solver.COMMAND_TRAJ, solver.COMMAND_END, solver.TICK_RUN)
    assert (FC.KIND_NONE, FC.KIND_YAW, FC.KIND_NO_YAW_INPUT) == (solver.COMMAND_NONE, solver.COMMAND_YAW, solver.COMMAND_NO_YAW_INPUT)
    assert solver.FlightRecord.__module__.endswith(".flight") and "frp_flight_record.hip" in __import__("forces_resilient_planner_amd.build", fromlist=["x"]).SOURCES


def _rec(B=4, **kw):
    a = {f: 0x1000 * (i + 1) for i, (f, _) in enumerate(capi.FlightRecordArgs._fields_[1:])}     # the addresses are never dereferenced on the host
    a.update(kw)
    return capi.FlightRecordArgs(B, *[a[f] for f, _ in capi.FlightRecordArgs._fields_[1:]])


GOOD = dict(samples=dict(S=5, trace=0x100000, stride=9, cmd=0x200000, kind=0x300000, sat=0x400000, active=0x500000),
            period=dict(fsm_state=0x100000, gate=0x200000, result=0x300000, exit_code=0x400000, active=0x500000),
            reset=dict(mask=0x100000, x=0x200000),
            summary=dict(min_clear=0x100000, hits=0x200000, mask=0x300000, n_edges=4, edges=0x400000, out_i=0x500000, out_f=0x600000, hist=0x700000,
                         workspace=0x800000, workspace_bytes=None))


def _call(which, rec="good", B=4, rec_kw=None, **kw):
    l = solver.lib()
    r = _rec(B, **(rec_kw or {}))
    p = None if rec is None else ctypes.byref(r)
    a = dict(GOOD[which]); a.update(kw)
    if which == "samples":
        return l.frp_nmpc_flight_record_samples(p, a["S"], a["trace"], a["stride"], a["cmd"], a["kind"], a["sat"], a["active"], None)
    if which == "period":
        return l.frp_nmpc_flight_record_period(p, a["fsm_state"], a["gate"], a["result"], a["exit_code"], a["active"], None)
    if which == "reset":
        return l.frp_nmpc_flight_record_reset(p, a["mask"], a["x"], None)
    ws = l.frp_nmpc_flight_summary_workspace_bytes(B) if a["workspace_bytes"] is None else a["workspace_bytes"]
    return l.frp_nmpc_flight_summary(p, a["min_clear"], a["hits"], a["mask"], a["n_edges"], a["edges"], a["out_i"], a["out_f"], a["hist"], a["workspace"], ws, None)


def test_every_bad_argument_is_refused_before_any_device_call():
    """Without a device a call that passes the argument checks answers FRP_ERR_NO_DEVICE, so FRP_ERR_ARG here was decided before any device
    call; with a device the same order holds and the good calls are not made here (their addresses are not memory)."""
    ARG, NODEV = solver.FRP_ERR_ARG, solver.FRP_ERR_NO_DEVICE
    l = solver.lib()
    row = 8 * (FO.SUM_INTS + FO.MAX_EDGES + 1 + FO.SUM_F64)
    assert [l.frp_nmpc_flight_summary_workspace_bytes(B) for B in (-1, 0, 1, 256, 257, 4096)] == [0, row, row, row, 2 * row, 16 * row]
    for which in GOOD:
        assert _call(which, rec=None) == ARG, which
        assert _call(which, B=-1, workspace_bytes=1 << 20) == ARG, which
        for f, _ in capi.FlightRecordArgs._fields_[1:]:
            assert _call(which, rec_kw={f: None}) == ARG, (which, f)
    for bad in (dict(trace=None), dict(cmd=None), dict(kind=None), dict(S=0), dict(S=-1), dict(stride=5), dict(stride=0), dict(stride=-9)):
        assert _call("samples", **bad) == ARG, bad
    assert _call("samples", B=1 << 20, S=1 << 8, stride=8) == ARG and _call("samples", B=(1 << 31) - 1, S=1, stride=6) == ARG      # B * S * stride = 2^31
    assert _call("samples", B=1 << 16, S=1 << 16, stride=6) == ARG
    for f in ("fsm_state", "gate", "result", "exit_code"):
        assert _call("period", **{f: None}) == ARG, f
    for bad in (dict(n_edges=-1), dict(n_edges=65), dict(edges=None), dict(min_clear=None), dict(hits=None), dict(out_i=None), dict(out_f=None), dict(hist=None),
                dict(workspace=None), dict(workspace_bytes=row - 1), dict(workspace_bytes=0)):
        assert _call("summary", **bad) == ARG, bad
    assert _call("summary", B=257, workspace_bytes=2 * row - 1) == ARG
    if not _has_gpu():
        for which in GOOD:
            assert _call(which) == NODEV and _call(which, B=0) == NODEV and _call(which, B=1) == NODEV, which
        assert _call("samples", sat=None, active=None, S=1, stride=6) == NODEV and _call("samples", B=1 << 20, S=5, stride=409) == NODEV   # 2^31 - 1 - 2^20 * 3
        assert _call("period", active=None) == NODEV and _call("reset", mask=None, x=None) == NODEV
        assert _call("summary", min_clear=None, hits=None, mask=None, n_edges=0, edges=None) == NODEV and _call("summary", n_edges=64) == NODEV
        assert _call("summary", n_edges=0, edges=0x9000) == NODEV and _call("summary", B=257, workspace_bytes=2 * row) == NODEV


def test_the_python_object_refuses_what_it_cannot_launch():
    """FlightRecord's checks that need no device: the trace fallback's error and the edge limit are raised before any call."""
    import types
    fake = types.SimpleNamespace(trace=None, estimator=None, sat=None, x=None, torch=None, B=4)
    rec = solver.FlightRecord.__new__(solver.FlightRecord)
    rec.torch, rec.vehicle, rec.clearance, rec.B = None, fake, None, 4
    try:
        rec.update_samples(types.SimpleNamespace(cmd=None, kind=None))
        raise AssertionError("no trace: expected a ValueError")
    except ValueError as e:
        assert "keeps no trace" in str(e) and "ForceEstimator" in str(e)
    try:
        rec.summary(edges=np.zeros(65))
        raise AssertionError("65 edges: expected a ValueError")
    except ValueError as e:
        assert "64" in str(e)
    assert solver.FlightRecord is __import__("forces_resilient_planner_amd.flight", fromlist=["x"]).FlightRecord
