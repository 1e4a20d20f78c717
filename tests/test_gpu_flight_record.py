"""GPU tests of the flight record (include/frp_nmpc.h section 14, csrc/frp_flight_record.hip, solver.FlightRecord) against
tests/flight_record_oracle.py, BIT FOR BIT throughout: the integers are exact, and so are the float accumulators -- the order of every sum is
stated, the unit is built without contraction, and the device's FP64 square root is correctly rounded.  The synthetic cases of
tests/flight_record_cases.py through the three updates and the reset with a tail workgroup of 1 and of 44, one call of five samples against
five of one, the summary over one to three workgroups with and without mask, edges and clearance arrays, the three calls replayed from a
hipGraph, and the record kept over a closed-loop flight of the estimator test's fleet with nothing copied to the host inside the loop."""
import math
import types

import numpy as np
import pytest

from forces_resilient_planner_amd import layout as L, solver, workloads

from . import flight_record_cases as FC
from . import flight_record_oracle as FO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _vehicle(n, S=5, trace=True):
    """A solver.Vehicle for n vehicles without a fleet behind it (the class reads the fleet's size and device alone)."""
    import torch
    fleet = types.SimpleNamespace(torch=torch, B=n, solver=types.SimpleNamespace(device=torch.device(DEV)))
    return solver.Vehicle(fleet, trace=trace, S=S)


def _load(rec, arrays):
    for n in FO.FIELDS:
        getattr(rec, n).copy_(_dev(arrays[n], arrays[n].dtype))


class DeviceApi:
    """solver.FlightRecord behind the interface flight_record_cases.play() drives."""

    def __init__(self, B):
        self.rec = solver.FlightRecord(_vehicle(B))

    def load(self, arrays):
        _load(self.rec, arrays)

    def reset(self, mask, x):
        self.rec.reset(_dev(mask, np.int32), None if x is None else _dev(x, np.float64))

    def samples(self, trace, cmd, kind, sat, active):
        cmds = solver.Commands(_dev(cmd, np.float64), _dev(kind, np.int32), None, None, None)
        self.rec.update_samples(cmds, trace=_dev(trace, np.float64), sat=None if sat is None else _dev(sat, np.int32), active=_dev(active, np.int32))

    def period(self, state, gate, result, exit_code, active):
        i = lambda a: _dev(a, np.int32)
        self.rec.update_period(types.SimpleNamespace(state=i(state), tick=types.SimpleNamespace(gate=i(gate), result=i(result), exit_code=i(exit_code))), active=i(active))

    def result(self):
        return self.rec.arrays()


@pytest.fixture(scope="module")
def script():
    return FC.script()


def _differences(got, want):
    return [n for n in FO.FIELDS if not FO.same({**want, n: got[n]}, want)]


# ---- the three updates and the reset ----
@pytest.mark.parametrize("S", FC.S_VALUES)
@pytest.mark.parametrize("B", [1, 257, 300])
def test_a_updates_and_reset_equal_the_oracle_on_the_synthetic_cases(script, B, S):
    sc = FC.tiled(script, B)
    want = FC.play(FC.OracleApi(), sc, S)
    got = FC.play(DeviceApi(B), sc, S)
    assert not _differences(got, want), _differences(got, want)
    idle = sc["active"] == 0                                   # NaN-poisoned, inactive: as the resets left them
    if idle.any():
        assert np.all(got["samples"][idle] == 0) and np.all(got["periods"][idle] == 0) and np.all(got["track_sum2"][idle] == 0.0)


def test_b_one_call_of_five_samples_equals_five_calls_of_one(script):
    sc = FC.tiled(script, 300)
    one, five = FC.play(DeviceApi(300), sc, 1), FC.play(DeviceApi(300), sc, 5)
    assert not _differences(one, five), _differences(one, five)
    assert int(five["bad"].sum()) > 0 and int(five["track_n"].sum()) > 0 and float(five["path_len"].max()) > 0.0


def test_c_the_object_finds_the_trace_or_says_that_there_is_none():
    import torch
    B, S = 3, 5
    cmds = solver.Commands(torch.zeros((B, S, 16), dtype=torch.float64, device=DEV), torch.ones((B, S), dtype=torch.int32, device=DEV), None, None, None)
    bare = _vehicle(B, trace=False)
    with pytest.raises(ValueError, match="keeps no trace"):
        solver.FlightRecord(bare).update_samples(cmds)
    est = solver.ForceEstimator(bare)
    est.meas.fill_(1.0)
    rec = solver.FlightRecord(bare)
    rec.reset(x=bare.x)
    rec.update_samples(cmds)                                  # the estimator's meas: p = v = (1, 1, 1), setpoint 0, from p_prev = 0
    a = rec.arrays()
    assert a["samples"].tolist() == [S] * B and a["speed_max2"].tolist() == [3.0] * B and a["track_sum2"].tolist() == [0.0 + 4 * 3.0] * B
    assert a["path_len"].tolist() == [math.sqrt(3.0)] * B and a["sat_bits"].tolist() == [0] * B
    own = _vehicle(B, trace=True)
    own.trace.fill_(2.0); own.sat.fill_(solver.VEHICLE_SAT_ROLL)
    rec = solver.FlightRecord(own)
    rec.update_samples(cmds)                                  # the vehicle's own trace, and with it its sat words
    a = rec.arrays()
    assert a["sat_bits"].tolist() == [solver.VEHICLE_SAT_ROLL] * B and a["sat_samples"].tolist() == [S] * B and a["speed_max2"].tolist() == [12.0] * B
    assert list(rec.speed_max) == [math.sqrt(12.0)] * B and list(rec.track_max) == [math.sqrt(12.0)] * B and list(rec.track_rms) == [math.sqrt(12.0)] * B


# ---- the summary ----
@pytest.mark.parametrize("B", FC.SUMMARY_B)
def test_d_summary_equals_the_oracle_in_the_stated_order(B):
    r, min_clear, hits = FC.summary_record(B)
    veh = _vehicle(B)
    clear = types.SimpleNamespace(B=B, min_clear=_dev(min_clear, np.float64), hits=_dev(hits, np.int32))
    recs = {False: solver.FlightRecord(veh), True: solver.FlightRecord(veh, clearance=clear)}
    for rec in recs.values():
        _load(rec, r)
    mask = FC.summary_mask(B)
    assert B < 512 or not mask[256:512].any()                   # a whole workgroup without a selected vehicle
    d_mask = _dev(mask, np.int32)
    for n in FC.SUMMARY_EDGES:
        edges = FC.summary_edges(r, n)
        d_edges = _dev(edges, np.float64) if n else None
        for m, dm in ((None, None), (mask, d_mask)):
            for with_clear, rec in recs.items():
                want = FO.summary(r, min_clear if with_clear else None, hits if with_clear else None, m, edges)
                runs = []
                for _ in range(2):                               # the same bits on every run
                    s = rec.summary(mask=dm, edges=d_edges)
                    runs.append((s.ints.cpu().numpy(), s.floats.cpu().numpy(), s.hist.cpu().numpy()))
                for got in runs:
                    what = (B, n, m is not None, with_clear)
                    assert got[2].shape == (n + 1,) and np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]), (what, got[0], want[0], got[2], want[2])
                    assert np.array_equal(FO.bits(got[1]), FO.bits(want[1])), (what, got[1], want[1])
                assert int(want[2].sum()) == int(((r["track_n"] > 0) & (np.ones(B, int) if m is None else m != 0)).sum())
    assert np.isinf(FO.summary(r)[1][FO.F_MIN_CLEAR]) and FO.summary(r, min_clear, hits)[0][FO.I_WITH_HITS] == int((hits > 0).sum())


# ---- the three launches in a graph ----
def test_e_samples_period_and_summary_replayed_from_a_hipgraph_equal_eager_launches(script):
    """Captured once on one stream with the default queue count; replayed three times with new contents of every input."""
    import torch
    B, S = 300, 5
    sc = FC.tiled(script, B)
    f64, i32 = dict(dtype=torch.float64, device=DEV), dict(dtype=torch.int32, device=DEV)
    edges = _dev(10.0 ** np.linspace(-4, 1, 9), np.float64)

    def make():
        veh = _vehicle(B, S)
        rec = solver.FlightRecord(veh)
        cmds = solver.Commands(torch.zeros((B, S, 16), **f64), torch.zeros((B, S), **i32), None, None, None)
        fsm = types.SimpleNamespace(state=torch.zeros((B,), **i32), tick=types.SimpleNamespace(gate=torch.zeros((B,), **i32), result=torch.zeros((B,), **i32),
                                                                                              exit_code=torch.zeros((B,), **i32)))
        return rec, cmds, fsm, torch.zeros((B,), **i32), torch.zeros((B,), **i32)

    def chain(rec, cmds, fsm, active, mask, stream=None):
        rec.update_samples(cmds, active=active, stream=stream)
        rec.update_period(fsm, active=active, stream=stream)
        rec.summary(mask=mask, edges=edges, stream=stream)

    def run(rec, cmds, fsm, active, mask, fn):
        rec.reset(x=_dev(sc["x0"], np.float64))
        res = []
        for k in range(3):
            roll = lambda a, axis=0: np.roll(a, 7 * k, axis=axis)
            w = slice(k * 2, k * 2 + S)
            rec.vehicle.trace.copy_(_dev(roll(sc["trace"][:, w]), np.float64)); rec.vehicle.sat.copy_(_dev(roll(sc["sat"][:, w]), np.int32))
            cmds.cmd.copy_(_dev(roll(sc["cmd"][:, w]), np.float64)); cmds.kind.copy_(_dev(roll(sc["kind"][:, w]), np.int32))
            fsm.state.copy_(_dev(sc["state"][k], np.int32)); fsm.tick.gate.copy_(_dev(sc["gate"][k], np.int32))
            fsm.tick.result.copy_(_dev(sc["result"][k], np.int32)); fsm.tick.exit_code.copy_(_dev(sc["exit_code"][k], np.int32))
            active.copy_(_dev(roll(sc["active"]), np.int32)); mask.copy_(_dev(roll(FC.summary_mask(B)), np.int32))
            fn()
            torch.cuda.synchronize()
            res.append((rec.arrays(), rec.sum_ints.cpu().numpy(), rec.sum_floats.cpu().numpy(), rec.sum_hist.cpu().numpy()))
        return res

    a = make()
    ref = run(*a, lambda: chain(*a))
    assert int(ref[-1][1][FO.I_SAMPLES]) > 0 and int(ref[-1][3].sum()) > 0 and int(ref[-1][0]["bad"].sum()) > 0
    g_ = make()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        chain(*g_, side)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        chain(*g_, torch.cuda.current_stream())
    torch.cuda.synchronize()
    got = run(*g_, g.replay)
    for k, (p, q) in enumerate(zip(got, ref)):
        assert not _differences(p[0], q[0]), (k, _differences(p[0], q[0]))
        assert np.array_equal(p[1], q[1]) and np.array_equal(FO.bits(p[2]), FO.bits(q[2])) and np.array_equal(p[3], q[3]), k
    # ... and the eager launches are the oracle's
    want = FO.new(B)
    FO.reset(want, None, sc["x0"])
    for k in range(3):
        roll = lambda a: np.roll(a, 7 * k, axis=0)
        w = slice(k * 2, k * 2 + S)
        act = roll(sc["active"])
        FO.samples(want, roll(sc["trace"][:, w]), roll(sc["cmd"][:, w]), roll(sc["kind"][:, w]), roll(sc["sat"][:, w]), act)
        FO.period(want, sc["state"][k], sc["gate"][k], sc["result"][k], sc["exit_code"][k], act)
        assert not _differences(ref[k][0], want), (k, _differences(ref[k][0], want))
        s = FO.summary(want, None, None, roll(FC.summary_mask(B)), edges.cpu().numpy())
        assert np.array_equal(ref[k][1], s[0]) and np.array_equal(FO.bits(ref[k][2]), FO.bits(s[1])) and np.array_equal(ref[k][3][:10], s[2]), k


# ---- a closed-loop flight: the fleet of test_gpu_estimator's closed loop ----
WEIGHTS = (15.0, 3.0, 80.0, 15.0, 0.0)
FB, S_LOOP = 8, 5
PERIODS = 120
FORCE_AT = 20
FORCED = {1: (1.5, 0.0, 0.0), 6: (0.0, -1.8, 0.0)}
LANES = np.array([-8.05, -6.55, -5.05, -3.55, -2.05, 2.05, 3.55])


def _layout():
    """Seven planners fly 3 m along x in lanes of their own, planner 7 flies 5 m past the pillar at the origin."""
    start = np.zeros((FB, 9)); goal = np.zeros((FB, 3))
    start[:7, 0] = -6.05; start[:7, 1] = LANES; goal[:7, 0] = -3.05; goal[:7, 1] = LANES
    start[7, 0:2] = (-2.55, 0.05); goal[7, 0:2] = (2.55, 0.05)
    start[:, 2] = 1.2; goal[:, 2] = 1.2
    d = goal[:, 0:2] - start[:, 0:2]
    start[:, 8] = np.arctan2(d[:, 1], d[:, 0])
    return start, goal


def _fly(recorded):
    """PERIODS periods of FleetFSM.period(force=est.force, force_fresh=est.fresh, vehicle=veh).  recorded: a FlightRecord is updated after
    every period and NOTHING is copied to the host inside the loop; returns its arrays.  Otherwise the same flight with every period's
    inputs of the record kept in device rings, read back after the loop."""
    import torch
    w = workloads.astar_world(0, "empty", allocate_num=12000)
    dm = solver.OccupancyMap(w)
    pillar = np.array([(x, y, z) for x in np.arange(-0.25, 0.26, 0.1) for y in np.arange(-0.25, 0.26, 0.1) for z in np.arange(-0.95, 2.96, 0.1)], dtype=np.float32)
    dm.insert_cloud(pillar)
    fleet = solver.DeviceFleet(FB, 20, 30, 64, L.MODEL_NORMAL, WEIGHTS, weights_final=WEIGHTS)
    fleet.poly_index = torch.zeros((FB, 20), dtype=torch.int32, device=DEV)
    fsm = solver.FleetFSM(fleet)
    pl = solver.AstarPlanner(dm, FB, K=512)
    fsm.bind(pl)
    cloud = _dev(pillar.astype(np.float64), np.float64)
    veh = solver.Vehicle(fleet, trace=True, S=S_LOOP)
    est = solver.ForceEstimator(veh)
    rec = solver.FlightRecord(veh)
    start, goal = _layout()
    veh.reset(_dev(start, np.float64))
    veh.odometry(fsm)
    rec.reset(x=veh.x)
    f64, i32 = dict(dtype=torch.float64, device=DEV), dict(dtype=torch.int32, device=DEV)
    d_goal, fresh_goal = _dev(goal, np.float64), torch.zeros((FB,), **i32)
    clock = torch.zeros((3,), **f64)
    ring = dict(trace=torch.zeros((PERIODS, FB, S_LOOP, 9), **f64), cmd=torch.zeros((PERIODS, FB, S_LOOP, 16), **f64), kind=torch.zeros((PERIODS, FB, S_LOOP), **i32),
                sat=torch.zeros((PERIODS, FB, S_LOOP), **i32), state=torch.zeros((PERIODS, FB), **i32), gate=torch.zeros((PERIODS, FB), **i32),
                result=torch.zeros((PERIODS, FB), **i32), exit_code=torch.zeros((PERIODS, FB), **i32))
    f_step = np.zeros((FB, 3))
    for b, f in FORCED.items():
        f_step[b] = f
    d_step, ones, zeros = _dev(f_step, np.float64), torch.ones((FB,), **i32), torch.zeros((FB,), **i32)
    clocks = [_dev(solver.FleetFSM.clock_for(0.05 * k, 1), np.float64) for k in range(PERIODS)]
    torch.cuda.synchronize()
    for k in range(PERIODS):                                                   # ---- nothing is copied to the host in here ----
        fresh_goal.copy_(ones if k == 0 else zeros)
        if k == FORCE_AT:
            veh.f_true.copy_(d_step)
        clock.copy_(clocks[k])
        cmds = fsm.period(pl, dm, None, clock, cloud, goal=d_goal, goal_fresh=fresh_goal, force=est.force, force_fresh=est.fresh, fsm_steps=1, vehicle=veh)
        if recorded:
            rec.update_samples(cmds)
            rec.update_period(fsm)
        else:
            for n, t in (("trace", veh.trace), ("cmd", cmds.cmd), ("kind", cmds.kind), ("sat", veh.sat), ("state", fsm.state), ("gate", fsm.tick.gate),
                         ("result", fsm.tick.result), ("exit_code", fsm.tick.exit_code)):
                ring[n][k].copy_(t)
    torch.cuda.synchronize()
    if recorded:
        s = rec.summary()
        return rec.arrays(), (s.ints.cpu().numpy(), s.floats.cpu().numpy(), s.hist.cpu().numpy()), (rec.track_rms, rec.track_max, rec.speed_max)
    return {n: t.cpu().numpy() for n, t in ring.items()}, start


def test_f_the_record_of_a_closed_loop_flight_is_the_oracles():
    got, summ, roots = _fly(True)
    h, start = _fly(False)
    want = FO.new(FB)
    FO.reset(want, None, start)
    for k in range(PERIODS):
        FO.samples(want, h["trace"][k], h["cmd"][k], h["kind"][k], h["sat"][k])
        FO.period(want, h["state"][k], h["gate"][k], h["result"][k], h["exit_code"][k])
    print("first_arrival", got["first_arrival"].tolist(), "track_n", got["track_n"].tolist(), "flown", got["flown"].tolist())
    print("rms tracking error", np.round(roots[0], 4).tolist(), "max", np.round(roots[1], 4).tolist(), "max speed", np.round(roots[2], 3).tolist())
    print("path", np.round(got["path_len"], 3).tolist(), "sat_bits", got["sat_bits"].tolist(), "ticks run / converged", got["ticks_run"].tolist(), got["ticks_converged"].tolist())
    assert not _differences(got, want), _differences(got, want)
    assert (got["first_arrival"] >= 0).any() and (got["bad"] == 0).all() and (got["flown"] > 0).all()
    assert (got["samples"] == PERIODS * S_LOOP).all() and (got["periods"] == PERIODS).all() and (got["path_len"] > 0.0).all()
    s = FO.summary(want)
    assert np.array_equal(summ[0], s[0]) and np.array_equal(FO.bits(summ[1]), FO.bits(s[1])) and np.array_equal(summ[2], s[2])
    assert np.array_equal(FO.bits(roots[1]), FO.bits(np.sqrt(want["track_max2"]))) and np.array_equal(FO.bits(roots[2]), FO.bits(np.sqrt(want["speed_max2"])))
