#!/usr/bin/env python3
"""The flight record (include/frp_nmpc.h section 14, solver.FlightRecord) -> profiles/flight_record_bench.json.
    python tools/flight_record_bench.py [B=4096] [replays=40] [out=...]
  * update_samples(), update_period() and summary() for B vehicles with S = 5: eager, windows of back-to-back calls between two events.
  * What the three calls (four launches) add to the replayed period graph of tools/estimator_bench.py's baseline (tick, command timer, six
    state-machine kernels, a vehicle that traces): the graph without them and the graph with them, captured in this run, replayed
    ALTERNATELY from the same start state; medians and spread.
Recorded, not asserted anywhere.  No device: the tool fails."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from forces_resilient_planner_amd import layout as L  # noqa: E402
from forces_resilient_planner_amd import solver  # noqa: E402

DEV = "cuda:0"


def stat(a):
    return {"median": float(np.median(a)), "min": float(np.min(a)), "max": float(np.max(a)), "std": float(np.std(a)), "n": len(a)}


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def run(B=4096, REPLAYS=40):
    assert torch.cuda.is_available(), "flight_record_bench needs a GPU"
    N, M, F, K, S, N_SUB = 20, 30, 64, 120, 5, 4
    rng = np.random.default_rng(0)
    s = np.arange(K) * 0.05 * 1.6
    path = np.c_[s, 0.4 * np.sin(0.8 * s), 1.0 + 0.1 * np.cos(s)]
    cloud = np.c_[rng.uniform(-3, 12, 20000), rng.uniform(-4, 4, 20000), rng.uniform(-0.5, 3, 20000)]
    cx = np.interp(cloud[:, 0], path[:, 0], path[:, 1]); cz = np.interp(cloud[:, 0], path[:, 0], path[:, 2])
    cloud = cloud[np.hypot(cloud[:, 1] - cx, cloud[:, 2] - cz) > 0.9]
    plan = np.zeros((B, N + 1, 17)); plan[..., 3] = 7.3; plan[..., 7] = 7.3
    plan[..., 8:11] = path[0] + rng.normal(0, 0.02, (B, 1, 3)); plan[..., 16] = 0.2
    fleet = solver.DeviceFleet(B, N, M, F, L.MODEL_NORMAL, (15.0, 3.0, 80.0, 15.0, 0.0), weights_final=(15.0, 3.0, 80.0, 15.0, 0.0))
    fleet.poly_index = torch.zeros((B, N), dtype=torch.int32, device=DEV)
    d_plan, d_path, d_cloud = fleet.to_device(plan), fleet.to_device(path), fleet.to_device(cloud)
    x_start = fleet.to_device(plan[:, 1, 8:17].copy())
    grid = solver.CloudGrid(d_cloud, 0.5)
    toff = fleet.to_device(rng.uniform(0, 0.01, B))
    fsm = solver.FleetFSM(fleet)
    ts = fsm.tick
    ts.path_size(K)
    veh = solver.Vehicle(fleet, n_sub=N_SUB, trace=True, S=S)
    veh.f_true.copy_(fleet.to_device(rng.normal(0, 0.5, (B, 3))))
    rec = solver.FlightRecord(veh)
    edges = fleet.to_device(10.0 ** np.linspace(-6, 1, 16))
    d_state = veh.state
    i32 = lambda v: torch.full((B,), v, dtype=torch.int32, device=DEV)
    goal, fresh = fleet.to_device(np.tile(path[-1], (B, 1))), i32(0)
    fresh[::16] = 1
    force = fleet.to_device(rng.normal(0, 0.5, (B, 3)))
    ffresh, blocked, first_hit = i32(1), i32(0), i32(-1)
    now = fleet.to_device(np.array([1.0]))
    t_step = fleet.to_device(np.full(B, 0.06))
    t_cmd = fleet.to_device(np.tile(0.01 * np.arange(1, S + 1), (B, 1)))
    bufs = [torch.zeros((B, 3), dtype=torch.float64, device=DEV) for _ in range(5)]
    status = i32(solver.ASTAR_REACH_END)
    out = None

    def reset_state():
        fleet.mpc_output.copy_(d_plan); fleet.solver.exitflag.fill_(1); fleet.solver.iters.zero_(); fleet.mode.zero_()
        for k in ("fail_count", "replan_count", "kino_replan", "pub_end"):
            getattr(ts, k).zero_()
        ts.initialized.fill_(1); ts.exit_code.fill_(1); ts.cmd_status.fill_(solver.CMD_PUB_TRAJ); ts.exec_mpc.fill_(1)
        for k in fsm.INT_FIELDS:
            getattr(fsm, k).zero_()
        fsm.state.fill_(solver.FSM_EXEC_TRAJ); fsm.have_odom.fill_(1); fsm.have_target.fill_(1); fsm.have_traj.fill_(1); fsm.consider_force.fill_(1)
        fsm.end_pt.copy_(goal); fsm.external_acc.zero_(); fsm.last_external_acc.zero_()
        veh.reset(x_start); veh.state.copy_(x_start)
        rec.reset(x=x_start)

    def record(stream=None):
        rec.update_samples(out, stream=stream)
        rec.update_period(fsm, stream=stream)
        rec.summary(edges=edges, stream=stream)

    def chain(with_record, stream):
        nonlocal out
        fsm.goal(goal, fresh, stream); fsm.force(force, ffresh, stream); fsm.safety_verdict(blocked, first_hit, stream)
        fsm.exec_begin(d_state, t_step, now, *bufs, stream=stream); fsm.exec_end(status, now, stream)
        fleet.full_tick(fsm.external_acc, d_path, toff, d_cloud, fsm.ref_pos, fsm.ref_yaw, stream=stream, grid=grid, state=d_state, tick=ts, end_pt=fsm.end_pt)
        fsm.mpc_result(stream=stream)
        out = fleet.commands(t_cmd, ts.cmd_status, ts.pub_end, ts.cmd_end_pt, odom=fsm.yaw_odom, init_yaw=fsm.init_yaw, t_yaw=t_cmd, out=out, stream=stream)
        veh.step(out, stream)
        veh.odometry(fsm, stream=stream)
        if with_record:
            record(stream)

    reset_state()
    side = torch.cuda.Stream()
    graphs = {}
    for w in (False, True):
        with torch.cuda.stream(side):
            chain(w, side)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            chain(w, torch.cuda.current_stream())
        graphs[w] = g
    times = {False: [], True: []}
    for r in range(REPLAYS + 5):
        for w in (False, True):
            reset_state()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); graphs[w].replay(); e1.record(); torch.cuda.synchronize()
            if r >= 5:
                times[w].append(e0.elapsed_time(e1))
    ints, floats = rec.sum_ints.cpu().numpy(), rec.sum_floats.cpu().numpy()
    seen = dict(selected=int(ints[solver.FLIGHT_I_SELECTED]), samples=int(ints[solver.FLIGHT_I_SAMPLES]), flown=int(ints[solver.FLIGHT_I_FLOWN]),
                tracked=int(ints[solver.FLIGHT_I_TRACK_N]), bad=int(ints[solver.FLIGHT_I_BAD]), periods=int(ints[solver.FLIGHT_I_PERIODS]),
                ticks_run=int(ints[solver.FLIGHT_I_TICKS_RUN]), track_sum2=float(floats[solver.FLIGHT_F_TRACK_SUM2]), path_sum=float(floats[solver.FLIGHT_F_PATH_SUM]),
                hist=rec.sum_hist[:17].cpu().numpy().tolist())
    eager = {}
    calls = {"update_samples": lambda: rec.update_samples(out), "update_period": lambda: rec.update_period(fsm), "summary": lambda: rec.summary(edges=edges),
             "all_three": record}
    for _ in range(3):
        for fn in calls.values():
            window(fn, 5)
    for name, fn in calls.items():
        eager[name] = dict(stat([window(fn, 200) for _ in range(5)]), calls_per_window=200)
    added = float(np.median(times[True]) - np.median(times[False]))
    spread = float(max(np.std(times[False]), np.std(times[True])))
    return {"device": torch.cuda.get_device_name(0),
            "workload": f"{B} planners, N = {N}, the period of tools/estimator_bench.py's baseline (tick, command timer S = {S}, six state-machine kernels, vehicle "
                        f"n_sub = {N_SUB}, trace on); the record takes the vehicle's trace and sat words, 16 histogram edges",
            "in_period_graph_ms": {"period_and_vehicle": stat(times[False]), "period_vehicle_and_record": stat(times[True]), "added_ms_median": added,
                                   "largest_std_of_a_replay_ms": spread, "added_is_below_the_spread": bool(abs(added) < spread), "replays_each": REPLAYS,
                                   "kernels_added": 4,
                                   "what": "two captured graphs replayed alternately in this run, same start state; the baseline is the graph without update_samples(), "
                                           "update_period() and summary(); the added time is a difference of medians; recorded, not asserted"},
            "eager_ms_per_call": dict(eager, what="back-to-back calls between two events, ctypes marshalling included; summary() is two launches"),
            "what_the_last_replay_saw": seen}


if __name__ == "__main__":
    a = sys.argv[1:]
    res = run(int(a[0]) if len(a) > 0 else 4096, int(a[1]) if len(a) > 1 else 40)
    out = a[2] if len(a) > 2 else os.path.join(ROOT, "profiles", "flight_record_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
