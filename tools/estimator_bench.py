#!/usr/bin/env python3
"""The force estimator (include/frp_nmpc_estimator.h, solver.ForceEstimator) for a fleet: what it adds to the replayed graph of a period.
   python tools/estimator_bench.py [B=4096] [replays=40] [out=profiles/estimator_bench.json]
Two captured graphs: the period with the vehicle as it was (the chain of tools/vehicle_bench.py: the six state-machine kernels around
full_tick(tick=...) and the command timer, S = 5, then Vehicle.step (n_sub = 4) -> message -> odometry; the force callback reads a tensor
the host wrote), and the same with a ForceEstimator attached: the observed step instead of the plain one, one more launch (the update), and
the force callback reading the estimator's force / fresh.  Replayed alternately by that tool's method (`replays` pairs, plans and state
reset before each, the vehicle and the estimator put back on their start state); the baseline is the graph WITHOUT the estimator; the
added time is the difference of the two medians and is recorded next to the spread of a replay -- it is not asserted anywhere.
No device: the tool fails."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from forces_resilient_planner_amd import layout as L  # noqa: E402
from forces_resilient_planner_amd import solver  # noqa: E402


def run(B=4096, REPLAYS=40):
    assert torch.cuda.is_available(), "estimator_bench needs a GPU"
    dev = "cuda:0"
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
    fleet.poly_index = torch.zeros((B, N), dtype=torch.int32, device=dev)
    d_plan, d_path, d_cloud = fleet.to_device(plan), fleet.to_device(path), fleet.to_device(cloud)
    x_start = fleet.to_device(plan[:, 1, 8:17].copy())
    grid = solver.CloudGrid(d_cloud, 0.5)
    toff = fleet.to_device(rng.uniform(0, 0.01, B))
    fsm = solver.FleetFSM(fleet)
    ts = fsm.tick
    ts.path_size(K)
    veh = solver.Vehicle(fleet, n_sub=N_SUB)
    veh.f_true.copy_(fleet.to_device(rng.normal(0, 0.5, (B, 3))))
    est = solver.ForceEstimator(veh)
    veh.estimator = None                                                 # attached per graph, below
    d_state = veh.state                                                  # both graphs read the odometry from the same tensor
    i32 = lambda v: torch.full((B,), v, dtype=torch.int32, device=dev)
    goal, fresh = fleet.to_device(np.tile(path[-1], (B, 1))), i32(0)
    fresh[::16] = 1
    force = fleet.to_device(rng.normal(0, 0.5, (B, 3)))
    ffresh, blocked, first_hit = i32(1), i32(0), i32(-1)
    now = fleet.to_device(np.array([1.0]))
    t_step = fleet.to_device(np.full(B, 0.06))
    t_cmd = fleet.to_device(np.tile(0.01 * np.arange(1, S + 1), (B, 1)))
    bufs = [torch.zeros((B, 3), dtype=torch.float64, device=dev) for _ in range(5)]
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
        veh.estimator = None
        veh.reset(x_start); veh.state.copy_(x_start)
        # the estimator as a period in flight finds it: a previous measurement, a fresh estimate (the same for every replay)
        est.reset(); est.y_prev.copy_(x_start); est.count.fill_(est.min_samples); est.f_hat.copy_(force); est.force.copy_(force); est.fresh.fill_(1)

    def chain(with_estimator, stream):
        nonlocal out
        veh.estimator = est if with_estimator else None
        f_in, f_fresh = (est.force, est.fresh) if with_estimator else (force, ffresh)
        fsm.goal(goal, fresh, stream); fsm.force(f_in, f_fresh, stream); fsm.safety_verdict(blocked, first_hit, stream)
        fsm.exec_begin(d_state, t_step, now, *bufs, stream=stream); fsm.exec_end(status, now, stream)
        fleet.full_tick(fsm.external_acc, d_path, toff, d_cloud, fsm.ref_pos, fsm.ref_yaw, stream=stream, grid=grid, state=d_state, tick=ts, end_pt=fsm.end_pt)
        fsm.mpc_result(stream=stream)
        out = fleet.commands(t_cmd, ts.cmd_status, ts.pub_end, ts.cmd_end_pt, odom=fsm.yaw_odom, init_yaw=fsm.init_yaw, t_yaw=t_cmd, out=out, stream=stream)
        veh.step(out, stream)
        veh.odometry(fsm, stream=stream)
        veh.estimator = None

    reset_state()
    side = torch.cuda.Stream()
    graphs = {}
    for with_estimator in (False, True):
        with torch.cuda.stream(side):
            chain(with_estimator, side)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            chain(with_estimator, torch.cuda.current_stream())
        graphs[with_estimator] = g
    times = {False: [], True: []}
    for r in range(REPLAYS + 5):
        for w in (False, True):
            reset_state()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); graphs[w].replay(); e1.record(); torch.cuda.synchronize()
            if r >= 5:
                times[w].append(e0.elapsed_time(e1))
    stat = lambda a: {"median": float(np.median(a)), "mean": float(np.mean(a)), "std_of_a_replay": float(np.std(a)), "min": float(np.min(a))}
    absorbed = int(est.count.min().item()) - est.min_samples
    # the two launches alone (observed step, update), eagerly back to back between two events, against the plain step
    torch.cuda.synchronize()
    alone = {}
    for name, e in (("step", None), ("observed_step_and_update", est)):
        veh.estimator = e
        win = []
        for _ in range(3):
            for _ in range(5):
                veh.step(out)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                veh.step(out)
            e1.record(); torch.cuda.synchronize()
            win.append(e0.elapsed_time(e1) / 200)
        alone[name] = {"ms_per_call_mean_of_3_windows": float(np.mean(win)), "windows": win}
    veh.estimator = None
    return {"workload": f"{B} planners, N = {N}, the period of tools/vehicle_bench.py (tick, command timer S = {S}, six state-machine kernels, vehicle n_sub = {N_SUB}) with the force estimator, alpha = {est.alpha:.6f}, min_samples = {est.min_samples}",
            "device": torch.cuda.get_device_name(0),
            "in_period_graph_ms": {"period_and_vehicle": stat(times[False]), "period_vehicle_and_estimator": stat(times[True]),
                                   "added_ms_median": float(np.median(times[True]) - np.median(times[False])), "replays_each": REPLAYS,
                                   "estimator_kernels_added": 1, "kernels_replaced": "frp_nmpc_vehicle_step by frp_nmpc_vehicle_step_observed",
                                   "residuals_absorbed_per_estimator_in_the_last_replay": absorbed,
                                   "what": "two captured graphs replayed alternately, same start state; the baseline is the graph without the estimator (the parent's period with a vehicle); the added time is a difference of medians and is below the spread when the spread says so; recorded, not asserted"},
            "eager_ms": dict(alone, calls_per_window=200, what="Vehicle.step eagerly, back to back between two events (ctypes marshalling included): the plain step, and the observed step followed by the estimator's update")}


if __name__ == "__main__":
    a = sys.argv[1:]
    res = run(int(a[0]) if len(a) > 0 else 4096, int(a[1]) if len(a) > 1 else 40)
    out = a[2] if len(a) > 2 else os.path.join(ROOT, "profiles", "estimator_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
