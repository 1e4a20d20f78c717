#!/usr/bin/env python3
"""The mission (include/frp_nmpc.h section 17, solver.Mission) for a fleet: what its two launches -- the clock and the step -- add to the
replayed graph of a period, against the same graph without them, and the step on its own.
   python tools/mission_bench.py [B=4096] [replays=40] [out=profiles/mission_bench.json]
Two captured graphs, both the period of tools/vehicle_bench.py (the chain of tools/fsm_bench.py followed by Vehicle.step -> message ->
odometry): one whose goal callback reads host-written goal / fresh arrays (the baseline: the parent's period), one with Mission.clock and
Mission.step in front (random mode, R = 4, a 0.1 m occupancy map given) whose goal callback reads the mission's arrays.  Replayed
alternately (`replays` pairs, plans, state and mission reset before each, so every vehicle is IDLE and draws); the added time is the
difference of the two medians, its spread the standard deviation of the per-replay times.
The step alone, one captured launch replayed `replays` times between event pairs: with every vehicle FLYING and on time (four loads and one
store per wave: the launch floor), and with every vehicle IDLE and drawing (the mission reset before each replay, outside the events).
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
    assert torch.cuda.is_available(), "mission_bench needs a GPU"
    dev = "cuda:0"
    N, M, F, K, S, N_SUB, R = 20, 30, 64, 120, 5, 4, 4
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
    dm = solver.OccupancyMap(origin=(-4.0, -6.0, -1.0), map_size=(18.0, 12.0, 5.0), resolution=0.1, device=dev)
    dm.insert_cloud(cloud.astype(np.float32))
    mission = solver.Mission(fsm, goal_box=(-2.0, 11.0, -3.5, 3.5), min_dist=0.5, max_dist=8.0, R=R, seed=1)
    d_state = veh.state
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
        veh.reset(x_start); veh.state.copy_(x_start); mission.reset(); mission.k.zero_()

    def chain(with_mission, stream):
        nonlocal out
        if with_mission:
            clock = mission.clock(1.0, 1, stream=stream)
            mission.step(d_state, clock, dm, stream=stream)
            fsm.goal(mission.goal, mission.fresh, stream)
        else:
            fsm.goal(goal, fresh, stream)
        fsm.force(force, ffresh, stream); fsm.safety_verdict(blocked, first_hit, stream)
        fsm.exec_begin(d_state, t_step, now, *bufs, stream=stream); fsm.exec_end(status, now, stream)
        fleet.full_tick(fsm.external_acc, d_path, toff, d_cloud, fsm.ref_pos, fsm.ref_yaw, stream=stream, grid=grid, state=d_state, tick=ts, end_pt=fsm.end_pt)
        fsm.mpc_result(stream=stream)
        out = fleet.commands(t_cmd, ts.cmd_status, ts.pub_end, ts.cmd_end_pt, odom=fsm.yaw_odom, init_yaw=fsm.init_yaw, t_yaw=t_cmd, out=out, stream=stream)
        veh.step(out, stream)
        veh.odometry(fsm, stream=stream)

    def capture(fn):
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            fn(side)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fn(torch.cuda.current_stream())
        torch.cuda.synchronize()
        return g

    def timed(g):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    reset_state()
    graphs = {w: capture(lambda st, w=w: chain(w, st)) for w in (False, True)}
    times = {False: [], True: []}
    for r in range(REPLAYS + 5):
        for w in (False, True):
            reset_state()
            t = timed(graphs[w])
            if r >= 5:
                times[w].append(t)
    stat = lambda a: {"median": float(np.median(a)), "mean": float(np.mean(a)), "std_of_a_replay": float(np.std(a)), "min": float(np.min(a))}
    issued, blocked_n = int(mission.issued.sum().item()), int(mission.blocked.sum().item())
    # the step alone
    clock = mission.clock_out[:3]
    g_step = capture(lambda st: mission.step(d_state, clock, dm, stream=st))
    alone = {"all_flying": [], "all_drawing": []}
    for r in range(REPLAYS + 5):
        mission.reset(); mission.phase.fill_(solver.MISSION_FLYING); fsm.have_target.fill_(1); fsm.have_odom.fill_(1)
        t = timed(g_step)
        flying_untouched = int(mission.issued.sum().item()) == 0
        mission.reset()
        u = timed(g_step)
        if r >= 5:
            alone["all_flying"].append(t); alone["all_drawing"].append(u)
    drew = int(mission.issued.sum().item()) + int(mission.blocked.sum().item())
    return {"workload": f"{B} vehicles, random mode, R = {R}, a {dm.grid[0]} x {dm.grid[1]} x {dm.grid[2]} map of 0.1 m given, in the period of tools/vehicle_bench.py",
            "device": torch.cuda.get_device_name(0),
            "in_period_graph_ms": {"period_without_mission (the parent's period: the baseline)": stat(times[False]), "period_with_clock_and_step": stat(times[True]),
                                   "added_ms_median": float(np.median(times[True]) - np.median(times[False])), "replays_each": REPLAYS,
                                   "issued_and_blocked_in_the_last_replay": [issued, blocked_n],
                                   "what": "two captured graphs replayed alternately, same start state, every vehicle IDLE and drawing; the added time is a "
                                           "difference of medians and means nothing where it is below the spread of a replay"},
            "step_alone_replayed_ms": {"every_vehicle_flying_and_on_time": stat(alone["all_flying"]), "every_vehicle_drawing": stat(alone["all_drawing"]),
                                       "vehicles_that_drew_in_the_last_replay": drew, "flying_fleet_left_untouched": flying_untouched,
                                       "what": "one captured launch between an event pair, host idle before it: the figure holds the graph launch itself"},
            "not_measured": "route mode; other R, map sizes and body sizes; the eager calls (ctypes and the struct's construction on the host); "
                            "counters (no rocprofv3 pass was made); a fleet spread over several devices"}


if __name__ == "__main__":
    a = sys.argv[1:]
    res = run(int(a[0]) if len(a) > 0 else 4096, int(a[1]) if len(a) > 1 else 40)
    out = a[2] if len(a) > 2 else os.path.join(ROOT, "profiles", "mission_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
