#!/usr/bin/env python3
"""The fleet state machine (include/frp_nmpc_fsm.h, solver.FleetFSM) for a fleet: what its six kernels add to the replayed tick graph, and
what an exec step costs with and without searches.
   python tools/fsm_bench.py [B=4096] [replays=40] [steps=200] [out=profiles/fsm_bench.json]
  in graph   two captured graphs, full_tick(tick=...) -> commands (S = 5) as it was, and the same with the six state-machine kernels
             around it (goal, force, safety transitions, exec_begin, exec_end before the tick; the mpc switch after it; no A* launch and
             no collision check: those are measured on their own, below and in profiles/occmap_bench.json), replayed alternately
             (`replays` pairs, plans and state reset before each).  The baseline is the graph WITHOUT the entries; the added time is the
             difference of the two medians, its spread the standard deviation of the per-replay times
  exec step  FleetFSM.exec_step (exec_begin -> frp_nmpc_astar_batch with active = search -> exec_end) eagerly between two HIP events,
             `steps` back-to-back calls with NOBODY searching (everybody executes: the A* launch with an empty mask -- what one more
             fsm_steps costs a period in the common case), and the same call with a quarter of the fleet in GEN_NEW_TRAJ (each searches
             4 m across an empty 20 x 20 x 4 m world with one pillar; the state is put back before every call, by one copy that the
             empty-mask figure carries as well)
No device: the tool fails."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from forces_resilient_planner_amd import layout as L  # noqa: E402
from forces_resilient_planner_amd import solver, workloads  # noqa: E402


def run(B=4096, REPLAYS=40, STEPS=200):
    assert torch.cuda.is_available(), "fsm_bench needs a GPU"
    dev = "cuda:0"
    N, M, F, K, S = 20, 30, 64, 120, 5
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
    d_state = fleet.to_device(plan[:, 1, 8:17].copy())
    grid = solver.CloudGrid(d_cloud, 0.5)
    toff = fleet.to_device(rng.uniform(0, 0.01, B))
    fsm = solver.FleetFSM(fleet)
    ts = fsm.tick
    ts.path_size(K)
    i32 = lambda v: torch.full((B,), v, dtype=torch.int32, device=dev)
    goal, fresh = fleet.to_device(np.tile(path[-1], (B, 1))), i32(0)
    fresh[::16] = 1                                                    # a message for every 16th planner
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

    def chain(with_fsm, stream):
        nonlocal out
        if with_fsm:
            fsm.goal(goal, fresh, stream); fsm.force(force, ffresh, stream); fsm.safety_verdict(blocked, first_hit, stream)
            fsm.exec_begin(d_state, t_step, now, *bufs, stream=stream); fsm.exec_end(status, now, stream)
        fleet.full_tick(fsm.external_acc, d_path, toff, d_cloud, fsm.ref_pos, fsm.ref_yaw, stream=stream, grid=grid, state=d_state, tick=ts, end_pt=fsm.end_pt)
        if with_fsm:
            fsm.mpc_result(stream=stream)
        out = fleet.commands(t_cmd, ts.cmd_status, ts.pub_end, ts.cmd_end_pt, odom=fsm.yaw_odom, init_yaw=fsm.init_yaw, t_yaw=t_cmd, out=out, stream=stream)

    reset_state()
    side = torch.cuda.Stream()
    graphs = {}
    for with_fsm in (False, True):
        with torch.cuda.stream(side):
            chain(with_fsm, side)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            chain(with_fsm, torch.cuda.current_stream())
        graphs[with_fsm] = g
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
    states = {int(k): int((fsm.state == k).sum().item()) for k in torch.unique(fsm.state).tolist()}
    in_graph = {"tick_and_commands": stat(times[False]), "tick_commands_and_fsm": stat(times[True]),
                "added_ms_median": float(np.median(times[True]) - np.median(times[False])), "replays_each": REPLAYS, "fsm_kernels_added": 6,
                "states_after_the_last_replay (state: planners)": states,
                "what": "two captured graphs replayed alternately, same start state; the baseline is the graph without the entries; the added time is a difference of medians and is below the spread when the spread says so"}
    # ---- the exec step ----
    w = workloads.astar_world(0, "empty", allocate_num=4000)
    dm = solver.OccupancyMap(w)
    dm.insert_cloud(np.array([(x, y, z) for x in np.arange(-0.25, 0.26, 0.1) for y in np.arange(-0.25, 0.26, 0.1) for z in np.arange(-0.95, 2.96, 0.1)], dtype=np.float32))
    pl = solver.AstarPlanner(dm, B, K=256)
    fsm.bind(pl)
    odom = np.zeros((B, 9)); odom[:, 0] = rng.uniform(-8, 4, B); odom[:, 1] = rng.uniform(-8, 8, B); odom[:, 2] = 1.2
    d_odom = fleet.to_device(odom)
    end = odom[:, 0:3].copy(); end[:, 0] += 4.0
    reset_state()
    fsm.end_pt.copy_(fleet.to_device(end))
    exec_step = {}
    for name, every, reps in (("nobody_searching", 0, STEPS), ("a_quarter_searching", 4, max(5, STEPS // 20))):
        st0 = i32(solver.FSM_EXEC_TRAJ)
        if every:
            st0[::every] = solver.FSM_GEN_NEW_TRAJ
        windows, searched, found = [], 0, 0
        for _ in range(3):
            for _ in range(3):
                fsm.state.copy_(st0); fsm.exec_step(pl, d_odom, t_step, now)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fsm.state.copy_(st0); fsm.exec_step(pl, d_odom, t_step, now)
            e1.record(); torch.cuda.synchronize()
            windows.append(e0.elapsed_time(e1) / reps)
            searched = int(fsm.search.sum().item()); found = int(((fsm.search != 0) & (pl.status != solver.ASTAR_NO_PATH)).sum().item())
        exec_step[name] = {"ms_per_step_mean_of_3_windows": float(np.mean(windows)), "windows": windows, "steps_per_window": reps,
                           "planners_searching": searched, "searches_that_found_a_path": found}
    exec_step["what"] = ("FleetFSM.exec_step eagerly, back to back between two events (ctypes marshalling and one state copy included): three launches, "
                         "the middle one frp_nmpc_astar_batch over the whole fleet with active = search")
    exec_step["astar"] = {"world": "empty 20 x 20 x 4 m, 0.1 m voxels, one pillar", "allocate_num": 4000, "K": 256, "goal": "4 m along x"}
    return {"workload": f"{B} planners, N = {N}, the tick of tools/outcome_bench.py with the command timer (S = {S})", "device": torch.cuda.get_device_name(0),
            "in_tick_graph_ms": in_graph, "exec_step_ms": exec_step}


if __name__ == "__main__":
    a = sys.argv[1:]
    res = run(int(a[0]) if len(a) > 0 else 4096, int(a[1]) if len(a) > 1 else 40, int(a[2]) if len(a) > 2 else 200)
    out = a[3] if len(a) > 3 else os.path.join(ROOT, "profiles", "fsm_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
