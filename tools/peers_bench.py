#!/usr/bin/env python3
"""The fleet peers (include/frp_nmpc.h section 18, solver.FleetPeers): what update() -- the grid build and the separation record, seven
launches -- adds to the replayed graph of a period, against the same graph without it; the build, the separation and the peer cloud on
their own at B = 4096 and B = 65536 in the 18 x 12 x 5 m hall with R = cell = 1 m; and a brute-force all-pairs separation in torch beside
them.
   python tools/peers_bench.py [B=4096] [replays=40] [out=profiles/peers_bench.json]
Two captured graphs, both the period of tools/vehicle_bench.py with a tracing Vehicle: one as it is (the baseline: the parent's period,
measured in this run), one with FleetPeers.update() behind it.  Replayed alternately (`replays` pairs, state reset before each); the added
time is the difference of the two medians, its spread the standard deviation of the per-replay times.
The same alternation for cloud() in front of the period: there the period's corridor reads a per-planner LocalView (local_view per period,
a map with a 2 x 2 x 1.5 m local radius), once as it is and once with FleetPeers.cloud() between local_view and the tick.
The launches alone: each call captured into a graph of its own and replayed between an event pair, vehicles uniformly random in the hall;
the brute force in torch eager and captured the same way.
The crossing flight: the 8-planner closed loop of tests/test_gpu_peers.py, vehicles 0 and 1 on crossing routes, flown with the per-planner
view as the corridor's cloud, without and with cloud() in front of every period: the separation record and the tick results of both.
The code object: registers, scratch and LDS of every kernel of csrc/frp_peers.hip, from the compiler's resource remarks.
No device: the tool fails."""
import collections
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from forces_resilient_planner_amd import layout as L  # noqa: E402
from forces_resilient_planner_amd import build as BLD  # noqa: E402
from forces_resilient_planner_amd import solver, workloads  # noqa: E402


def code_object():
    """{kernel: registers, scratch, LDS, occupancy} of csrc/frp_peers.hip for gfx950, from -Rpass-analysis=kernel-resource-usage."""
    src = os.path.join(BLD.CSRC, "frp_peers.hip")
    cmd = [BLD.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include")] + BLD.PER_SOURCE_FLAGS["frp_peers.hip"] + \
          ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, cur = {}, None
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "Occupancy [waves/SIMD]": "waves_per_simd",
            "LDS Size [bytes/block]": "lds_bytes_per_workgroup", "VGPR Spill": "vgpr_spill", "SGPR Spill": "sgpr_spill"}
    for line in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip() or m.group(1)
            cur = out.setdefault(name.split("(")[0].replace("frp::peers::", ""), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None and m.group(1).strip() in keys:
            cur[keys[m.group(1).strip()]] = int(m.group(2))
    return out


def crossing(with_cloud, periods=40):
    """The closed loop of tests/test_gpu_peers.py with vehicles 0 and 1 on crossing routes; the corridor reads a per-planner view."""
    dev = "cuda:0"
    FB, P = 8, 4096
    lanes = np.array([-8.05, -6.55, -5.05, -3.55, -2.05, 2.05, 3.55, 5.05])
    weights = (15.0, 3.0, 80.0, 15.0, 0.0)
    w = workloads.astar_world(0, "empty", allocate_num=12000)
    dm = solver.OccupancyMap(w)
    pillar = np.array([(x, y, z) for x in np.arange(-0.25, 0.26, 0.1) for y in np.arange(-0.25, 0.26, 0.1) for z in np.arange(-0.95, 2.96, 0.1)], dtype=np.float32)
    dm.insert_cloud(pillar)
    fleet = solver.DeviceFleet(FB, 20, 30, 64, L.MODEL_NORMAL, weights, weights_final=weights)
    fleet.poly_index = torch.zeros((FB, 20), dtype=torch.int32, device=dev)
    fsm = solver.FleetFSM(fleet)
    pl = solver.AstarPlanner(dm, FB, K=512)
    fsm.bind(pl)
    veh = solver.Vehicle(fleet, trace=True)
    start = np.zeros((FB, 9)); start[:, 0] = -6.05; start[:, 1] = lanes; start[:, 2] = 1.2
    route = np.array([[[-3.05, y, 1.2]] for y in lanes])
    route[0, 0, 1], route[1, 0, 1] = lanes[1], lanes[0]
    veh.reset(fleet.to_device(start))
    veh.odometry(fsm)
    m = solver.Mission(fsm, route=route, arrive_radius=0.3, dwell=0.1, leg_timeout=30.0)
    fp = solver.FleetPeers(veh, (-12.0, -12.0, -1.0), (24, 24, 5), 1.0, 1.0, 0.5, 0.25, S=5, r_body=0.2, stages=(2, 5, 9))
    clock = m.clock_out[:3]
    centres = torch.zeros((FB, 3), dtype=torch.float64, device=dev)
    view = dm.local_view(veh.state[:, :3].contiguous(), P)
    results, exits = [collections.Counter() for _ in range(FB)], [collections.Counter() for _ in range(FB)]
    added, overflowed, closest = 0, 0, []
    for k in range(periods):
        m.clock(0.0, 1)
        m.step(veh.state, clock, None)
        centres.copy_(veh.state[:, :3])
        dm.local_view(centres, P, out=view)
        if with_cloud:
            fp.cloud(fleet, veh.state, view, dm)
            added += int(fp.added.sum().item()); overflowed += int((view.cloud_count < 0).sum().item())
        fsm.period(pl, dm, None, clock, view.cloud, goal=m.goal, goal_fresh=m.fresh, fsm_steps=1, vehicle=veh, cloud_count=view.cloud_count)
        fp.update()
        res, ex, gate = fsm.tick.result.cpu().numpy(), fsm.tick.exit_code.cpu().numpy(), fsm.tick.gate.cpu().numpy()
        tr = veh.trace.cpu().numpy()
        closest.append(float(np.sqrt(((tr[0, :, :3] - tr[1, :, :3]) ** 2).sum(axis=1)).min()))
        for b in range(FB):
            results[b][int(res[b])] += 1
            if gate[b] == solver.TICK_RUN:
                exits[b][int(ex[b])] += 1
    a = fp.arrays()
    hist = lambda cs: {str(k): v for k, v in sorted(sum(cs, collections.Counter()).items())}
    return {"periods": periods, "sep2_min": a["sep2_min"].tolist(), "min_separation_m_of_vehicles_0_and_1": float(np.sqrt(a["sep2_min"][:2].min())),
            "closest_approach_of_0_and_1_per_period_m (min over the 5 samples)": closest,
            "nearest": a["nearest"].tolist(), "near_samples": a["near_samples"].tolist(), "hit_samples": a["hit_samples"].tolist(), "first_hit": a["first_hit"].tolist(),
            "tick_result_histogram_vehicles_0_and_1 (result: periods)": hist(results[:2]), "tick_result_histogram_vehicles_2_to_7": hist(results[2:]),
            "solver_exit_code_histogram_of_ticks_that_ran_vehicles_0_and_1": hist(exits[:2]), "solver_exit_code_histogram_vehicles_2_to_7": hist(exits[2:]),
            "peer_points_added_over_the_flight": added, "planner_periods_whose_cloud_passed_P": overflowed,
            "final_position_0_and_1": veh.x[:2, :3].cpu().numpy().tolist(), "arrived (mission reached)": m.reached.cpu().numpy().tolist()}


def run(B=4096, REPLAYS=40):
    assert torch.cuda.is_available(), "peers_bench needs a GPU"
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
    veh = solver.Vehicle(fleet, n_sub=N_SUB, trace=True, S=S)
    veh.f_true.copy_(fleet.to_device(rng.normal(0, 0.5, (B, 3))))
    dm = solver.OccupancyMap(origin=(-4.0, -6.0, -1.0), map_size=(18.0, 12.0, 5.0), resolution=0.1, device=dev)
    dm.insert_cloud(cloud.astype(np.float32))
    peers = solver.FleetPeers(veh, (-4.0, -6.0, -1.0), (18, 12, 5), 1.0, 1.0, 0.6, 0.3, S=S, r_body=0.2, stages=(2, 5, 9))
    PV = 4096
    dm_v = solver.OccupancyMap(origin=(-4.0, -6.0, -1.0), map_size=(18.0, 12.0, 5.0), resolution=0.1, local_radius=(2.0, 2.0, 1.5), device=dev)
    dm_v.insert_cloud(cloud.astype(np.float32))
    centres = torch.zeros((B, 3), dtype=torch.float64, device=dev)
    view = dm_v.local_view(x_start[:, :3].contiguous(), PV)
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
        veh.reset(x_start); veh.state.copy_(x_start); peers.reset(); peers.tick.zero_()

    def chain(with_peers, stream, per_planner=False, with_cloud=False):
        nonlocal out
        fsm.goal(goal, fresh, stream)
        fsm.force(force, ffresh, stream); fsm.safety_verdict(blocked, first_hit, stream)
        fsm.exec_begin(d_state, t_step, now, *bufs, stream=stream); fsm.exec_end(status, now, stream)
        if per_planner:
            with torch.cuda.stream(stream):
                centres.copy_(d_state[:, :3])
            dm_v.local_view(centres, PV, out=view, stream=stream)
            if with_cloud:
                peers.cloud(fleet, d_state, view, dm_v, stream=stream)
            fleet.full_tick(fsm.external_acc, d_path, toff, view.cloud, fsm.ref_pos, fsm.ref_yaw, stream=stream, cloud_count=view.cloud_count, state=d_state, tick=ts,
                            end_pt=fsm.end_pt)
        else:
            fleet.full_tick(fsm.external_acc, d_path, toff, d_cloud, fsm.ref_pos, fsm.ref_yaw, stream=stream, grid=grid, state=d_state, tick=ts, end_pt=fsm.end_pt)
        fsm.mpc_result(stream=stream)
        out = fleet.commands(t_cmd, ts.cmd_status, ts.pub_end, ts.cmd_end_pt, odom=fsm.yaw_odom, init_yaw=fsm.init_yaw, t_yaw=t_cmd, out=out, stream=stream)
        veh.step(out, stream)
        veh.odometry(fsm, stream=stream)
        if with_peers:
            peers.update(stream=stream)

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
    rec = {n: a for n, a in peers.arrays().items()}
    in_period = {"period_without_peers (the parent's period: the baseline, measured in this run)": stat(times[False]), "period_with_update_behind_it": stat(times[True]),
                 "added_ms_median": float(np.median(times[True]) - np.median(times[False])), "replays_each": REPLAYS,
                 "samples_entered_in_the_last_replay": int(rec["samples"].sum()), "vehicles_with_a_peer_within_R": int((rec["nearest"] >= 0).sum()),
                 "what": "two captured graphs replayed alternately, same start state; the vehicles of this workload start within centimetres of each other, so "
                         "every vehicle has thousands of peers in its 27 cells: the dense end of the separation kernel.  The added time is a difference of medians"}

    # ---- cloud() in front of the period whose corridor reads a per-planner view ----
    reset_state()
    graphs_v = {w: capture(lambda st, w=w: chain(False, st, True, w)) for w in (False, True)}
    times_v, seen = {False: [], True: []}, {}
    for r in range(REPLAYS + 5):
        for w in (False, True):
            reset_state()
            t = timed(graphs_v[w])
            if r >= 5:
                times_v[w].append(t)
            seen[w] = (int((view.cloud_count < 0).sum().item()), float(view.cloud_count.abs().double().mean().item()))
    in_period_cloud = {"period_on_a_per_planner_view_without_cloud (the baseline, measured in this run)": stat(times_v[False]),
                       "the_same_period_with_cloud_in_front_of_the_tick": stat(times_v[True]),
                       "added_ms_median": float(np.median(times_v[True]) - np.median(times_v[False])), "replays_each": REPLAYS,
                       "rows_per_planner_P": PV, "mean_cloud_count_without_and_with": [seen[False][1], seen[True][1]],
                       "planners_whose_cloud_passed_P_without_and_with": [seen[False][0], seen[True][0]],
                       "peer_points_added_mean": float(peers.added.double().mean().item()), "planners_with_more_than_64_peers": int(peers.overflow.sum().item()),
                       "what": "local_view per period on a map with a 2 x 2 x 1.5 m local radius, the corridor on the per-planner cloud (no grid): another corridor "
                               "path than the period above, hence a baseline of its own.  K = 3 stages, r_body = 0.2.  All 4096 vehicles start within centimetres of "
                               "one point, so every planner has 4095 candidates and keeps 64: the added time holds the corridor's work on up to 64 * 4 * 7 more points "
                               "a planner as well as the two launches"}

    # ---- the launches alone, vehicles uniformly random in the hall ----
    def alone(Bn):
        pos = torch.from_numpy(np.c_[rng.uniform(-4, 14, Bn * S), rng.uniform(-6, 6, Bn * S), rng.uniform(-1, 4, Bn * S)].reshape(Bn, S, 3)).to(dev).contiguous()
        fp = solver.FleetPeers(Bn, (-4.0, -6.0, -1.0), (18, 12, 5), 1.0, 1.0, 0.6, 0.3, S=S, r_body=0.2, stages=(2, 5, 9), device=dev)
        state = torch.zeros((Bn, 9), dtype=torch.float64, device=dev); state[:, :3] = pos[:, 0]

        class Stub:
            pass
        fl = Stub(); fl.N = N; fl.pre_plan = torch.zeros((Bn, N, 17), dtype=torch.float64, device=dev); fl.pre_plan[:, :, 8:11] = pos[:, :1]
        fl.have_traj = torch.ones((Bn,), dtype=torch.int32, device=dev)
        P = 512
        box = torch.tensor([0, 0, 0, 180, 120, 50], dtype=torch.int32, device=dev).repeat(Bn, 1).contiguous()
        view = solver.LocalView(box, torch.zeros((Bn, P, 3), dtype=torch.float64, device=dev), torch.zeros((Bn,), dtype=torch.int32, device=dev))
        fp.build(pos)
        res = {}
        for name, fn in (("build (five launches)", lambda st: fp.build(pos, stream=st)), ("separation (two launches)", lambda st: fp.separation(stream=st)),
                         ("cloud (S = 1 build + one launch, K = 3, r_body = 0.2, P = 512)", lambda st: (view.cloud_count.zero_(), fp.cloud(fl, state, view, dm, stream=st)))):
            g = capture(fn)
            ts_ = [timed(g) for _ in range(REPLAYS + 5)][5:]
            res[name] = stat(ts_)
        res["points_added_per_planner_mean (whether stored or beyond P)"] = float(fp.added.double().mean().item())
        res["planners_whose_cloud_overflowed_P"] = int((view.cloud_count < 0).sum().item())
        return res, pos

    launches = {}
    for Bn in (4096, 65536):
        launches[f"B = {Bn}"], pos_n = alone(Bn)
        if Bn == 4096:
            p0 = pos_n[:, 0].contiguous()

            def brute():
                d = p0[:, None, :] - p0[None, :, :]
                d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                d2.fill_diagonal_(float("inf"))
                return d2.min(dim=1)
            for _ in range(3):
                brute()
            bt = []
            for _ in range(REPLAYS):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); brute(); e1.record(); torch.cuda.synchronize()
                bt.append(e0.elapsed_time(e1))
            launches["brute force in torch, B = 4096, ONE sample (eager: difference, squares, min over a 4096 x 4096 matrix)"] = stat(bt)
            g_b = capture(lambda st: brute())
            launches["the same brute force captured into a graph and replayed, as the grid's calls are"] = stat([timed(g_b) for _ in range(REPLAYS + 5)][5:])
    return {"workload": f"{B} vehicles in the period of tools/vehicle_bench.py; the launches alone in an 18 x 12 x 5 m hall, R = cell = 1 m, S = {S}",
            "device": torch.cuda.get_device_name(0), "in_period_graph_ms": in_period, "cloud_in_front_of_the_period_graph_ms": in_period_cloud,
            "launches_alone_replayed_ms": launches,
            "crossing_flight": {"without_the_peer_cloud": crossing(False), "with_the_peer_cloud": crossing(True),
                                "what": "8 planners, 40 periods, vehicles 0 and 1 swap lanes 1.5 m apart over 3 m, r_body = 0.2, stages (2, 5, 9), R = 1, d_warn = 0.5, "
                                        "d_hit = 0.25; both flights plan on the per-planner view.  Recorded, nothing asserted"},
            "code_object_gfx950": code_object(),
            "not_measured": "other R, cell, S, K, r_body and densities; a fleet spread through the hall inside the period graph; the eager calls' host side; "
                            "counters (no rocprofv3 pass was made); several devices"}


if __name__ == "__main__":
    a = sys.argv[1:]
    res = run(int(a[0]) if len(a) > 0 else 4096, int(a[1]) if len(a) > 1 else 40)
    out = a[2] if len(a) > 2 else os.path.join(ROOT, "profiles", "peers_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
