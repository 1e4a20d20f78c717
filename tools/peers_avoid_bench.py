#!/usr/bin/env python3
"""Peer avoidance (include/frp_nmpc.h section 19: FleetPeers.boxes / check_paths, AstarPlanner.overlay).  Everything is recorded, nothing
is asserted.
   python tools/peers_avoid_bench.py [B=4096] [replays=40] [out=profiles/peers_avoid_bench.json]
The crossing flight: the 8-planner closed loop of tools/peers_bench.py (e), vehicles 0 and 1 on crossing routes, planning on the
per-planner view -- flown as recorded there (without and with the peer cloud) and with avoidance on (boxes, the path walk with its verdict
and the planner's overlay in front of every period), without and with the peer cloud: closest approach, hit samples, tick results, exit
codes, and per period the boxes, the paths hit and the searches.
The search: the 1024-planner pillar world of tests/tools/astar_bench.py -- the plain entry, the overlay entry with no boxes (Q = 0: the
plain kernel), the overlay kernel with every count 0, with 3 boxes on every planner's own start-goal line, and with those plus 29 boxes
elsewhere in the map; Q = 256 rows a planner.  Each the median of three timed calls of the whole batch after one warm-up, in the same run.
The period: the captured period of tools/peers_bench.py with `B` vehicles, replayed alternately as it is (the baseline, measured in this
run) and with boxes(), check_paths() and the second verdict in front of it; and those launches alone with the vehicles uniformly random
in the 18 x 12 x 5 m hall.
No device: the tool fails."""
import collections
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from forces_resilient_planner_amd import layout as L  # noqa: E402
from forces_resilient_planner_amd import solver, workloads  # noqa: E402

DEV = "cuda:0"
HALF = (0.3, 0.3, 0.3)
stat = lambda a: {"median": float(np.median(a)), "mean": float(np.mean(a)), "std_of_a_replay": float(np.std(a)), "min": float(np.min(a))}


def crossing(with_cloud, avoid, periods=40):
    """tools/peers_bench.py's crossing flight; avoid: boxes, the path walk + verdict and the overlay in front of every period."""
    FB, P = 8, 4096
    lanes = np.array([-8.05, -6.55, -5.05, -3.55, -2.05, 2.05, 3.55, 5.05])
    weights = (15.0, 3.0, 80.0, 15.0, 0.0)
    w = workloads.astar_world(0, "empty", allocate_num=12000)
    dm = solver.OccupancyMap(w)
    pillar = np.array([(x, y, z) for x in np.arange(-0.25, 0.26, 0.1) for y in np.arange(-0.25, 0.26, 0.1) for z in np.arange(-0.95, 2.96, 0.1)], dtype=np.float32)
    dm.insert_cloud(pillar)
    fleet = solver.DeviceFleet(FB, 20, 30, 64, L.MODEL_NORMAL, weights, weights_final=weights)
    fleet.poly_index = torch.zeros((FB, 20), dtype=torch.int32, device=DEV)
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
    if avoid:
        pl.overlay = fp
    clock = m.clock_out[:3]
    centres = torch.zeros((FB, 3), dtype=torch.float64, device=DEV)
    view = dm.local_view(veh.state[:, :3].contiguous(), P)
    results, exits = [collections.Counter() for _ in range(FB)], [collections.Counter() for _ in range(FB)]
    closest, per_period, searches = [], [], collections.Counter()
    for k in range(periods):
        m.clock(0.0, 1)
        m.step(veh.state, clock, None)
        centres.copy_(veh.state[:, :3])
        dm.local_view(centres, P, out=view)
        if with_cloud:
            fp.cloud(fleet, veh.state, view, dm)
        if avoid:
            fp.boxes(fleet, veh.state, dm, HALF)
            fp.check_paths(pl, fsm)
        fsm.period(pl, dm, None, clock, view.cloud, goal=m.goal, goal_fresh=m.fresh, fsm_steps=1, vehicle=veh, cloud_count=view.cloud_count)
        fp.update()
        res, ex, gate = fsm.tick.result.cpu().numpy(), fsm.tick.exit_code.cpu().numpy(), fsm.tick.gate.cpu().numpy()
        tr = veh.trace.cpu().numpy()
        closest.append(float(np.sqrt(((tr[0, :, :3] - tr[1, :, :3]) ** 2).sum(axis=1)).min()))
        srch, ast = fsm.search.cpu().numpy(), pl.status.cpu().numpy()
        for b in np.nonzero(srch[:2])[0]:
            searches[int(ast[b])] += 1
        if avoid:
            per_period.append({"boxes_0_and_1": fp.box_count[:2].cpu().numpy().tolist(), "dropped_own_0_and_1": fp.dropped_own[:2].cpu().numpy().tolist(),
                               "path_hit_0_and_1": fp.path_hit[:2].cpu().numpy().tolist(), "searched_0_and_1": srch[:2].tolist()})
        for b in range(FB):
            results[b][int(res[b])] += 1
            if gate[b] == solver.TICK_RUN:
                exits[b][int(ex[b])] += 1
    a = fp.arrays()
    hist = lambda cs: {str(k): v for k, v in sorted(sum(cs, collections.Counter()).items())}
    out = {"periods": periods, "min_separation_m_of_vehicles_0_and_1": float(np.sqrt(a["sep2_min"][:2].min())), "sep2_min": a["sep2_min"].tolist(),
           "closest_approach_of_0_and_1_per_period_m (min over the 5 samples)": closest, "hit_samples": a["hit_samples"].tolist(),
           "near_samples": a["near_samples"].tolist(), "first_hit": a["first_hit"].tolist(),
           "tick_result_histogram_vehicles_0_and_1 (result: periods)": hist(results[:2]), "tick_result_histogram_vehicles_2_to_7": hist(results[2:]),
           "solver_exit_code_histogram_of_ticks_that_ran_vehicles_0_and_1": hist(exits[:2]), "solver_exit_code_histogram_vehicles_2_to_7": hist(exits[2:]),
           "astar_status_histogram_of_the_searches_of_0_and_1": {str(k): v for k, v in sorted(searches.items())},
           "final_position_0_and_1": veh.x[:2, :3].cpu().numpy().tolist(), "arrived (mission reached)": m.reached.cpu().numpy().tolist()}
    if avoid:
        out["per_period"] = per_period
        out["periods_with_a_path_hit_of_0_or_1"] = int(sum(1 for p in per_period if max(p["path_hit_0_and_1"]) >= 0))
    return out


def search(B=1024, Q=256):
    """The overlay search against the plain one on tests/tools/astar_bench.py's world, in one run."""
    w = workloads.astar_world(5, "pillars", allocate_num=20000, n_obstacles=40)
    q = workloads.astar_queries(B, 5)
    g = w["occ"].shape
    vox = lambda p: [int(np.floor((p[k] - w["origin"][k]) / w["resolution"])) for k in range(3)]
    rng = np.random.default_rng(5)
    rows = np.zeros((B, Q, 6), dtype=np.int32)
    for b in range(B):
        for j in range(32):
            c = vox(q["start_pt"][b] + (0.35, 0.6, 0.8)[j] * (q["end_pt"][b] - q["start_pt"][b])) if j < 3 else [int(rng.integers(0, g[k])) for k in range(3)]
            rows[b, j] = [max(c[k] - 3, 0) for k in range(3)] + [min(c[k] + 3, g[k] - 1) for k in range(3)]
    d_rows = torch.from_numpy(rows).to(DEV)
    out = {}
    for name, overlay in (("plain entry", None), ("overlay entry, Q = 0 (the plain kernel)", (torch.zeros((B, 0, 6), dtype=torch.int32, device=DEV), 0)),
                          ("overlay kernel, every count 0", (d_rows, 0)), ("overlay kernel, 3 boxes on every planner's line", (d_rows, 3)),
                          ("overlay kernel, those 3 and 29 boxes elsewhere in the map", (d_rows, 32))):
        pl = solver.AstarPlanner(w, B, K=1024)
        if overlay is not None:
            pl.overlay = types.SimpleNamespace(box_rows=overlay[0], box_count=torch.full((B,), overlay[1], dtype=torch.int32, device=DEV))
        pl.upload(q["start_pt"], q["start_v"], q["start_a"], q["end_pt"], q["end_v"], q["f_ext"])
        pl.plan(); torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter(); pl.plan(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        stats, st = pl.stats.cpu().numpy(), pl.status.cpu().numpy()
        out[name] = {"batch_ms_median_of_3": float(np.median(ts)) * 1e3, "batch_ms_each": [t * 1e3 for t in ts], "searches_per_s": B / float(np.median(ts)),
                     "expansions_total": int(stats[:, 1].sum()), "expansions_max": int(stats[:, 1].max()),
                     "us_per_expansion_of_the_longest_search": float(np.median(ts)) * 1e6 / max(1, int(stats[:, 1].max())),
                     "status_counts[1..4]": np.bincount(st, minlength=5)[1:].tolist()}
    out["what"] = f"{B} planners, pillar world (seed 5, 40 obstacles, allocate_num 20000), K = 1024, Q = {Q}; boxes of 7 x 7 x 7 voxels; wall clock of the whole " \
                  "batch with a synchronise.  With boxes the searches are other searches (other expansion counts): compare per expansion as well as per batch"
    return out


def period(B=4096, REPLAYS=40):
    """tools/peers_bench.py's period, as it is and with boxes, the path walk and the second verdict in front of it."""
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
    dm = solver.OccupancyMap(origin=(-4.0, -6.0, -1.0), map_size=(18.0, 12.0, 5.0), resolution=0.1, device=DEV)
    dm.insert_cloud(cloud.astype(np.float32))
    peers = solver.FleetPeers(veh, (-4.0, -6.0, -1.0), (18, 12, 5), 1.0, 1.0, 0.6, 0.3, S=S, stages=(2, 5, 9))
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
    held = types.SimpleNamespace(kino_path=d_path[None].expand(B, K, 3).contiguous(), kino_size=i32(K))      # the path every planner holds
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

    def chain(avoid, stream):
        nonlocal out
        fsm.goal(goal, fresh, stream)
        fsm.force(force, ffresh, stream); fsm.safety_verdict(blocked, first_hit, stream)
        if avoid:
            peers.boxes(fleet, d_state, dm, HALF, stream=stream)
            peers.check_paths(held, fsm, stream=stream)
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
    in_period = {"period_without_avoidance (the baseline, measured in this run)": stat(times[False]),
                 "period_with_boxes_walk_and_second_verdict_in_front": stat(times[True]),
                 "added_ms_median": float(np.median(times[True]) - np.median(times[False])), "replays_each": REPLAYS,
                 "boxes_per_planner_mean": float(peers.box_count.clamp(min=0).double().mean().item()), "planners_with_more_than_64_peers": int(peers.box_overflow.sum().item()),
                 "dropped_own_mean": float(peers.dropped_own.double().mean().item()), "planners_whose_path_is_hit": int((peers.path_hit >= 0).sum().item()),
                 "rows_per_planner_Q": int(peers.box_rows.shape[1]),
                 "what": "two captured graphs replayed alternately, same start state; all vehicles start within centimetres of one point (tools/peers_bench.py's "
                         "workload), so every planner has B - 1 candidates, keeps 64, and nearly every box holds its own voxel: the dense end of the selection.  "
                         "The period has no search in it (exec_begin / exec_end on a fixed status): the overlay search's cost is the section above"}

    def alone(Bn):
        pos = np.c_[rng.uniform(-4, 14, Bn), rng.uniform(-6, 6, Bn), rng.uniform(-1, 4, Bn)]
        fp = solver.FleetPeers(Bn, (-4.0, -6.0, -1.0), (18, 12, 5), 1.0, 1.0, 0.6, 0.3, S=1, stages=(2, 5, 9), device=DEV)
        state = torch.zeros((Bn, 9), dtype=torch.float64, device=DEV); state[:, :3] = torch.from_numpy(pos).to(DEV)
        fl = types.SimpleNamespace(N=N, pre_plan=torch.zeros((Bn, N, 17), dtype=torch.float64, device=DEV), have_traj=torch.ones((Bn,), dtype=torch.int32, device=DEV))
        fl.pre_plan[:, :, 8:11] = state[:, None, :3] + 0.1 * torch.arange(N, dtype=torch.float64, device=DEV)[None, :, None]
        kp = (state[:, None, :3] + 0.04 * torch.arange(K, dtype=torch.float64, device=DEV)[None, :, None]).contiguous()
        hold = types.SimpleNamespace(kino_path=kp, kino_size=torch.full((Bn,), K, dtype=torch.int32, device=DEV))
        fp.boxes(fl, state, dm, HALF)
        res = {}
        for name, fn in (("boxes (S = 1 build + one launch, K = 3)", lambda st: fp.boxes(fl, state, dm, HALF, stream=st)),
                         ("check_paths (one launch, 120 samples, stride 5)", lambda st: fp.check_paths(hold, None, stream=st))):
            g = capture(fn)
            res[name] = stat([timed(g) for _ in range(REPLAYS + 5)][5:])
        res["boxes_per_planner_mean"] = float(fp.box_count.clamp(min=0).double().mean().item())
        res["planners_whose_path_is_hit"] = int((fp.path_hit >= 0).sum().item())
        return res

    return {"in_period_graph_ms": in_period, f"launches_alone_replayed_ms, B = {B}, vehicles uniformly random in the 18 x 12 x 5 m hall": alone(B)}


def run(B=4096, REPLAYS=40):
    assert torch.cuda.is_available(), "peers_avoid_bench needs a GPU"
    return {"device": torch.cuda.get_device_name(0),
            "crossing_flight": {"without_the_peer_cloud": crossing(False, False), "with_the_peer_cloud": crossing(True, False),
                                "with_avoidance": crossing(False, True), "with_avoidance_and_the_peer_cloud": crossing(True, True),
                                "what": "8 planners, 40 periods, vehicles 0 and 1 swap lanes 1.5 m apart over 3 m, stages (2, 5, 9), R = 1, d_warn = 0.5, d_hit = 0.25, "
                                        "r_body = 0.2 (the cloud's), boxes of 0.3 m half edge; every flight plans on the per-planner view.  Recorded, nothing asserted"},
            "overlay_search_against_the_plain_search": search(),
            "period": period(B, REPLAYS),
            "not_measured": "other half edges, stages, R and densities; a fleet spread through the hall inside the period graph; a period graph with searches in it; "
                            "counters (no rocprofv3 pass was made); several devices"}


if __name__ == "__main__":
    a = sys.argv[1:]
    res = run(int(a[0]) if len(a) > 0 else 4096, int(a[1]) if len(a) > 1 else 40)
    out = a[2] if len(a) > 2 else os.path.join(ROOT, "profiles", "peers_avoid_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res)[:3000])
