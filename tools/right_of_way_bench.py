#!/usr/bin/env python3
"""Right of way (include/frp_nmpc.h section 20: FleetPeers.boxes(priority=...), solver.RightOfWay).  Everything is recorded, nothing is
asserted.
   python tools/right_of_way_bench.py [B=4096] [replays=40] [out=profiles/right_of_way_bench.json]
The crossing flight of tools/peers_avoid_bench.py (8 planners, 40 periods, vehicles 0 and 1 swapping lanes, planning on the per-planner
view), in one run: as on record (symmetric avoidance) and with right of way -- closest approach, hit samples, the searches' statuses,
tick results, holds, releases, timeouts, periods held and whether both vehicles arrive.
The launches alone: `B` vehicles uniformly random in the 18 x 12 x 5 m hall of tools/peers_bench.py, each captured and replayed between
an event pair: boxes() (the existing entry), boxes(priority=...) (the ranked entry) and RightOfWay.step(), in the same run.
The period: the crossing period captured twice, without and with the unit, the replays of the two graphs alternated in one process.
Each part runs in a child process of its own under a time limit of its own; a part that fails ends the run.  No device: the tool fails."""
import collections
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DEV = "cuda:0"
HALF = (0.3, 0.3, 0.3)
ROW = dict(r_release=0.8, n_clear=3, a_brake=2.0, hold_timeout=12)
LIMITS = dict(crossing=240, launches=120, period=180)      # seconds, per part
stat = lambda a: {"median": float(np.median(a)), "mean": float(np.mean(a)), "std_of_a_replay": float(np.std(a)), "min": float(np.min(a))}


def setup(right_of_way):
    """The crossing fleet, and period(stream): one period of it -- clock, mission, view, boxes [ranked, RightOfWay.step], check_paths, the
    state machine's period, the separation record -- eager on the current stream or, inside a capture, on `stream`."""
    import torch
    from forces_resilient_planner_amd import layout as L, solver, workloads
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
    pl.overlay = fp
    row = solver.RightOfWay(fp, fsm, pl, **ROW) if right_of_way else None
    clock = m.clock_out[:3]
    centres = torch.zeros((FB, 3), dtype=torch.float64, device=DEV)
    view = dm.local_view(veh.state[:, :3].contiguous(), P)

    def period(stream=None):
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            m.clock(0.0, 1, stream=stream)
            m.step(veh.state, clock, None, stream=stream)
            centres.copy_(veh.state[:, :3])
            dm.local_view(centres, P, out=view, stream=stream)
            goal, fresh = m.goal, m.fresh
            if row is None:
                fp.boxes(fleet, veh.state, dm, HALF, stream=stream)
            else:
                fp.boxes(fleet, veh.state, dm, HALF, stream=stream, priority=row.priority)
                goal, fresh = row.step(veh.state, m.goal, m.fresh, stream=stream)
            fp.check_paths(pl, fsm, stream=stream)
            fsm.period(pl, dm, None, clock, view.cloud, goal=goal, goal_fresh=fresh, fsm_steps=1, vehicle=veh, cloud_count=view.cloud_count, stream=stream)
            fp.update(stream=stream)

    return dict(FB=FB, route=route, fsm=fsm, pl=pl, veh=veh, m=m, fp=fp, row=row, period=period)


def crossing(right_of_way, periods=40):
    c = setup(right_of_way)
    FB, route, fsm, pl, veh, m, fp, row = (c[n] for n in ("FB", "route", "fsm", "pl", "veh", "m", "fp", "row"))
    results = [collections.Counter() for _ in range(FB)]
    closest, per_period, searches = [], [], collections.Counter()
    for k in range(periods):
        c["period"]()
        res = fsm.tick.result.cpu().numpy()
        tr = veh.trace.cpu().numpy()
        closest.append(float(np.sqrt(((tr[0, :, :3] - tr[1, :, :3]) ** 2).sum(axis=1)).min()))
        srch, ast = fsm.search.cpu().numpy(), pl.status.cpu().numpy()
        for b in np.nonzero(srch[:2])[0]:
            searches[int(ast[b])] += 1
        per_period.append({"boxes_0_and_1": fp.box_count[:2].cpu().numpy().tolist(), "path_hit_0_and_1": fp.path_hit[:2].cpu().numpy().tolist(),
                           "searched_0_and_1": srch[:2].tolist(), "fsm_state_0_and_1": fsm.state[:2].cpu().numpy().tolist(),
                           "holding_0_and_1": row.holding[:2].cpu().numpy().tolist() if row is not None else None})
        for b in range(FB):
            results[b][int(res[b])] += 1
    a = fp.arrays()
    hist = lambda cs: {str(k): v for k, v in sorted(sum(cs, collections.Counter()).items())}
    out = {"periods": periods, "right_of_way": bool(right_of_way), "parameters": ROW if right_of_way else None,
           "min_separation_m_of_vehicles_0_and_1": float(np.sqrt(a["sep2_min"][:2].min())), "sep2_min": a["sep2_min"].tolist(),
           "closest_approach_of_0_and_1_per_period_m (min over the 5 samples)": closest, "hit_samples": a["hit_samples"].tolist(), "near_samples": a["near_samples"].tolist(),
           "tick_result_histogram_vehicles_0_and_1 (result: periods)": hist(results[:2]), "tick_result_histogram_vehicles_2_to_7": hist(results[2:]),
           "astar_status_histogram_of_the_searches_of_0_and_1": {str(k): v for k, v in sorted(searches.items())},
           "final_position_0_and_1": veh.x[:2, :3].cpu().numpy().tolist(), "goal_0_and_1": route[:2, 0].tolist(), "arrived (mission reached)": m.reached.cpu().numpy().tolist(),
           "per_period": per_period}
    if row is not None:
        out.update({n: getattr(row, n).cpu().numpy().tolist() for n in ("holds", "releases", "timeouts", "hold_periods", "longest_hold", "bad")})
    return out


def period_graph(replays, eager=2):
    """The crossing period captured twice -- boxes -> check_paths -> period, and boxes(priority=) -> RightOfWay.step -> check_paths -> period
    -- on two fleets of their own in one process, after `eager` periods each, the replays of the two alternated: ms per replay between an
    event pair.  The flights go on under the replays (a replay is the next period), so a replay's work is that period's: per_replay_ms keeps
    every one, in order, beside the median and the std."""
    import torch
    sides = {"as_on_record (boxes -> check_paths -> period)": setup(False), "with_right_of_way (boxes(priority=) -> step -> check_paths -> period)": setup(True)}
    graphs = {}
    for name, c in sides.items():
        for _ in range(eager):
            c["period"]()
        torch.cuda.synchronize()
        side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c["period"](torch.cuda.current_stream())
        torch.cuda.synchronize()
        graphs[name] = g
    ms = {name: [] for name in sides}
    for _ in range(replays):
        for name, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); g.replay(); b.record(); torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b))
    out = {"planners": 8, "replays_each": replays, "eager_periods_before_the_capture": eager, "unit": "ms per replay of the captured period, the two graphs replayed alternately"}
    for name, c in sides.items():
        out[name] = dict(stat(ms[name]), per_replay_ms=ms[name], hit_samples=c["fp"].hit_samples.cpu().numpy().tolist(),
                         holds=c["row"].holds.cpu().numpy().tolist() if c["row"] is not None else None)
    a, b = (np.array(v) for v in ms.values())
    out["difference_of_the_medians_ms (with - without)"] = float(np.median(b) - np.median(a))
    out["median_of_the_paired_differences_ms"] = float(np.median(b - a))
    return out


def launches(B, replays):
    import torch
    from forces_resilient_planner_amd import solver
    rng = np.random.default_rng(1)
    state = np.zeros((B, 9)); state[:, :3] = rng.random((B, 3)) * (18.0, 12.0, 5.0) + (-9.0, -6.0, 0.0); state[:, 3:6] = rng.random((B, 3)) - 0.5
    N = 20
    plan = np.zeros((B, N, 17))
    for k in range(N):
        plan[:, k, 8:11] = state[:, :3] + 0.05 * (k + 1) * state[:, 3:6]
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    fleet = type("Fleet", (), dict(N=N, pre_plan=dev(plan, np.float64), have_traj=dev(np.ones(B), np.int32)))()
    hall = type("Map", (), dict(origin=(-9.0, -6.0, 0.0), resolution=0.1, grid=(180, 120, 50)))()
    fp = solver.FleetPeers(B, (-9.0, -6.0, 0.0), (18, 12, 5), 1.0, 1.0, 0.5, 0.25, S=1, stages=(2, 5, 9), device=DEV)
    st = dev(state, np.float64)
    i32 = lambda v=0: torch.full((B,), v, dtype=torch.int32, device=DEV)
    tick = type("Tick", (), dict(cmd_end_pt=torch.zeros((B, 3), dtype=torch.float64, device=DEV)))()
    names = [n for n, _ in solver.Fsm._fields_[1:]]
    fsm = type("Fsm", (), dict(torch=torch, B=B, fleet=fleet, tick=tick, state=i32(4), end_pt=torch.zeros((B, 3), dtype=torch.float64, device=DEV)))()
    filler = torch.zeros((B, 9), dtype=torch.float64, device=DEV)
    for n in names:
        if not hasattr(fsm, n):
            setattr(fsm, n, i32() if n in ("have_target", "have_traj", "exec_mpc", "plan_fail_count", "cmd_status", "pub_end") else filler)
    fsm.struct = lambda: solver.Fsm(B, *[getattr(fsm, n).data_ptr() for n in names])
    planner = type("Planner", (), dict(B=B, status=i32(3)))()
    row = solver.RightOfWay(fp, fsm, planner, **ROW)

    def timed(fn):
        fn(); torch.cuda.synchronize()
        side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fn(torch.cuda.current_stream())
        torch.cuda.synchronize()
        ms = []
        for _ in range(replays + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); g.replay(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return stat(ms[3:])

    out = {"B": B, "replays": replays, "unit": "ms per replay of a captured graph holding the launch (boxes: with its S = 1 grid build)",
           "boxes()": timed(lambda s=None: fp.boxes(fleet, st, hall, HALF, stream=s)),
           "boxes(priority=...)": timed(lambda s=None: fp.boxes(fleet, st, hall, HALF, stream=s, priority=row.priority)),
           "RightOfWay.step()": timed(lambda s=None: row.step(st, stream=s))}
    out["boxes_per_planner_mean"] = float(fp.box_count.clamp(min=0).double().mean().item())
    out["planners_with_outranking_boxes"] = int((fp.outrank_boxes > 0).sum().item())
    out["holding_after_the_replays"] = int(row.holding.sum().item())
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--part":
        part, B, replays = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
        res = {"as_on_record (symmetric avoidance)": crossing(False), "with_right_of_way": crossing(True)} if part == "crossing" else \
            launches(B, replays) if part == "launches" else period_graph(replays)
        print("RESULT " + json.dumps(res))
        return 0
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    replays = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "right_of_way_bench.json")
    res = {"tool": "tools/right_of_way_bench.py", "compare_with": "profiles/peers_avoid_bench.json: 4.47 mm, 35 hit samples each, 18 of 20 searches NO_PATH",
           "not_measured": ["the period graph of a large fleet (4096 vehicles) with and without the unit", "other r_release / n_clear / a_brake / hold_timeout, priorities other than all zero",
                            "other half edges, stages, R and densities", "a fleet in which many planners hold at once", "counters"]}
    for part in ("crossing", "launches", "period"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part, str(B), str(replays)], capture_output=True, text=True, timeout=LIMITS[part])
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            return 1
        res[part] = json.loads(line[-1][7:])
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    brief = {k: {n: v for n, v in d.items() if n not in ("per_period", "closest_approach_of_0_and_1_per_period_m (min over the 5 samples)")} for k, d in res["crossing"].items()}
    per = {k: ({n: v for n, v in d.items() if n != "per_replay_ms"} if isinstance(d, dict) else d) for k, d in res["period"].items()}
    print(json.dumps({"crossing": brief, "launches": res["launches"], "period": per}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
