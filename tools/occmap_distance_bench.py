#!/usr/bin/env python3
"""The occupancy map's distance field and clearance queries (include/frp_nmpc_occmap_distance.h, solver.DistanceField / FlightClearance)
-> profiles/occmap_distance_bench.json.   python tools/occmap_distance_bench.py [reps=9] [B=4096] [replays=40] [out=...]
  * DistanceField.update() on the two maps of tools/occmap_bench.py (the pillar world, 20 x 20 x 4 m, and a map of the reference's
    size, 40 x 40 x 5 m at 0.1 m with 25 pillars) at R = 10, 20 and 40, next to OccupancyMap.refresh() on the same map, which streams
    the same volume: windows of back-to-back calls between two events, the variants ALTERNATING, `reps` windows each, median and spread;
    the same as graph replays of a captured window (no launch cost of the host in it); and the bytes per voxel the three passes move,
    computed from the shapes and the tiling (the halo rows a workgroup re-reads included).
  * FlightClearance.update() for B vehicles with S = 5: eager, and as an addition to the replayed period graph of
    tools/estimator_bench.py's baseline (the period with a vehicle that traces), both graphs replayed alternately in this run.
Recorded, not asserted anywhere.  No device: the tool fails."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from forces_resilient_planner_amd import layout as L  # noqa: E402
from forces_resilient_planner_amd import solver, workloads  # noqa: E402

DEV = "cuda:0"
RADII = (10, 20, 40)
WINDOW = 50


def stat(a):
    return {"median": float(np.median(a)), "min": float(np.min(a)), "max": float(np.max(a)), "std": float(np.std(a)), "n": len(a)}


def pillar_cloud(rng, n_pillars, lo, hi, top):
    """(tools/occmap_bench.py's) points on a 0.05 m lattice inside random vertical boxes: every voxel of a box is hit."""
    out = []
    for _ in range(n_pillars):
        cx, cy = rng.uniform(lo[0], hi[0]), rng.uniform(lo[1], hi[1])
        hx, hy = rng.uniform(0.15, 0.6, 2)
        out.append(np.mgrid[cx - hx:cx + hx:0.05, cy - hy:cy + hy:0.05, 0.0:top:0.05].reshape(3, -1).T)
    return np.concatenate(out).astype(np.float32)


def pass_tiling(A, I, R):
    """csrc/frp_occmap_distance.hip plan_pass: (TY, TZ) of a pass along an axis of length A with inner extent I."""
    TZ = I if I <= 128 else 64
    rows = (32768 if R <= 32 else 61440) // (2 * TZ)
    nty = -(-A // (rows - 2 * R))
    return -(-A // nty), TZ


def bytes_per_voxel(grid, R):
    """What the three passes read and write per voxel, from the shapes: the bit plane and a byte; a byte (+ halo) and two; two (+ halo)
    and two."""
    gx, gy, gz = grid
    ty_y, _ = pass_tiling(gy, gz, R)
    ty_x, _ = pass_tiling(gx, gy * gz, R)
    halo_y, halo_x = min(2 * R, gy) / ty_y, min(2 * R, gx) / ty_x    # (rows outside the axis are not read)
    z = -(-gz // 32) * 4 / gz + 1
    y = 1 * (1 + halo_y) + 2
    x = 2 * (1 + halo_x) + 2
    return {"z_pass": z, "y_pass": y, "x_pass": x, "total": z + y + x, "halo_rows_over_tile_rows": {"y": halo_y, "x": halo_x},
            "refresh_for_comparison": 8 + 1 + -(-gz // 32) * 4 / gz + 1}


def window(fn, n=WINDOW):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def captured(fn, n=WINDOW):
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fn(side)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(n):
            fn(torch.cuda.current_stream())
    torch.cuda.synchronize()
    return g


def update_bench(name, dm, reps):
    fields = {R: dm.distance_field(R=R, border=True) for R in RADII}
    eager = {"refresh": dm.refresh}
    eager.update({f"update_R{R}": f.update for R, f in fields.items()})
    graphs = {"refresh": captured(lambda s: dm.refresh(s))}
    graphs.update({f"update_R{R}": captured(lambda s, f=f: f.update(s)) for R, f in fields.items()})
    for fn in eager.values():                                     # warm every variant
        window(fn, 5)
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    t_eager, t_graph = {k: [] for k in eager}, {k: [] for k in graphs}
    for _ in range(reps):                                         # alternating: one window of each variant per repetition
        for k, fn in eager.items():
            t_eager[k].append(window(fn))
        for k, g in graphs.items():
            t_graph[k].append(window(g.replay, 1) / WINDOW)
    far = {R: float((f.field.view(torch.int16) == -1).float().mean().item()) for R, f in fields.items()}
    n = int(np.prod(dm.grid))
    out = {"grid": list(dm.grid), "voxels": n, "occupied_voxels": int(dm.occ.sum().item()), "border": True,
           "ms_per_call_eager": {k: stat(v) for k, v in t_eager.items()}, "ms_per_call_in_a_replayed_graph": {k: stat(v) for k, v in t_graph.items()},
           "calls_per_window": WINDOW, "windows_each": reps, "share_of_voxels_FAR": far,
           "bytes_per_voxel": {f"R{R}": bytes_per_voxel(dm.grid, R) for R in RADII}}
    ref = out["ms_per_call_in_a_replayed_graph"]["refresh"]["median"]
    out["update_over_refresh_in_a_graph"] = {f"R{R}": out["ms_per_call_in_a_replayed_graph"][f"update_R{R}"]["median"] / ref for R in RADII}
    out["GB_per_s_implied_in_a_graph"] = {f"R{R}": n * out["bytes_per_voxel"][f"R{R}"]["total"] / (out["ms_per_call_in_a_replayed_graph"][f"update_R{R}"]["median"] * 1e6) for R in RADII}
    print(name, json.dumps(out), flush=True)
    return out


def flight_bench(dm, B, REPLAYS):
    """tools/estimator_bench.py's baseline period (tick, command timer, six state-machine kernels, a vehicle that traces) with and without
    FlightClearance.update() at its end."""
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
    df = dm.distance_field()                                             # R = 20, border
    fc = solver.FlightClearance(veh, df)
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
        fc.reset()

    def chain(with_clearance, stream):
        nonlocal out
        fsm.goal(goal, fresh, stream); fsm.force(force, ffresh, stream); fsm.safety_verdict(blocked, first_hit, stream)
        fsm.exec_begin(d_state, t_step, now, *bufs, stream=stream); fsm.exec_end(status, now, stream)
        fleet.full_tick(fsm.external_acc, d_path, toff, d_cloud, fsm.ref_pos, fsm.ref_yaw, stream=stream, grid=grid, state=d_state, tick=ts, end_pt=fsm.end_pt)
        fsm.mpc_result(stream=stream)
        out = fleet.commands(t_cmd, ts.cmd_status, ts.pub_end, ts.cmd_end_pt, odom=fsm.yaw_odom, init_yaw=fsm.init_yaw, t_yaw=t_cmd, out=out, stream=stream)
        veh.step(out, stream)
        veh.odometry(fsm, stream=stream)
        if with_clearance:
            fc.update(stream=stream)

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
    seen = dict(samples_per_vehicle=int(fc.samples.min().item()), hits=int(fc.hits.sum().item()),
                vehicles_with_a_finite_clearance=int(torch.isfinite(fc.min_clear).sum().item()), min_clear_min=float(fc.min_clear.min().item()))
    for _ in range(3):
        window(fc.update, 5)
    eager = [window(fc.update, 200) for _ in range(5)]
    return {"workload": f"{B} planners, N = {N}, the period of tools/estimator_bench.py's baseline (tick, command timer S = {S}, six state-machine kernels, vehicle n_sub = {N_SUB}, trace on) on a "
                        f"{'x'.join(map(str, dm.grid))} map, field R = {df.R} with the border",
            "in_period_graph_ms": {"period_and_vehicle": stat(times[False]), "period_vehicle_and_clearance": stat(times[True]),
                                   "added_ms_median": float(np.median(times[True]) - np.median(times[False])), "replays_each": REPLAYS, "kernels_added": 1,
                                   "what": "two captured graphs replayed alternately in this run, same start state; the baseline is the graph without FlightClearance.update(); the added time is a difference of medians and is below the spread when the spread says so; recorded, not asserted"},
            "eager_ms_per_update": dict(stat(eager), calls_per_window=200, what="FlightClearance.update() back to back between two events, ctypes marshalling included"),
            "what_the_last_replay_saw": seen}


def run(reps=9, B=4096, REPLAYS=40):
    assert torch.cuda.is_available(), "occmap_distance_bench needs a GPU"
    rng = np.random.default_rng(0)
    maps = {"pillars_20x20x4": solver.OccupancyMap(workloads.astar_world(2, "pillars", n_obstacles=12))}
    ref_map = solver.OccupancyMap(origin=(-20.0, -20.0, 0.0), map_size=(40.0, 40.0, 5.0), resolution=0.1)
    ref_map.insert_cloud(torch.from_numpy(pillar_cloud(rng, 25, (-18, -18), (18, 18), 3.0)).to(DEV))
    maps["reference_40x40x5"] = ref_map
    res = {"device": torch.cuda.get_device_name(0),
           "method": "ms per call from windows of back-to-back calls between two device events; variants alternate window by window; median, min, max and std over the windows",
           "update": {name: update_bench(name, dm, reps) for name, dm in maps.items()}}
    res["flight_clearance"] = flight_bench(ref_map, B, REPLAYS)
    return res


if __name__ == "__main__":
    a = sys.argv[1:]
    res = run(int(a[0]) if len(a) > 0 else 9, int(a[1]) if len(a) > 1 else 4096, int(a[2]) if len(a) > 2 else 40)
    out = a[3] if len(a) > 3 else os.path.join(ROOT, "profiles", "occmap_distance_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["flight_clearance"]))
