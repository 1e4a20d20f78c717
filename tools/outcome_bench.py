#!/usr/bin/env python3
"""The tick outcome (frp_nmpc_tick_begin / frp_nmpc_tick_end, include/frp_nmpc_outcome.h) for a fleet: what it adds to the replayed tick
graph, and the two kernels eagerly.
   python tools/outcome_bench.py [B=4096] [calls=2000] [replays=40] [out=profiles/outcome_bench.json]
  in graph  two captured graphs, full_tick -> snapshot_commands (the tick as it was) and full_tick(tick=...) (tick_begin and tick_end
            added, the masks taken from them), replayed alternately (`replays` pairs, plans and state reset before each); the added
            time is the difference of the two medians, its spread the standard deviation of the per-replay times
  gated     the same graph with a quarter and with all of the fleet gated (exec_mpc = 0): gated planners stay in the batch and their
            solve is discarded, so the tick costs what it costs with everyone running -- the figure says whether that holds
  eager     `calls` back-to-back calls of each entry point between two HIP events on the launch stream, after a warm-up of 50: the
            enqueue rate of a one-kernel call
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


def run(B=4096, CALLS=2000, REPLAYS=40):
    assert torch.cuda.is_available(), "outcome_bench needs a GPU"
    dev = "cuda:0"
    N, M, F, K = 20, 30, 64, 120
    rng = np.random.default_rng(0)
    s = np.arange(K) * 0.05 * 1.6
    path = np.c_[s, 0.4 * np.sin(0.8 * s), 1.0 + 0.1 * np.cos(s)]
    cloud = np.c_[rng.uniform(-3, 12, 20000), rng.uniform(-4, 4, 20000), rng.uniform(-0.5, 3, 20000)]
    cx = np.interp(cloud[:, 0], path[:, 0], path[:, 1]); cz = np.interp(cloud[:, 0], path[:, 0], path[:, 2])
    cloud = cloud[np.hypot(cloud[:, 1] - cx, cloud[:, 2] - cz) > 0.9]
    plan = np.zeros((B, N + 1, 17)); plan[..., 3] = 7.3; plan[..., 7] = 7.3
    plan[..., 8:11] = path[0] + rng.normal(0, 0.02, (B, 1, 3)); plan[..., 16] = 0.2
    fleet = solver.DeviceFleet(B, N, M, F, L.MODEL_NORMAL, (15.0, 3.0, 80.0, 15.0, 0.0))
    fleet.poly_index = torch.zeros((B, N), dtype=torch.int32, device=dev)
    d_plan, d_path, d_cloud, d_f = fleet.to_device(plan), fleet.to_device(path), fleet.to_device(cloud), fleet.to_device(rng.normal(0, 0.5, (B, 3)))
    d_state, d_end = fleet.to_device(plan[:, 1, 8:17].copy()), fleet.to_device(path[-1].copy())
    grid = solver.CloudGrid(d_cloud, 0.5)
    rp = torch.zeros((B, N, 3), dtype=torch.float64, device=dev); ry = torch.zeros((B, N), dtype=torch.float64, device=dev)
    toff = fleet.to_device(rng.uniform(0, 0.01, B))
    ts = solver.TickState(fleet)
    ts.path_size(K)
    exec_mpc = torch.ones((B,), dtype=torch.int32, device=dev)

    def reset_state():
        fleet.mpc_output.copy_(d_plan); fleet.solver.exitflag.fill_(1); fleet.solver.iters.zero_()
        for k in ("fail_count", "replan_count", "kino_replan", "pub_end"):
            getattr(ts, k).zero_()
        ts.initialized.fill_(1); ts.exit_code.fill_(1); ts.cmd_status.fill_(solver.CMD_PUB_TRAJ); ts.exec_mpc.copy_(exec_mpc)

    def chain(with_outcome, stream):
        if with_outcome:
            fleet.full_tick(d_f, d_path, toff, d_cloud, rp, ry, stream=stream, grid=grid, state=d_state, tick=ts, end_pt=d_end)
        else:
            fleet.full_tick(d_f, d_path, toff, d_cloud, rp, ry, stream=stream, grid=grid, state=d_state)
            fleet.snapshot_commands(stream=stream)

    reset_state()
    side = torch.cuda.Stream()
    graphs = {}
    for with_outcome in (False, True):
        with torch.cuda.stream(side):
            chain(with_outcome, side)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            chain(with_outcome, torch.cuda.current_stream())
        graphs[with_outcome] = g

    def replay_pairs(which):
        times = {w: [] for w in which}
        for r in range(REPLAYS + 5):
            for w in which:
                reset_state()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); graphs[w].replay(); e1.record(); torch.cuda.synchronize()
                if r >= 5:
                    times[w].append(e0.elapsed_time(e1))
        return times

    t = replay_pairs((False, True))
    results = {int(k): int((ts.result == k).sum().item()) for k in torch.unique(ts.result).tolist()}
    stat = lambda a: {"median": float(np.median(a)), "mean": float(np.mean(a)), "std_of_a_replay": float(np.std(a)), "min": float(np.min(a))}
    in_graph = {"tick_and_snapshot": stat(t[False]), "tick_with_outcome": stat(t[True]),
                "added_ms_median": float(np.median(t[True]) - np.median(t[False])), "replays_each": REPLAYS,
                "results_of_the_last_replay (result: planners)": results,
                "what": "two captured graphs replayed alternately, same start state; the added time is a difference of medians and is below the spread when the spread says so"}
    gated = {}
    for name, frac in (("quarter_idle", 4), ("all_idle", 1)):
        exec_mpc.fill_(1); exec_mpc[::frac] = 0
        g = replay_pairs((True,))[True]
        gated[name] = dict(stat(g), idle_planners=int((exec_mpc == 0).sum().item()))
    exec_mpc.fill_(1)
    gated["what"] = "tick_with_outcome with part of the fleet gated: the batch is not compacted, a gated planner's stages run and are discarded"
    # ---- eager ----
    reset_state()
    reset = torch.zeros((B,), dtype=torch.int32, device=dev)
    ds = fleet.solver
    ksize = ts.path_size(K)
    calls = {"tick_begin": lambda: ts.begin(reset),
             "tick_end": lambda: ts.end(ds.z, ds.exitflag, fleet.mpc_output, d_state, d_end, d_path, ksize, toff)}
    eager = {}
    for name, call in calls.items():
        w = []
        for _ in range(3):
            for _ in range(50):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                call()
            e1.record(); torch.cuda.synchronize()
            w.append(e0.elapsed_time(e1) / CALLS)
        eager[name] = {"mean_of_3_windows": float(np.mean(w)), "windows": w}
    eager["calls_per_window"] = CALLS
    eager["what"] = "back-to-back calls between two events on the launch stream: the enqueue-bound cost of one launch (ctypes marshalling included)"
    return {"workload": f"{B} planners, N = {N}, the tick of tools/command_bench.py", "device": torch.cuda.get_device_name(0),
            "in_tick_graph_ms": in_graph, "gated_fleet_ms": gated, "eager_ms_per_call": eager}


if __name__ == "__main__":
    a = sys.argv[1:]
    res = run(int(a[0]) if len(a) > 0 else 4096, int(a[1]) if len(a) > 1 else 2000, int(a[2]) if len(a) > 2 else 40)
    out = a[3] if len(a) > 3 else os.path.join(ROOT, "profiles", "outcome_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
