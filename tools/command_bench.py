#!/usr/bin/env python3
"""The command timer (frp_nmpc_command_batch, include/frp_nmpc_command.h) for a fleet: ms per call, eager and inside the replayed tick
graph, and the number of launches a call makes.
   python tools/command_bench.py [B=4096] [S=5] [calls=2000] [replays=40] [out=profiles/command_bench.json]
  eager     `calls` back-to-back DeviceFleet.commands calls between two HIP events on the launch stream, after a warm-up of 50: the
            enqueue rate of a one-kernel call, i.e. one launch's cost
  in graph  two captured graphs, full_tick -> snapshot_commands and full_tick -> snapshot_commands -> commands, replayed alternately
            (`replays` pairs, plans reset before each); the timer's share is the difference of the two means, its spread the
            standard deviation of the per-replay times
  launches  frp_nmpc_command_batch captured alone on a stream of the runtime the library links; the kernel nodes of the graph
No device: the tool fails."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from forces_resilient_planner_amd import layout as L  # noqa: E402
from forces_resilient_planner_amd import solver  # noqa: E402


def count_launches(c):
    """Kernel nodes of one captured frp_nmpc_command_batch call (the struct c holds live device pointers)."""
    # the HIP runtime of this process: the one torch loaded first, which the library binds to as well (solver.lib())
    loaded = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln})
    if len(loaded) != 1:
        raise RuntimeError(f"expected one HIP runtime in the process, found {loaded}")
    hip = ctypes.CDLL(loaded[0])
    vp = ctypes.c_void_p
    stream, graph, n = vp(), vp(), ctypes.c_size_t(0)
    chk = lambda rc, what: (_ for _ in ()).throw(RuntimeError(f"{what} failed: {rc}")) if rc != 0 else None
    chk(hip.hipStreamCreate(ctypes.byref(stream)), "hipStreamCreate")
    chk(hip.hipStreamBeginCapture(stream, 2), "hipStreamBeginCapture")   # hipStreamCaptureModeRelaxed
    rc = solver.lib().frp_nmpc_command_batch(ctypes.byref(c), stream)
    chk(hip.hipStreamEndCapture(stream, ctypes.byref(graph)), "hipStreamEndCapture")
    chk(rc, "frp_nmpc_command_batch under capture")
    chk(hip.hipGraphGetNodes(graph, None, ctypes.byref(n)), "hipGraphGetNodes")
    nodes = (vp * n.value)()
    chk(hip.hipGraphGetNodes(graph, nodes, ctypes.byref(n)), "hipGraphGetNodes")
    kernels = 0
    for k in range(n.value):
        ty = ctypes.c_int(-1)
        chk(hip.hipGraphNodeGetType(vp(nodes[k]), ctypes.byref(ty)), "hipGraphNodeGetType")
        kernels += ty.value == 0          # hipGraphNodeTypeKernel
    hip.hipGraphDestroy(graph); hip.hipStreamDestroy(stream)
    return dict(graph_nodes=int(n.value), kernel_nodes=int(kernels))


def run(B=4096, S=5, CALLS=2000, REPLAYS=40):
    assert torch.cuda.is_available(), "command_bench needs a GPU"
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
    grid = solver.CloudGrid(d_cloud, 0.5)
    rp = torch.zeros((B, N, 3), dtype=torch.float64, device=dev); ry = torch.zeros((B, N), dtype=torch.float64, device=dev)
    toff = fleet.to_device(rng.uniform(0, 0.01, B))
    # the 100 Hz timer against a 20 Hz tick: five callbacks 10 ms apart; a fleet in flight (PUB_TRAJ) with a few planners in every other state
    t_cur = fleet.to_device(rng.uniform(0.0, 0.01, (B, 1)) + 0.01 * np.arange(S)[None, :])
    st0 = np.full(B, solver.CMD_PUB_TRAJ, dtype=np.int32); st0[::17] = solver.CMD_ROTATE_YAW; st0[5::29] = solver.CMD_PUB_END; st0[7::31] = solver.CMD_WAIT
    d_st0 = fleet.to_device(st0); status = d_st0.clone()
    pub_end = torch.zeros((B,), dtype=torch.int32, device=dev); end_pt = fleet.to_device(rng.uniform(-8, 8, (B, 3)))
    odom = fleet.to_device(rng.uniform(-3, 3, (B, 9))); init_yaw = fleet.to_device(rng.uniform(-3, 3, B)); t_yaw = t_cur.clone()
    fleet.mpc_output.copy_(d_plan)
    fleet.full_tick(d_f, d_path, toff, d_cloud, rp, ry, grid=grid)
    fleet.snapshot_commands()
    out = fleet.commands(t_cur, status, pub_end, end_pt, odom, init_yaw, t_yaw)
    torch.cuda.synchronize()
    kinds = {int(k): int((out.kind == k).sum().item()) for k in torch.unique(out.kind).tolist()}
    call = lambda stream=None: fleet.commands(t_cur, status, pub_end, end_pt, odom, init_yaw, t_yaw, out=out, stream=stream)
    # ---- eager ----
    eager = []
    for _ in range(3):
        status.copy_(d_st0)
        for _ in range(50):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            call()
        e1.record(); torch.cuda.synchronize()
        eager.append(e0.elapsed_time(e1) / CALLS)
    # ---- inside the replayed tick graph ----
    def chain(with_timer, stream):
        fleet.full_tick(d_f, d_path, toff, d_cloud, rp, ry, stream=stream, grid=grid)
        fleet.snapshot_commands(stream=stream)
        if with_timer:
            call(stream)
    side = torch.cuda.Stream()
    graphs = {}
    for with_timer in (False, True):
        with torch.cuda.stream(side):
            chain(with_timer, side)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            chain(with_timer, torch.cuda.current_stream())
        graphs[with_timer] = g
    times = {False: [], True: []}
    for r in range(REPLAYS + 5):
        for with_timer in (False, True):
            fleet.mpc_output.copy_(d_plan); status.copy_(d_st0); fleet.solver.exitflag.fill_(1)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); graphs[with_timer].replay(); e1.record(); torch.cuda.synchronize()
            if r >= 5:
                times[with_timer].append(e0.elapsed_time(e1))
    m0, m1 = float(np.mean(times[False])), float(np.mean(times[True]))
    # ---- launches ----
    c = solver.Command(B, N, S, 0.05, 0.74, 9.81, fleet.pre_plan.data_ptr(), t_cur.data_ptr(), status.data_ptr(), fleet.have_traj.data_ptr(),
                       pub_end.data_ptr(), end_pt.data_ptr(), odom.data_ptr(), init_yaw.data_ptr(), t_yaw.data_ptr(), out.cmd.data_ptr(),
                       out.kind.data_ptr(), out.finish.data_ptr(), out.reset_output.data_ptr())
    try:
        launches = count_launches(c)
    except Exception as e:  # (the timings above are still written; the tool then exits with an error)
        launches = {"error": repr(e)}
    torch.cuda.synchronize()
    return {"workload": f"{B} planners x {S} callbacks, N = {N}; kinds of the warm-up call (kind: samples): {kinds}",
            "device": torch.cuda.get_device_name(0),
            "eager_ms_per_call": {"mean_of_3_windows": float(np.mean(eager)), "windows": eager, "calls_per_window": CALLS,
                                  "what": "back-to-back calls between two events on the launch stream: the enqueue-bound cost of one launch"},
            "in_tick_graph_ms": {"tick_and_snapshot": m0, "tick_snapshot_and_timer": m1, "timer_share": m1 - m0,
                                 "std_of_a_replay": [float(np.std(times[False])), float(np.std(times[True]))], "replays_each": REPLAYS,
                                 "what": "two captured graphs replayed alternately, same start state; the share is a difference of means and is below the spread when the spread says so"},
            "launches_per_call": launches}


if __name__ == "__main__":
    a = sys.argv[1:]
    res = run(int(a[0]) if len(a) > 0 else 4096, int(a[1]) if len(a) > 1 else 5, int(a[2]) if len(a) > 2 else 2000, int(a[3]) if len(a) > 3 else 40)
    out = a[4] if len(a) > 4 else os.path.join(ROOT, "profiles", "command_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if res["launches_per_call"] != {"graph_nodes": 1, "kernel_nodes": 1}:
        sys.exit("frp_nmpc_command_batch is meant to be ONE launch: " + json.dumps(res["launches_per_call"]))
