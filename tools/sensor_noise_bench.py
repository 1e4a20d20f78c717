#!/usr/bin/env python3
"""The sensor noise (include/frp_nmpc.h section 16, solver.SensorNoise) measured -> profiles/sensor_noise_bench.json.
   python tools/sensor_noise_bench.py [--replays 40] [--reps 20] [--windows 7] [--out FILE]      on the GPU: (a), (b), (c)
   python tools/sensor_noise_bench.py --resources [--out FILE]                                   where the objects were built: (d)
 (a) The period: 4096 vehicles, S = 5 -- the period graph of tools/disturbance_bench.py (plain vehicle step, message, odometry), captured
     twice, without and with a SensorNoise attached (all three state channels and the bias on: Vehicle.step launches
     frp_nmpc_sensor_noise_states, the message is built from its y), replayed ALTERNATELY from the same start state; medians, the standard
     deviation of a replay, and the difference of the medians.
 (b) Depth: SensorNoise.depth on the 16 frames of 480 x 640 that tools/render_bench.py renders, next to render_depth and
     fuse_depth_batch of the same frames, the three calls alternated window by window in one run; pixels/s and bytes/s (2 B read + 2 B
     written per pixel) of the noise.  Once more with p_drop = 1 (every pixel with a return is lost before its normal is drawn: the
     kernel without its logarithm, square root and cosine) -- the evidence for what bounds it.
 (c) Scan: SensorNoise.scan on 16 scans of 76 241 float64 points, next to fuse_points of the same points, alternated likewise.
 (d) VGPRs, SGPRs and scratch of the kernels, from the metadata notes of the gfx950 code object inside the unit's object file.
Each part keeps what the file already holds of the others.  No device: (a)-(c) fail."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "sensor_noise_bench.json")
NOISE = dict(sigma_p=(0.02, 0.02, 0.03), sigma_v=(0.05, 0.05, 0.08), sigma_a=(0.01, 0.01, 0.02), sigma_bias=(0.1, 0.1, 0.2), tau_bias=(5.0, 5.0, 2.0),
             depth=dict(sigma0=0.002, sigma2=0.0005, p_drop=0.02), scan=dict(sigma0=0.01, sigma1=0.002, p_drop=0.02), seed=1)


def resources():
    from forces_resilient_planner_amd import build
    obj = os.path.join(build.OBJDIR, "frp_sensor_noise.hip.o")
    llvm = "/opt/rocm/lib/llvm/bin"
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fatbin.bin"), os.path.join(d, "dev.co")
        subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, obj, os.path.join(d, "copy.o")])
        subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fb, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    out = {}
    for block in notes.split("- .agpr_count:")[1:]:
        get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.search(r"sensor_noise\d+(\w+?)_kernel", name)
        out[m.group(1) if m else name] = dict(vgpr=get("vgpr_count"), sgpr=get("sgpr_count"), agpr=int(re.match(r"\s*(\d+)", block).group(1)),
                                              scratch_bytes=get("private_segment_fixed_size"), lds_bytes=get("group_segment_fixed_size"),
                                              vgpr_spills=get("vgpr_spill_count"), sgpr_spills=get("sgpr_spill_count"))
    return {"source": "the amdhsa metadata notes of the gfx950 code object in frp_sensor_noise.hip.o (llvm-readelf --notes)", "kernels": out}


def windows_ms(fns, reps, windows):
    """Device events around `reps` back-to-back calls of each function, the functions ALTERNATED window by window: {name: stats}."""
    import torch
    ms = {k: [] for k in fns}
    for k, fn in fns.items():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(windows):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    return {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), std=float(np.std(v))) for k, v in ms.items()}


def period(B, REPLAYS):
    import torch
    from forces_resilient_planner_amd import layout as L, solver
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
    noise = solver.SensorNoise(veh, **NOISE)
    veh.noise = None                                                     # attached per graph below
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
        veh.reset(x_start); veh.state.copy_(x_start); noise.reset()

    def chain(with_noise, stream):
        nonlocal out
        fsm.goal(goal, fresh, stream); fsm.force(force, ffresh, stream); fsm.safety_verdict(blocked, first_hit, stream)
        fsm.exec_begin(d_state, t_step, now, *bufs, stream=stream); fsm.exec_end(status, now, stream)
        fleet.full_tick(fsm.external_acc, d_path, toff, d_cloud, fsm.ref_pos, fsm.ref_yaw, stream=stream, grid=grid, state=d_state, tick=ts, end_pt=fsm.end_pt)
        fsm.mpc_result(stream=stream)
        out = fleet.commands(t_cmd, ts.cmd_status, ts.pub_end, ts.cmd_end_pt, odom=fsm.yaw_odom, init_yaw=fsm.init_yaw, t_yaw=t_cmd, out=out, stream=stream)
        veh.noise = noise if with_noise else None
        veh.step(out, stream)
        veh.odometry(fsm, stream=stream)
        veh.noise = None

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
    stat = lambda a: {"median": float(np.median(a)), "mean": float(np.mean(a)), "std_of_a_replay": float(np.std(a)), "min": float(np.min(a))}
    parent = None
    p = os.path.join(ROOT, "profiles", "disturbance_bench.json")
    if os.path.exists(p):
        with open(p) as f:
            parent = json.load(f).get("in_period_graph_ms", {}).get("period_with_plain_step", {}).get("median")
    return {"workload": f"{B} vehicles, S = {S}, n_sub = {N_SUB}, the period of tools/disturbance_bench.py with the plain step; noise: {NOISE}",
            "period_without_noise": stat(times[False]), "period_with_noise": stat(times[True]),
            "added_ms_median": float(np.median(times[True]) - np.median(times[False])), "replays_each": REPLAYS,
            "largest_measurement_error_in_the_last_replay": float((noise.y - veh.x).abs().amax().item()),
            "tick_min_max_after_the_last_replay": (int(noise.tick.min().item()), int(noise.tick.max().item())),
            "what": "two captured graphs replayed alternately, same start state; the added time is a difference of medians and means nothing where it is below the "
                    "spread of a replay",
            "context_only_plain_step_period_recorded_by_the_parent_ms (profiles/disturbance_bench.json)": parent}


def depth_and_scan(reps, windows):
    import torch
    from forces_resilient_planner_amd import solver, workloads
    from tests import occmap_fusion_oracle as FO
    from tools import render_bench as RB
    w = workloads.astar_world(seed=0, kind="pillars")
    T = RB.poses()
    world = solver.OccupancyMap(world=w, **FO.LAUNCH_CLAMPS)
    belief = solver.OccupancyMap(origin=w["origin"], map_size=w["map_size"], resolution=w["resolution"], **FO.LAUNCH_CLAMPS)
    dev = world.device
    F, ROWS, COLS = RB.F, RB.ROWS, RB.COLS
    Td = torch.from_numpy(T).to(dev)
    depth = torch.zeros((F, ROWS, COLS), dtype=torch.int16, device=dev).view(torch.uint16)
    noisy = torch.zeros((F, ROWS, COLS), dtype=torch.int16, device=dev).view(torch.uint16)
    rstatus, fstatus = torch.zeros((F, 2), dtype=torch.int32, device=dev), torch.zeros((F, 2), dtype=torch.int32, device=dev)
    fleet = type("Fleet", (), dict(torch=torch, B=F, solver=type("S", (), dict(device=torch.device(dev)))()))()
    veh = solver.Vehicle(fleet)
    noise = solver.SensorNoise(veh, **NOISE)
    lossy = solver.SensorNoise(solver.Vehicle(fleet), **dict(NOISE, depth=dict(NOISE["depth"], p_drop=1.0)))
    world.render_depth(Td, RB.K, ROWS, COLS, max_range=RB.MAX_RANGE, out=depth, status=rstatus)
    torch.cuda.synchronize()
    returns = int(rstatus[:, 1].sum().item())
    res = {}
    d = windows_ms({"noise_depth": lambda: noise.depth(depth, out=noisy),
                    "noise_depth_every_return_dropped_before_its_normal": lambda: lossy.depth(depth, out=noisy),
                    "render_depth": lambda: world.render_depth(Td, RB.K, ROWS, COLS, max_range=RB.MAX_RANGE, out=depth, status=rstatus),
                    "fuse_depth_batch": lambda: belief.fuse_depth_batch(noisy, RB.K, Td, status=fstatus)}, reps, windows)
    npix = F * ROWS * COLS
    t = d["noise_depth"]["median"] * 1e-3
    res["depth"] = {"frames": F, "image": [ROWS, COLS], "pixels": npix, "pixels_with_a_return": returns, "ms_per_call": d,
                    "pixels_per_second": npix / t, "returns_per_second": returns / t, "bytes_per_second (2 B read + 2 B written per pixel)": 4 * npix / t,
                    "timing": f"device events around {reps} back-to-back calls, {windows} windows per call, the calls alternated window by window; two launches per noise call"}
    # (c) 16 scans of 76 241 points around the cameras' positions, 1 ... 6 m away
    S, P = 16, 76241
    rng = np.random.default_rng(1)
    dirs = rng.normal(size=(S, P, 3)); dirs /= np.linalg.norm(dirs, axis=2, keepdims=True)
    origin_h = np.ascontiguousarray(T[:, :3, 3])
    pts = torch.from_numpy(origin_h[:, None, :] + dirs * rng.uniform(1.0, 6.0, (S, P, 1))).to(dev)
    origin = torch.from_numpy(origin_h).to(dev)
    count = torch.full((S,), P, dtype=torch.int32, device=dev)
    out = torch.empty_like(pts)
    pstatus = torch.zeros((S, 2), dtype=torch.int32, device=dev)
    c = windows_ms({"noise_scan": lambda: noise.scan(pts, origin, count=count, out=out),
                    "fuse_points": lambda: belief.fuse_points(out, origin, count=count, status=pstatus)}, reps, windows)
    t = c["noise_scan"]["median"] * 1e-3
    res["scan"] = {"scans": S, "points_per_scan": P, "ms_per_call": c, "points_per_second": S * P / t,
                   "bytes_per_second (24 B read + 24 B written per point)": 48 * S * P / t, "lost_points_in_the_last_call": int(torch.isnan(out[..., 0]).sum().item())}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--replays", type=int, default=40)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--base", default=OUT, help="the file whose other parts are kept")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    res = {}
    if os.path.exists(a.base):
        with open(a.base) as f:
            res = json.load(f)
    if a.resources:
        res["kernel_resources"] = resources()
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("sensor_noise_bench measures on the GPU: no device, nothing is reported")
        res["device"] = torch.cuda.get_device_name(0)
        res["period"] = period(a.B, a.replays)
        res.update(depth_and_scan(a.reps, a.windows))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
