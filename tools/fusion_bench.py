"""Depth-image fusion on the device (include/frp_nmpc_occmap_fuse.h, solver.OccupancyMap.fuse_depth) at the reference's
configuration -> profiles/occmap_fusion_bench.json: a 400 x 400 x 50 map at 0.1 m, 640 x 480 frames, skip_pixel 2, margin 1, ray
lengths 0.1 / 6.0 m, the launch file's log-odds values; synthetic scenes: those of tests/occmap_fusion_oracle.py\nat that image size and a ground plane (scene()).
Per scene:
  * ms per frame (device events over `reps` frames after a warm-up, `windows` windows: median and spread), at the default round
    cap, with the cap set to the rounds the frame needs, and replayed from a captured hipGraph;
  * rounds used and rays cast (the status words), checked against the counts of the CPU port;
  * cells the serial scan processes against cells of the full paths (what the rounds walk), from the CPU port;
  * the host time of tools/fusion_serial.cpp -- a single-thread C++ PORT of the serial scan, not the reference -- on this host.
The share of the mark pass needs per-kernel times: run `--profile N` (N frames per scene, nothing timed) under
rocprofv3 --kernel-trace --stats --output-format csv, then `--merge-stats <..._kernel_stats.csv>` adds the shares to the JSON.
Reported, not gated: there is no earlier device number to hold these against.
`--frames F` (device): F frames (the scenes in turn, cameras on a circle of 3 m, each turned 0.3 rad off its radius, so that neighbouring ray boxes
overlap) through ONE solver.OccupancyMap.fuse_depth_batch call and through F fuse_depth calls, each path in a child process of its
own under its own time limit, one after the other; ms per F frames, the round counts and whether both maps are the same bytes go
under the key "batch" of the JSON (the rest of the file is kept).
   python tools/fusion_bench.py [--reps 50] [--windows 5] | --cpu-only | --profile N | --merge-stats CSV | --frames F"""
import argparse
import csv
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from forces_resilient_planner_amd import solver  # noqa: E402
from tests import occmap_fusion_oracle as FO  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "occmap_fusion_bench.json")
GEO = dict(origin=(-20.0, -20.0, 0.0), map_size=(40.0, 40.0, 5.0), resolution=0.1)
ROWS, COLS = 480, 640
K = np.array([[386.0, 0.0, 319.5], [0.0, 386.0, 239.5], [0.0, 0.0, 1.0]])   # a 640 x 480 depth camera with a 79 degree field of view
T_WC = FO.pose((0.03, -0.02, 1.61))
SCENES = ("wall", "steps", "random", "floor")
KERNELS = ("init", "project", "setup", "mark", "stop", "status", "count", "update")


def scene(name):
    """The oracle's test scenes at 640 x 480, and "floor": a ground plane 1.61 m under the camera below the image centre (depth
    h * fy / (v - cy), up to 6.5 m) under a wall at 4 m -- neighbouring rows graze the same voxels, the long dependence chains."""
    if name != "floor":
        return FO.scene(name, rows=ROWS, cols=COLS)
    v = np.arange(ROWS, dtype=np.float64)[:, None].repeat(COLS, 1)
    z = np.where(v > K[1, 2] + 1.0, 1610.0 * K[1, 1] / np.maximum(v - K[1, 2], 1.0), 4000.0)
    return np.ascontiguousarray(np.minimum(z, 6500.0).astype(np.uint16))


def frame_file(path, depth):
    d = FO.FUSE_DEFAULTS
    grid = [int(np.ceil(m / GEO["resolution"])) for m in GEO["map_size"]]
    head = struct.pack("<8i37d", ROWS, COLS, d["depth_filter_margin"], d["skip_pixel"], *grid, 0, *GEO["origin"], GEO["resolution"],
                       *K.ravel(), *T_WC.ravel(), d["depth_scale"], d["depth_filter_mindist"], d["prob_hit_log"], d["prob_miss_log"],
                       d["min_ray_length"], d["max_ray_length"], FO.LAUNCH_CLAMPS["clamp_min_log"], FO.LAUNCH_CLAMPS["clamp_max_log"])
    with open(path, "wb") as f:
        f.write(head)
        f.write(np.ascontiguousarray(depth, dtype="<u2").tobytes())


def cpu_port(tmp, reps):
    """Build tools/fusion_serial.cpp and run it on every scene: {scene: its JSON line}."""
    exe = os.path.join(tmp, "fusion_serial")
    cxx = os.environ.get("CXX", "c++")
    subprocess.run([cxx, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "fusion_serial.cpp")], check=True)
    out = {}
    for name in SCENES:
        path = os.path.join(tmp, name + ".bin")
        frame_file(path, scene(name))
        r = subprocess.run([exe, path, str(reps)], check=True, capture_output=True, text=True)
        out[name] = json.loads(r.stdout)
        out[name]["compiler"] = f"{cxx} -O2"
        print(name, out[name], flush=True)
    return out


def windows_ms(fn, reps, windows):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def device_map():
    return solver.OccupancyMap(**GEO, **FO.LAUNCH_CLAMPS)


def to_device(dm, depth):
    import torch
    return torch.from_numpy(depth.view(np.int16)).to(dm.device).view(torch.uint16)


def device_scene(name, port, reps, windows):
    import torch
    dm = device_map()
    depth = to_device(dm, scene(name))
    status = torch.zeros((2,), dtype=torch.int32, device=dm.device)
    dm.fuse_depth(depth, K, T_WC, status=status)
    torch.cuda.synchronize()
    rounds, rays = (int(v) for v in status.cpu())
    res = dict(rounds=rounds, rays=rays, default_cap=solver.OCCMAP_FUSE_DEFAULT_ROUNDS, launches_default=2 * solver.OCCMAP_FUSE_DEFAULT_ROUNDS + 6,
               matches_port=bool(rounds == port["rounds"] and rays == port["rays"]))
    res["ms_default_cap"] = windows_ms(lambda: dm.fuse_depth(depth, K, T_WC, status=status), reps, windows)
    if rounds > 0:
        res["ms_cap_at_rounds"] = windows_ms(lambda: dm.fuse_depth(depth, K, T_WC, status=status, max_rounds=rounds), reps, windows)
        assert int(status.cpu()[0]) == rounds
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(g, stream=side):
        dm.fuse_depth(depth, K, T_WC, status=status, stream=torch.cuda.current_stream())
    res["ms_graph_default_cap"] = windows_ms(g.replay, reps, windows)
    assert [int(v) for v in status.cpu()] == [rounds, rays]
    return res


def keep_batch(res):
    """The "batch" key of an earlier --frames run survives a rewrite of the rest of the file."""
    if os.path.exists(OUT):
        with open(OUT) as f:
            old = json.load(f)
        if "batch" in old:
            res["batch"] = old["batch"]
    return res


def batch_frames(F):
    """F frames for the --frames mode: [(depth, T_wc)]."""
    out = []
    for k in range(F):
        a = 2.0 * np.pi * k / F
        out.append((scene(SCENES[k % len(SCENES)]), FO.pose((3.0 * np.cos(a), 3.0 * np.sin(a), 1.61), yaw=a + 0.3)))
    return out


def frames_step(path, F, reps, windows):
    """One path of the --frames mode (a process of its own): "batch" = one fuse_depth_batch call, "single" = F fuse_depth calls.
    Prints one JSON line."""
    import torch
    frames = batch_frames(F)
    dm = device_map()
    T = np.ascontiguousarray(np.stack([t for _, t in frames]))
    if path == "batch":
        depth = to_device(dm, np.ascontiguousarray(np.stack([d for d, _ in frames])))
        Td = torch.from_numpy(T).to(dm.device)
        status = torch.zeros((F, 2), dtype=torch.int32, device=dm.device)

        def run(**kw):
            dm.fuse_depth_batch(depth, K, Td, status=status, **kw)
    else:
        depth = [to_device(dm, d) for d, _ in frames]
        status = torch.zeros((F, 2), dtype=torch.int32, device=dm.device)

        def run(**kw):
            for k in range(F):
                dm.fuse_depth(depth[k], K, T[k], status=status[k], **kw)
    run()
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    res = dict(path=path, rounds=[int(v) for v in st[:, 0]], rays=[int(v) for v in st[:, 1]],
               map_sha256=hashlib.sha256(dm.log_odds.cpu().numpy().tobytes() + dm.occ.cpu().numpy().tobytes() + dm.ws.cpu().numpy().tobytes()).hexdigest(),
               launches_default=(2 * solver.OCCMAP_FUSE_DEFAULT_ROUNDS + 7) if path == "batch" else F * (2 * solver.OCCMAP_FUSE_DEFAULT_ROUNDS + 6))
    res["ms_default_cap"] = windows_ms(run, reps, windows)
    top = max(res["rounds"])
    if top > 0:
        res["ms_cap_at_largest_rounds"] = windows_ms(lambda: run(max_rounds=top), reps, windows)
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(g, stream=side):
        run(stream=torch.cuda.current_stream())
    res["ms_graph_default_cap"] = windows_ms(g.replay, reps, windows)
    print(json.dumps(res), flush=True)


def frames_mode(F, reps, windows, limit):
    """Both paths one after the other, each in a child under its own time limit; the second is not started when the first failed."""
    out = {}
    for path in ("batch", "single"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--frames", str(F), "--frames-step", path, "--reps", str(reps), "--windows", str(windows)],
                           capture_output=True, text=True, timeout=limit)
        if r.returncode != 0:
            raise SystemExit(f"--frames: the {path} step failed ({r.returncode}), nothing more is started\n{r.stdout}\n{r.stderr}")
        out[path] = json.loads(r.stdout.strip().splitlines()[-1])
        print(path, json.dumps(out[path]), flush=True)
    b, s = out["batch"], out["single"]
    res = dict(F=F, image=[ROWS, COLS], grid=[400, 400, 50], reps=reps, windows=windows, rounds=b["rounds"], rays=b["rays"],
               same_status=bool(b["rounds"] == s["rounds"] and b["rays"] == s["rays"]), same_map=bool(b["map_sha256"] == s["map_sha256"]),
               what="ms per F frames: one fuse_depth_batch call against F fuse_depth calls, same session, one process each", batch=b, single=s)
    for k in ("ms_default_cap", "ms_cap_at_largest_rounds", "ms_graph_default_cap"):
        if k in b and k in s:
            res["batch_over_single_" + k[3:]] = b[k]["median"] / s[k]["median"]
    full = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            full = json.load(f)
    full["batch"] = res
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(full, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("batch", "single")}))


def merge_stats(path):
    """Per-kernel totals of a rocprofv3 kernel-stats CSV -> the share of every fusion kernel among the fusion kernels."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    tot = {}
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        ns = float(r.get("TotalDurationNs") or r.get("TotalDuration(ns)") or 0)
        for k in KERNELS:
            if f"fuse::{k}_kernel" in name:
                tot[k] = tot.get(k, 0.0) + ns
                tot.setdefault("_calls", {})[k] = int(float(r.get("Calls") or 0))
    calls = tot.pop("_calls", {})
    if "mark" not in tot:
        raise SystemExit(f"{path}: no frp::occmap::fuse kernels in it")
    total = sum(tot.values())
    with open(OUT) as f:
        res = json.load(f)
    res["kernel_share"] = dict(source="rocprofv3 --kernel-trace --stats, a run of its own over every scene (--profile)", total_ns=total, calls=calls,
                               share={k: v / total for k, v in tot.items()}, mark_pass_share=tot["mark"] / total)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["kernel_share"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--cpu-only", action="store_true", help="the counts and the port's host time only (no device needed)")
    ap.add_argument("--profile", type=int, default=0, metavar="N", help="fuse N frames per scene and exit (for a run under the profiler)")
    ap.add_argument("--merge-stats", metavar="CSV")
    ap.add_argument("--frames", type=int, default=0, metavar="F", help="F frames through fuse_depth_batch and through F fuse_depth calls -> the key \"batch\"")
    ap.add_argument("--frames-step", choices=("batch", "single"), help="(what --frames starts: one of its two paths, in this process)")
    ap.add_argument("--step-limit", type=float, default=240.0, help="time limit of each --frames step in seconds")
    a = ap.parse_args()
    if a.frames:
        if a.frames_step:
            return frames_step(a.frames_step, a.frames, a.reps, a.windows)
        return frames_mode(a.frames, a.reps, a.windows, a.step_limit)
    if a.merge_stats:
        return merge_stats(a.merge_stats)
    if a.profile:
        import torch
        for name in SCENES:
            dm = device_map()
            depth = to_device(dm, scene(name))
            for _ in range(a.profile):
                dm.fuse_depth(depth, K, T_WC)
            torch.cuda.synchronize()
        return
    with tempfile.TemporaryDirectory() as tmp:
        port = cpu_port(tmp, 10)
    if a.cpu_only:
        res = {"device": "not measured (--cpu-only)", "scenes": {name: {"cpu_port": port[name]} for name in SCENES},
               "largest_rounds": max(p["rounds"] for p in port.values())}
        with open(OUT, "w") as f:
            json.dump(keep_batch(res), f, indent=1)
        return
    import torch
    scanned = len(range(1, ROWS - 1, 2)) * len(range(1, COLS - 1, 2))
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows,
           "config": dict(map=GEO, grid=[400, 400, 50], image=[ROWS, COLS], scanned_pixels=scanned, K=K.tolist(), T_wc=T_WC.tolist(),
                          fuse=FO.FUSE_DEFAULTS, clamps=FO.LAUNCH_CLAMPS),
           "scenes": {}}
    for name in SCENES:
        r = device_scene(name, port[name], a.reps, a.windows)
        r["cpu_port"] = port[name]
        r["port_host_ms_over_device_ms"] = port[name]["host_ms_median"] / r["ms_default_cap"]["median"]
        res["scenes"][name] = r
        print(name, json.dumps(r), flush=True)
    res["largest_rounds"] = max(r["rounds"] for r in res["scenes"].values())
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(keep_batch(res), f, indent=1)


if __name__ == "__main__":
    main()
