"""Point-scan fusion (include/frp_nmpc_occmap_fuse_points.h, solver.OccupancyMap.fuse_points) against batched depth fusion on the SAME
rays -> profiles/fuse_points_bench.json.  The workload is the one fuse_depth_batch was measured on (DESIGN 9b "Batched fusion",
tools/fusion_bench.py --frames 16): 16 frames of 640 x 480 on the 400 x 400 x 50 map, the tool's four scenes in turn from cameras on a
3 m circle, the launch file's parameters.  The scans are those frames projected on the host (projectDepthImage's statements,
vectorised: every operation is one IEEE double operation per element, in the written order of tests/occmap_fusion_oracle.py), so
both routes cast the same rays in the same order; the tool checks that the status words and the bytes of log_odds, occ and the bit
plane after one pass are the same on all three routes before it times anything.

Timed, in ONE process, the three routes ALTERNATING window by window, their order rotating (device events around `reps` calls per window, after a warm-up):
  * fuse_depth_batch on the frames            -- the existing entry, untouched code path;
  * fuse_points on the scans as float64;
  * fuse_points on the scans as float32 (rounded once on the host; its rays are those of the rounded points, checked on their own).
Per route: median, p10, p90, min and max over the windows; the p10 - p90 spread of the depth route is the yardstick for a
difference.  Also recorded: launches per call, the rounds and rays per scan, the bytes of the fusion workspaces.
Where a difference comes from needs per-kernel times.  Both routes run the same stage kernels (frp::occmap::fuse::batch::, the only
copy in the library), so a trace cannot tell them apart: profile ONE route per run -- `--profile N --route depth` and `--profile N
--route points` (N calls of that route, nothing timed), each under rocprofv3 --kernel-trace --stats --output-format csv in a run of
its own -- then `--merge-stats <..._kernel_stats.csv> --route ROUTE --calls N` once per run adds that route's microseconds per call
and kernel to the JSON.
   python tools/fuse_points_bench.py [--frames 16] [--reps 10] [--windows 15] [--out FILE] | --profile N --route R | --merge-stats CSV --route R --calls N"""
import argparse
import csv
import ctypes
import re
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from forces_resilient_planner_amd import solver  # noqa: E402
from tests import occmap_fusion_oracle as FO  # noqa: E402
import fusion_bench as FB  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "fuse_points_bench.json")


def project(depth, K, T):
    """FusionOracle.project without the shift filter, vectorised: the points of one frame in scan order, [n, 3] float64."""
    d = FO.FUSE_DEFAULTS
    m, s = d["depth_filter_margin"], d["skip_pixel"]
    rows, cols = depth.shape
    v, u = np.meshgrid(np.arange(m, rows - m, s), np.arange(m, cols - m, s), indexing="ij")
    z = depth[v, u].astype(np.float64) / d["depth_scale"]
    keep = ~(z < d["depth_filter_mindist"])
    u, v, z = u[keep].astype(np.float64), v[keep].astype(np.float64), z[keep]            # boolean indexing keeps the row-major scan order
    x = (u - K[0, 2]) * z / K[0, 0]
    y = (v - K[1, 2]) * z / K[1, 1]
    return np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], axis=1)


def stats(ms):
    return dict(median=float(np.median(ms)), p10=float(np.percentile(ms, 10)), p90=float(np.percentile(ms, 90)), min=float(min(ms)), max=float(max(ms)),
                windows=[float(x) for x in ms])


def map_sha(dm):
    return hashlib.sha256(dm.log_odds.cpu().numpy().tobytes() + dm.occ.cpu().numpy().tobytes() + dm.ws[:dm.ws_bytes // 4].cpu().numpy().tobytes()).hexdigest()


def merge_stats(path, out, calls, route):
    """Per-kernel totals of a rocprofv3 kernel-stats CSV of a --profile --route run -> that route's microseconds per call and kernel."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    us = {}
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        ns = float(r.get("TotalDurationNs") or r.get("TotalDuration(ns)") or 0)
        m = re.search(r"fuse::(?:batch|points)::(\w+)_kernel", name)
        if m:
            us[m.group(1)] = us.get(m.group(1), 0.0) + ns / 1000.0 / calls
    if ("load" in us) != (route == "points") or ("project" in us) != (route == "depth"):
        raise SystemExit(f"{path}: not a trace of the {route} route alone (its first stage: {'load' if route == 'points' else 'project'})")
    with open(out) as f:
        res = json.load(f)
    k = res.setdefault("kernel_us_per_call", {})
    k["source"] = ("rocprofv3 --kernel-trace --stats, one run per route (--profile --route): depth = fuse_depth_batch, points = fuse_points on "
                   "float64 and float32 scans in equal numbers (load is the mean of the two)")
    k["calls_per_route"] = calls
    k[route], k[route + "_total"] = us, sum(us.values())
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(k))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", type=int, default=0, metavar="N", help="N calls of the --route, nothing timed")
    ap.add_argument("--route", choices=("depth", "points"), help="with --profile / --merge-stats: fuse_depth_batch, or fuse_points (half float64, half float32)")
    ap.add_argument("--merge-stats", metavar="CSV")
    ap.add_argument("--calls", type=int, default=0, help="with --merge-stats: the N of the --profile run")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if (a.merge_stats or a.profile) and not a.route:
        ap.error("--profile and --merge-stats take one --route per run: both routes run the same kernels")
    if a.merge_stats:
        return merge_stats(a.merge_stats, a.out, a.calls if a.calls > 0 else 1, a.route)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fuse_points_bench needs a GPU: nothing here is a CPU number")
    F = a.frames
    frames = FB.batch_frames(F)
    scans = [project(d, FB.K, T) for d, T in frames]
    P = max(len(p) for p in scans)
    pts = np.full((F, P, 3), np.nan)
    for k, p in enumerate(scans):
        pts[k, :len(p)] = p
    count_h = np.array([len(p) for p in scans], dtype=np.int32)
    T_h = np.ascontiguousarray(np.stack([T for _, T in frames]))

    maps = {k: FB.device_map() for k in ("depth", "points_f64", "points_f32", "points_f32_widened")}
    dev = maps["depth"].device
    depth = FB.to_device(maps["depth"], np.ascontiguousarray(np.stack([d for d, _ in frames])))
    Td = torch.from_numpy(T_h).to(dev)
    origin = torch.from_numpy(np.ascontiguousarray(T_h[:, :3, 3])).to(dev)
    count = torch.from_numpy(count_h).to(dev)
    p64 = torch.from_numpy(pts).to(dev)
    p32 = torch.from_numpy(pts.astype(np.float32)).to(dev)
    p32w = torch.from_numpy(pts.astype(np.float32).astype(np.float64)).to(dev)
    status = {k: torch.zeros((F, 2), dtype=torch.int32, device=dev) for k in maps}
    run = {"depth": lambda: maps["depth"].fuse_depth_batch(depth, FB.K, Td, status=status["depth"]),
           "points_f64": lambda: maps["points_f64"].fuse_points(p64, origin, count=count, status=status["points_f64"]),
           "points_f32": lambda: maps["points_f32"].fuse_points(p32, origin, count=count, status=status["points_f32"])}

    if a.profile:
        for k in range(a.profile):
            run["depth" if a.route == "depth" else "points_f64" if k % 2 == 0 else "points_f32"]()
        torch.cuda.synchronize()
        return

    # one pass of each: the same rays, the same map
    for k in run:
        run[k]()
    maps["points_f32_widened"].fuse_points(p32w, origin, count=count, status=status["points_f32_widened"])
    torch.cuda.synchronize()
    st = {k: status[k].cpu().numpy() for k in maps}
    sha = {k: map_sha(maps[k]) for k in maps}
    same = dict(status_depth_vs_f64=bool((st["depth"] == st["points_f64"]).all()), map_depth_vs_f64=bool(sha["depth"] == sha["points_f64"]),
                status_f32_vs_widened_f64=bool((st["points_f32"] == st["points_f32_widened"]).all()),
                map_f32_vs_widened_f64=bool(sha["points_f32"] == sha["points_f32_widened"]))
    print(json.dumps(same), flush=True)
    if not all(same.values()):
        raise SystemExit("the routes do not cast the same rays: nothing is timed")

    for _ in range(3):
        for k in run:
            run[k]()
    torch.cuda.synchronize()
    ms = {k: [] for k in run}
    order = list(run)
    for w in range(a.windows):
        for k in order[w % 3:] + order[:w % 3]:                         # alternating, the order rotating: whatever else the machine does, and whatever a position in the order is worth, hits every route alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                run[k]()
            e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.reps)

    m = maps["depth"]._map()
    fb = solver.OccMapFuseBatch()
    fb.frames, fb.rows, fb.cols = F, FB.ROWS, FB.COLS
    fb.K[:] = [float(x) for x in FB.K.ravel()]
    fp = solver.OccMapFusePoints()
    fp.scans, fp.P = F, P
    for k, val in solver.OCCMAP_FUSE_DEFAULTS.items():
        setattr(fb, k, val)
        if k in solver.OCCMAP_FUSE_POINTS_PARAMS:
            setattr(fp, k, val)
    res = dict(device=torch.cuda.get_device_name(0), F=F, image=[FB.ROWS, FB.COLS], grid=[400, 400, 50], P=P, points=[int(c) for c in count_h],
               reps=a.reps, windows=a.windows, what="ms per call of F frames / scans, the three routes alternating window by window in one process",
               same=same, rounds=[int(x) for x in st["depth"][:, 0]], rays=[int(x) for x in st["depth"][:, 1]],
               rounds_f32=[int(x) for x in st["points_f32"][:, 0]], rays_f32=[int(x) for x in st["points_f32"][:, 1]],
               launches_per_call=dict(depth=2 * solver.OCCMAP_FUSE_DEFAULT_ROUNDS + 7, points=2 * solver.OCCMAP_FUSE_DEFAULT_ROUNDS + 7),
               fuse_workspace_bytes=dict(depth=int(solver.lib().frp_nmpc_occmap_fuse_batch_workspace_bytes(ctypes.byref(m), ctypes.byref(fb))),
                                         points=int(solver.lib().frp_nmpc_occmap_fuse_points_workspace_bytes(ctypes.byref(m), ctypes.byref(fp)))),
               input_bytes=dict(depth=int(depth.numel() * 2), points_f64=int(p64.numel() * 8), points_f32=int(p32.numel() * 4)),
               ms={k: stats(v) for k, v in ms.items()})
    d = res["ms"]["depth"]
    res["depth_spread_p10_p90_ms"] = d["p90"] - d["p10"]
    for k in ("points_f64", "points_f32"):
        res[k + "_minus_depth_ms"] = res["ms"][k]["median"] - d["median"]
        res[k + "_within_depth_spread"] = bool(res["ms"][k]["median"] <= d["median"] + res["depth_spread_p10_p90_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("ms", "points")} | {"ms": {k: {q: v[q] for q in ("median", "p10", "p90")} for k, v in res["ms"].items()}}))


if __name__ == "__main__":
    main()
