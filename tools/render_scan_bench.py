"""The point-scan renderer (include/frp_nmpc_occmap_render_scan.h, solver.OccupancyMap.render_scan) at the size a fleet would run it ->
profiles/render_scan_bench.json: 16 scans of a 64-ring, 1024-column LiDAR (65 536 beams each, solver.lidar_beams(64, 1024, -0.4, 0.4))
on the map and poses of tools/fuse_points_bench.py -- the 400 x 400 x 50 map at 0.1 m, sensors on a 3 m circle at 1.61 m height.  That
tool's map starts empty, and an empty map has nothing to return: the map rendered here is what its 16 depth frames (tools/fusion_bench.py's
four scenes in turn) leave in it after three passes of fuse_depth_batch, i.e. a belief map as a fleet holds it.
Timed in ONE process on one stream, the routes ALTERNATING window by window (device events around `reps` calls per window, after a
warm-up):
  * render_scan, float64 points;
  * render_scan, float32 points;
  * render_depth on the same map at 16 frames of 480 x 640 from cameras at the same positions and headings -- the yardstick, whose
    3.7 x 10^11 ray steps per second on the pillars world DESIGN 9b quotes.
Per route: median, p10, p90, min and max over the windows, and lane-steps per second: the cells the rays enter, counted on the host by
a vectorised form of the specification's walk (every beam; every `--stride`-th pixel in both directions of the images, scaled up), over
the median time.  The host's count of returns is recorded beside the device's.  Reported, not gated.
   python tools/render_scan_bench.py [--reps 200] [--windows 15] [--stride 4] [--out profiles/render_scan_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from forces_resilient_planner_amd import solver  # noqa: E402
from tests import occmap_render_oracle as RO  # noqa: E402
import fusion_bench as FB  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "render_scan_bench.json")
S, RINGS, COLUMNS, ELEVATION = 16, 64, 1024, (-0.4, 0.4)
ROWS, COLS = FB.ROWS, FB.COLS
MAX_RANGE = 6.0


def sensor_poses(frames):
    """The LiDAR where each camera of the frames stands, x along the camera's optical axis, z up."""
    out = []
    for _, T in frames:
        fwd = T[:3, 2].copy(); fwd[2] = 0.0; fwd /= np.linalg.norm(fwd)
        Ts = np.eye(4)
        Ts[:3, 0], Ts[:3, 1], Ts[:3, 2], Ts[:3, 3] = fwd, np.cross([0.0, 0.0, 1.0], fwd), (0.0, 0.0, 1.0), T[:3, 3]
        out.append(Ts)
    return np.ascontiguousarray(np.stack(out))


def pinhole(stride):
    u, v = np.meshgrid(np.arange(0, COLS, stride, dtype=np.float64), np.arange(0, ROWS, stride, dtype=np.float64))
    return np.stack([((u - FB.K[0, 2]) / FB.K[0, 0]).ravel(), ((v - FB.K[1, 2]) / FB.K[1, 1]).ravel(), np.ones(u.size)], 1)


def count_steps(occ, origin, res, T, b):
    """(cells entered, returns) of the rays T * b: the walk of tests/occmap_scan_oracle.py, all rays at once."""
    R, t = T[:3, :3], T[:3, 3]
    d = np.stack([(R[i, 0] * b[:, 0] + R[i, 1] * b[:, 1]) + R[i, 2] * b[:, 2] for i in range(3)], 1)
    length = np.sqrt((d[:, 0] ** 2 + d[:, 1] ** 2) + d[:, 2] ** 2)
    c = np.floor((t - np.array(origin)) * (1.0 / res)).astype(np.int64)[None, :].repeat(len(d), 0)
    step = np.sign(d).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        face = np.array(origin)[None, :] + (c + (step > 0)) * res
        s_next = np.where(step != 0, (face - t[None, :]) / d, np.inf)
        s_step = np.where(step != 0, res / np.abs(d), np.inf)
    g = np.array(occ.shape)

    def occupied(c):
        inside = ((c >= 0) & (c < g)).all(1)
        cc = np.clip(c, 0, g - 1)
        return inside & (occ[cc[:, 0], cc[:, 1], cc[:, 2]] != 0)

    live = ~occupied(c)
    steps = returns = 0
    rows = np.arange(len(d))
    for _ in range(RO.step_bound(MAX_RANGE, res)):
        if not live.any():
            break
        a = np.where(s_next[:, 0] < s_next[:, 1], np.where(s_next[:, 0] < s_next[:, 2], 0, 2), np.where(s_next[:, 1] < s_next[:, 2], 1, 2))
        s_in = s_next[rows, a]
        live &= s_in * length <= MAX_RANGE
        steps += int(live.sum())
        c[rows[live], a[live]] += step[rows[live], a[live]]
        s_next[rows[live], a[live]] += s_step[rows[live], a[live]]
        hit = live & occupied(c)
        returns += int(hit.sum())
        live &= ~hit
    return steps, returns


def stats(ms):
    return dict(median=float(np.median(ms)), p10=float(np.percentile(ms, 10)), p90=float(np.percentile(ms, 90)), min=float(min(ms)), max=float(max(ms)),
                windows=[float(x) for x in ms])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--stride", type=int, default=4, help="the host's step count of the depth images looks at every stride-th pixel in both directions")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("render_scan_bench needs a GPU: nothing here is a CPU number")
    frames = FB.batch_frames(S)
    dm = FB.device_map()
    dev = dm.device
    depth_in = FB.to_device(dm, np.ascontiguousarray(np.stack([d for d, _ in frames])))
    T_wc = np.ascontiguousarray(np.stack([T for _, T in frames]))
    Tc = torch.from_numpy(T_wc).to(dev)
    for _ in range(3):                                                     # -1 -> 0.2 -> 1.4 -> 2.0 crosses min_occupancy_log = 1.7
        dm.fuse_depth_batch(depth_in, FB.K, Tc)
    torch.cuda.synchronize()
    occ = dm.occ.cpu().numpy()
    T_ws = sensor_poses(frames)
    beams_h = solver.lidar_beams(RINGS, COLUMNS, *ELEVATION)
    P = len(beams_h)
    Ts, beams = torch.from_numpy(T_ws).to(dev), torch.from_numpy(beams_h).to(dev)

    counted = [count_steps(occ, dm.origin, dm.resolution, T_ws[k], beams_h) for k in range(S)]
    scan_steps, scan_returns_host = sum(c[0] for c in counted), [c[1] for c in counted]
    px = pinhole(a.stride)
    counted = [count_steps(occ, dm.origin, dm.resolution, T_wc[k], px) for k in range(S)]
    depth_steps = sum(c[0] for c in counted) * a.stride * a.stride

    buf = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        buf[name] = dict(points=torch.zeros((S, P, 3), dtype=dt, device=dev), origin=torch.zeros((S, 3), dtype=torch.float64, device=dev),
                         count=torch.zeros((S,), dtype=torch.int32, device=dev), status=torch.zeros((S, 2), dtype=torch.int32, device=dev))
    image = torch.zeros((S, ROWS, COLS), dtype=torch.int16, device=dev).view(torch.uint16)
    dstatus = torch.zeros((S, 2), dtype=torch.int32, device=dev)
    run = {"scan_f64": lambda: dm.render_scan(Ts, beams, max_range=MAX_RANGE, **buf["f64"]),
           "scan_f32": lambda: dm.render_scan(Ts, beams, max_range=MAX_RANGE, **buf["f32"]),
           "depth": lambda: dm.render_depth(Tc, FB.K, ROWS, COLS, max_range=MAX_RANGE, out=image, status=dstatus)}
    for _ in range(3):
        for k in run:
            run[k]()
    torch.cuda.synchronize()
    returns = {k: [int(v) for v in buf[k]["status"].cpu().numpy()[:, 1]] for k in buf}
    ms = {k: [] for k in run}
    order = list(run)
    for w in range(a.windows):
        for k in order[w % 3:] + order[:w % 3]:                            # alternating, the order rotating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                run[k]()
            e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.reps)

    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, windows=a.windows,
               what="ms per call of 16 scans / 16 frames, the three routes alternating window by window in one process, one stream; device events "
                    "around `reps` back-to-back calls after 3 warm-up calls of each",
               config=dict(scans=S, rings=RINGS, columns=COLUMNS, elevation=list(ELEVATION), P=P, image=[ROWS, COLS], grid=[int(v) for v in occ.shape],
                           resolution=dm.resolution, max_range=MAX_RANGE, occupied_voxels=int((occ != 0).sum()),
                           map="tools/fusion_bench.py batch_frames(16) fused three times into its empty map by fuse_depth_batch",
                           poses="the cameras of those frames: a 3 m circle at 1.61 m height; the LiDAR's x along the camera's heading, z up"),
               launches_per_call=2, beams=S * P, pixels=S * ROWS * COLS,
               scan_returns_device=returns["f64"], scan_returns_device_f32=returns["f32"], scan_returns_host=scan_returns_host,
               depth_returns_device=[int(v) for v in dstatus.cpu().numpy()[:, 1]],
               scan_lane_steps=scan_steps, depth_lane_steps=depth_steps,
               lane_steps_counted_on=f"the host: every beam; every {a.stride}-th pixel in both directions of the images, scaled",
               output_bytes=dict(scan_f64=S * P * 24 + S * 36, scan_f32=S * P * 12 + S * 36, depth=S * ROWS * COLS * 2),
               ms={k: stats(v) for k, v in ms.items()})
    for k, steps in (("scan_f64", scan_steps), ("scan_f32", scan_steps), ("depth", depth_steps)):
        res[k + "_lane_steps_per_second"] = steps / (res["ms"][k]["median"] * 1e-3)
    res["scan_f64_beams_per_second"] = S * P / (res["ms"]["scan_f64"]["median"] * 1e-3)
    res["depth_rays_per_second"] = S * ROWS * COLS / (res["ms"]["depth"]["median"] * 1e-3)
    res["scan_f64_over_depth_lane_step_rate"] = res["scan_f64_lane_steps_per_second"] / res["depth_lane_steps_per_second"]
    res["design_9b_render_depth_lane_steps_per_second"] = 3.7e11
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("ms", "config", "what")} | {"ms": {k: {q: v[q] for q in ("median", "p10", "p90")} for k, v in res["ms"].items()}}))


if __name__ == "__main__":
    main()
