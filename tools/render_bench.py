"""The depth renderer (include/frp_nmpc_occmap_render.h, solver.OccupancyMap.render_depth) at the size a fleet would run it ->
profiles/render_depth.json: F = 16 frames of 480 x 640 through the 20 x 20 x 4 m pillars world of workloads.astar_world at 0.1 m
(200 x 200 x 40 voxels), max_range 6 m, cameras at 1 m height on both sides of the pillar field looking into it.
Reported:
  * ms per render call (16 frames): device events around `reps` calls after a warm-up, `windows` windows, median and spread; the same
    replayed from a captured hipGraph;
  * ray steps per second: the cells the rays enter (counted on the host by a vectorised form of tests/occmap_render_oracle.py's walk over
    every `--stride`-th pixel in both directions, scaled up -- an estimate when stride > 1) over the median time;
  * for comparison, in the same process on the same frames: ms per solver.OccupancyMap.fuse_depth_batch call that fuses those 16 rendered
    images into an empty map of the same geometry at the launch file's parameters (default round cap, and the cap at the rounds used).
Reported, not gated: no render time was measured before.
   python tools/render_bench.py [--reps 20] [--windows 5] [--stride 4] [--out profiles/render_depth.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from forces_resilient_planner_amd import solver, workloads  # noqa: E402
from tests import occmap_fusion_oracle as FO  # noqa: E402
from tests import occmap_render_oracle as RO  # noqa: E402

F, ROWS, COLS = 16, 480, 640
K = np.array([[386.0, 0.0, 319.5], [0.0, 386.0, 239.5], [0.0, 0.0, 1.0]])   # tools/fusion_bench.py's camera: 79 degrees across
MAX_RANGE = 6.0


def poses():
    """Eight cameras at x = -5.5 looking along +x and eight at x = +5.5 looking along -x (the pillars stand in |x| < 4.5 + 0.6),
    y from -6 to 6, each turned a little differently."""
    out = []
    for k in range(F):
        side, j = k % 2, k // 2
        y = -6.0 + 12.0 * j / (F // 2 - 1)
        out.append(FO.pose((5.5 if side else -5.5, y, 1.0), yaw=(np.pi if side else 0.0) + 0.08 * (j - 3.5), pitch=-0.05))
    return np.ascontiguousarray(np.stack(out))


def count_steps(occ, origin, res, T, stride):
    """Cells entered by the rays of one frame, every stride-th pixel: the walk of RenderOracle.pixel, all rays at once."""
    u, v = np.meshgrid(np.arange(0, COLS, stride, dtype=np.float64), np.arange(0, ROWS, stride, dtype=np.float64))
    dcx, dcy = ((u - K[0, 2]) / K[0, 0]).ravel(), ((v - K[1, 2]) / K[1, 1]).ravel()
    R, t = T[:3, :3], T[:3, 3]
    d = np.stack([(R[i, 0] * dcx + R[i, 1] * dcy) + R[i, 2] for i in range(3)], 1)
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
    steps = 0
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
        live &= ~occupied(c)
    return steps


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--stride", type=int, default=4, help="the host's step count looks at every stride-th pixel in both directions")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_depth.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("render_bench.py measures on the GPU: no device, nothing is reported")
    w = workloads.astar_world(seed=0, kind="pillars")
    T = poses()
    for k in range(F):   # a camera inside a pillar would render nothing
        i = np.floor((T[k, :3, 3] - np.array(w["origin"])) / w["resolution"]).astype(int)
        assert w["occ"][i[0], i[1], i[2]] == 0, k
    steps = sum(count_steps(w["occ"], w["origin"], w["resolution"], T[k], a.stride) for k in range(F)) * a.stride * a.stride
    world = solver.OccupancyMap(world=w, **FO.LAUNCH_CLAMPS)
    belief = solver.OccupancyMap(origin=w["origin"], map_size=w["map_size"], resolution=w["resolution"], **FO.LAUNCH_CLAMPS)
    Td = torch.from_numpy(T).to(world.device)
    depth = torch.zeros((F, ROWS, COLS), dtype=torch.int16, device=world.device).view(torch.uint16)
    rstatus = torch.zeros((F, 2), dtype=torch.int32, device=world.device)
    fstatus = torch.zeros((F, 2), dtype=torch.int32, device=world.device)

    def render(**kw):
        world.render_depth(Td, K, ROWS, COLS, max_range=MAX_RANGE, out=depth, status=rstatus, **kw)

    def fuse(**kw):
        belief.fuse_depth_batch(depth, K, Td, status=fstatus, **kw)

    render(); fuse()
    torch.cuda.synchronize()
    returns = [int(v) for v in rstatus.cpu().numpy()[:, 1]]
    rounds = [int(v) for v in fstatus.cpu().numpy()[:, 0]]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows,
           "timing": "device events around `reps` back-to-back calls after 3 warm-up calls, `windows` windows; ms per call = per 16 frames",
           "config": dict(frames=F, image=[ROWS, COLS], grid=[int(v) for v in w["occ"].shape], resolution=w["resolution"], max_range=MAX_RANGE,
                          K=K.tolist(), world="workloads.astar_world(seed=0, kind='pillars')", fuse=FO.FUSE_DEFAULTS, clamps=FO.LAUNCH_CLAMPS),
           "rays": F * ROWS * COLS, "returns": returns, "ray_steps": steps, "ray_steps_counted_on": f"every {a.stride}-th pixel in both directions, scaled",
           "render_launches": 2, "fuse_rounds": rounds, "fuse_launches_default_cap": 2 * solver.OCCMAP_FUSE_DEFAULT_ROUNDS + 7}
    res["render_ms"] = windows_ms(render, a.reps, a.windows)
    res["fuse_batch_ms_default_cap"] = windows_ms(fuse, a.reps, a.windows)
    top = max(rounds)
    if top > 0:
        res["fuse_batch_ms_cap_at_largest_rounds"] = windows_ms(lambda: fuse(max_rounds=top), a.reps, a.windows)
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(g, stream=side):
        render(stream=torch.cuda.current_stream())
    res["render_ms_graph"] = windows_ms(g.replay, a.reps, a.windows)
    res["ray_steps_per_second"] = steps / (res["render_ms"]["median"] * 1e-3)
    res["rays_per_second"] = F * ROWS * COLS / (res["render_ms"]["median"] * 1e-3)
    res["render_over_fuse_default_cap"] = res["render_ms"]["median"] / res["fuse_batch_ms_default_cap"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("render_ms", "render_ms_graph", "fuse_batch_ms_default_cap", "ray_steps", "ray_steps_per_second",
                                          "render_over_fuse_default_cap", "fuse_rounds")}))


if __name__ == "__main__":
    main()
