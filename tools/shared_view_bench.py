"""The device-built shared view (include/frp_nmpc_occmap_view.h, solver.SharedView) -> profiles/shared_view_bench.json, on the
pillars world of tools/render_bench.py (workloads.astar_world(seed=0, kind="pillars"): 20 x 20 x 4 m at 0.1 m, 200 x 200 x 40 voxels).
Its pillars are solid: 100 737 occupied voxels, more than a shared cloud holds (FRP_CORRIDOR_MAX_POINTS = 65 536; shared_view() raises).
The map measured is the world's SURFACE -- the occupied voxels with a free face neighbour, 38 595 of them -- which is all a depth
sensor can ever put into a belief map:
  * rebuild: ms per SharedView.update() (device events around 50 x `reps` calls after a warm-up, `windows` windows, median and spread),
    the same replayed from a captured hipGraph, against OccupancyMap.shared_view() on the same map.  shared_view() is the code of
    the parent commit, unchanged by this one; it synchronises, so it is WALL time per call (perf_counter around `reps` calls, each
    ending in its own synchronisation), which is what a tick loop would pay;
  * corridor: ms per cut corridor for 4096 planners through view= (the count on the device, P = the capacity) against the same
    corridor through the trimmed cloud and grid of shared_view() (P = the count), alternating, two passes; and through a view whose
    capacity is chosen near the map's real count.  The two routes' outputs are compared (they must be equal to the bit).
Reported, not gated: no ratio was fixed in advance.
   python tools/shared_view_bench.py [--reps 20] [--windows 5] [--planners 4096] [--parent <commit>] [--out profiles/shared_view_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from forces_resilient_planner_amd import solver, workloads  # noqa: E402

DEV = "cuda:0"


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


def wall_ms(fn, reps, windows):
    """fn synchronises by itself: host clock around reps calls."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / reps)
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def planners(rng, B, N):
    """Stage references along tools/occmap_bench.py's curved 5 m path, started all over the pillar field at flight height."""
    s = np.linspace(0, 5, N)
    path = np.c_[s, 0.4 * np.sin(0.8 * s), 1.0 + 0.1 * np.cos(s)]
    start = np.c_[rng.uniform(-8.5, 3.0, B), rng.uniform(-8.0, 8.0, B), np.zeros(B)]
    ref = path[None] + start[:, None, :] + rng.normal(0, 0.03, (B, N, 3))
    yaw = np.arctan2(np.gradient(path[:, 1]), np.gradient(path[:, 0]))[None] + rng.normal(0, 0.05, (B, N))
    return ref, yaw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--planners", type=int, default=4096)
    ap.add_argument("--parent", default="unknown", help="the commit whose shared_view() this one is measured against (its code is unchanged here)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_view_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("shared_view_bench.py measures on the GPU: no device, nothing is reported")
    w = workloads.astar_world(seed=0, kind="pillars")
    solid = w["occ"] != 0
    p = np.pad(solid, 1, constant_values=True)                                   # (outside the map: no free neighbour)
    inner = p[2:, 1:-1, 1:-1] & p[:-2, 1:-1, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 1:-1, 2:] & p[1:-1, 1:-1, :-2]
    w = dict(w, occ=(solid & ~inner).astype(np.uint8))
    dm = solver.OccupancyMap(world=w)
    view = dm.shared_view_device()
    view.update(); torch.cuda.synchronize()
    n, total = int(view.count.item()), int(view.total.item())
    shared, grid = dm.shared_view()
    assert n == total == shared.shape[0] and torch.equal(view.cloud[:n], shared)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "parent_commit": a.parent,
           "timing": "device events around `reps` back-to-back calls after 3 warm-up calls, `windows` windows, median / min / max; "
                     "shared_view() synchronises and is wall time (perf_counter) around `reps` calls",
           "config": dict(world="workloads.astar_world(seed=0, kind='pillars'), surface voxels only", solid_voxels=int(solid.sum()), grid=[int(v) for v in dm.grid], resolution=dm.resolution,
                          plane_bytes=int(dm.ws_bytes), cell=view.cell, grid_dims=list(view.dims), cap=view.cap, points=n,
                          update_launches=solver.OCCMAP_VIEW_LAUNCHES)}
    # ---- the rebuild ----
    fast = a.reps * 50                                                           # (an update is tens of microseconds: windows of ~40 ms)
    rebuild = {"reps_update": fast, "update_ms": windows_ms(view.update, fast, a.windows)}
    rebuild["parent_shared_view_wall_ms"] = wall_ms(lambda: dm.shared_view(), a.reps * 5, a.windows)
    rebuild["update_ms_second_pass"] = windows_ms(view.update, fast, a.windows)
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        view.update()
    rebuild["update_ms_graph"] = windows_ms(g.replay, fast, a.windows)
    rebuild["shared_view_over_update"] = rebuild["parent_shared_view_wall_ms"]["median"] / rebuild["update_ms"]["median"]
    res["rebuild"] = rebuild
    print(json.dumps(rebuild), flush=True)
    # ---- the cut corridor ----
    B, N, F = a.planners, 20, 64
    rng = np.random.default_rng(0)
    ref, yaw = planners(rng, B, N)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(DEV)
    z = np.zeros((B, N, 17)); z[..., 3] = 7.3; z[..., 8:11] = ref; z[..., 16] = yaw
    mo = torch.zeros((B, N + 1, 17), dtype=torch.float64, device=DEV); mo[:, :N] = up(z)
    E = torch.empty((B, N, 3, 3), dtype=torch.float64, device=DEV)
    solver.tube_batch_device(mo, E)
    d_ref, d_yaw = up(ref), up(yaw)
    outs = [(torch.zeros((B, N, F, 3), dtype=torch.float64, device=DEV), torch.zeros((B, N, F), dtype=torch.float64, device=DEV),
             torch.zeros((B, N), dtype=torch.int32, device=DEV), torch.zeros((B, N), dtype=torch.int32, device=DEV),
             torch.zeros((B,), dtype=torch.int32, device=DEV)) for _ in range(3)]
    boxes = dm.local_view(up(ref[:, 0]), 0)
    cut = dm.cut(boxes.local_box)
    tight = dm.shared_view_device(cap=min(solver.CORRIDOR_MAX_POINTS, n + n // 16 + 1))
    tight.update()
    routes = {"shared_view_trimmed": lambda: solver.corridor_batch_device(shared, d_ref, d_yaw, E, *outs[0], grid=grid, cut=cut),
              "view": lambda: solver.corridor_batch_device(None, d_ref, d_yaw, E, *outs[1], view=view, cut=cut),
              "view_tight_capacity": lambda: solver.corridor_batch_device(None, d_ref, d_yaw, E, *outs[2], view=tight, cut=cut)}
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    equal = all(torch.equal(x, y) and torch.equal(x, t) for x, y, t in zip(*outs))
    cor = {"B": B, "N": N, "F": F, "P": {"shared_view_trimmed": n, "view": view.cap, "view_tight_capacity": tight.cap}, "outputs_equal": bool(equal),
           "passes": []}
    for _ in range(2):                                                           # alternating: no route owns a warmer device
        cor["passes"].append({k: windows_ms(fn, a.reps, a.windows) for k, fn in routes.items()})
    med = {k: float(np.median([p[k]["median"] for p in cor["passes"]])) for k in routes}
    cor["corridor_ms"] = med
    cor["view_over_trimmed"] = med["view"] / med["shared_view_trimmed"]
    cor["tight_view_over_trimmed"] = med["view_tight_capacity"] / med["shared_view_trimmed"]
    res["corridor"] = cor
    # what a tick that rebuilds the shared cloud pays on either route
    res["rebuild_plus_corridor_ms"] = {"shared_view_trimmed": rebuild["parent_shared_view_wall_ms"]["median"] + med["shared_view_trimmed"],
                                       "view": rebuild["update_ms"]["median"] + med["view"],
                                       "view_tight_capacity": rebuild["update_ms"]["median"] + med["view_tight_capacity"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("corridor", "rebuild_plus_corridor_ms")}))
    if not equal:
        raise SystemExit("the routes' corridors differ")


if __name__ == "__main__":
    main()
