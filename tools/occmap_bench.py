"""Timings of the occupancy map on the device (include/frp_nmpc.h (8), solver.OccupancyMap) -> profiles/occmap_bench.json:
  * insert of a cloud, ms per call;
  * the local view at B = 1 / 1024 / 4096, on the pillar world (20 x 20 x 4 m) and on a map of the reference's size
    (40 x 40 x 5 m at 0.1 m, local radius 6 / 6 / 3 m), with the bytes it must touch (bit-plane words in range + points written)
    and the bytes/s that implies;
  * the corridor step fed from per-planner clouds of the local view against the shared whole-map cloud + uniform grid
    (the route of tools/full_tick_bench.py) and against the same shared cloud + grid CUT to each planner's local box
    (frp_nmpc_corridor_batch_cut: box-only view + corridor), same planners, same session, with the bytes each route allocates;
  * `safety`: one tick of the safety timer (OccupancyMap.safety_check: goal test + search, path walk) for 4096 planners with
    200-sample paths, stride 5, on the reference-sized map with 25 pillars, against the only other device route: the same probes
    (243 per checked position) generated on the device with torch and pushed through frp_nmpc_occmap_query, then reduced.  The
    query route has no goal SEARCH (its candidates depend on one another); safety_check's time includes it.
Reported, not gated.   python tools/occmap_bench.py [reps=20] [safety]   (`safety`: that leg alone, merged into the existing file)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from forces_resilient_planner_amd import solver, workloads  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
DEV = "cuda:0"


def timed(fn, reps=REPS):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def pillar_cloud(rng, n_pillars, lo, hi, top):
    """Points on a 0.05 m lattice inside random vertical boxes: every voxel of a box is hit."""
    out = []
    for _ in range(n_pillars):
        cx, cy = rng.uniform(lo[0], hi[0]), rng.uniform(lo[1], hi[1])
        hx, hy = rng.uniform(0.15, 0.6, 2)
        g = np.mgrid[cx - hx:cx + hx:0.05, cy - hy:cy + hy:0.05, 0.0:top:0.05].reshape(3, -1).T
        out.append(g)
    return np.concatenate(out).astype(np.float32)


def view_bench(dm, centres, P):
    B = len(centres)
    c = torch.from_numpy(np.ascontiguousarray(centres)).to(DEV)
    view = dm.local_view(c, P)
    torch.cuda.synchronize()
    n = view.cloud_count.cpu().numpy()
    box = view.local_box.cpu().numpy().astype(np.int64)
    ext = np.maximum(box[:, 3:] - box[:, :3], 0)
    wz_in_range = np.where(ext[:, 2] > 0, (box[:, 5] - 1) // 32 - box[:, 2] // 32 + 1, 0)
    plane_bytes = int((ext[:, 0] * ext[:, 1] * wz_in_range * 4).sum())
    point_bytes = int(np.minimum(np.abs(n), P).sum()) * 24
    ms = timed(lambda: dm.local_view(c, P, out=view))
    return dict(B=B, P=P, ms=ms, overflowed=int((n < 0).sum()), points_mean=float(np.abs(n).mean()), points_max=int(np.abs(n).max()),
                plane_bytes=plane_bytes, point_bytes=point_bytes, GBps=(plane_bytes + point_bytes) / ms / 1e6), view


def safety_bench(dm, rng, B=4096, K=200, stride=5):
    """ms of safety_check and of the query route on the same planners; the two routes' goal_blocked and first_hit must agree."""
    ratio, (ego_r, ego_h) = solver.SAFETY_INFLATE_CHECK, solver.OCCMAP_BODY
    start = np.c_[rng.uniform(-17, 17, B), rng.uniform(-17, 17, B), rng.uniform(0.8, 1.6, B)]
    ang = rng.uniform(-np.pi, np.pi, B)
    step = 0.05 * np.arange(K)                                                  # samples 0.05 m apart: 10 m of path
    path = start[:, None, :] + np.stack([np.cos(ang)[:, None] * step, np.sin(ang)[:, None] * step, np.zeros((B, K))], -1)
    path[..., :2] = np.clip(path[..., :2], -19.0, 19.0)
    kp = torch.from_numpy(np.ascontiguousarray(path)).to(DEV)
    sz = torch.full((B,), K, dtype=torch.int32, device=DEV)
    end0 = kp[:, -1, :].clone()
    end = end0.clone()
    out = dm.safety_check(end, kp, sz, stride=stride)
    torch.cuda.synchronize()

    def run_check():
        end.copy_(end0)                                                         # (a moved goal would make the next repetition another problem)
        dm.safety_check(end, kp, sz, stride=stride, out=out)

    h = [int(np.ceil(e * ratio / dm.resolution)) for e in (ego_r, ego_r, ego_h)]
    off = torch.tensor([[i, j, k] for i in range(-h[0], h[0] + 1) for j in range(-h[1], h[1] + 1) for k in range(-h[2], h[2] + 1)],
                       dtype=torch.float64, device=DEV) * dm.resolution         # Vector3d(i, j, k) * resolution_
    S = len(range(0, K, stride))
    state = {}

    def run_query():
        pos = torch.cat([end0[:, None, :], kp[:, ::stride, :]], 1)              # [B, 1 + S, 3]: the goal, then the checked samples
        probes = (pos[:, :, None, :] + off[None, None, :, :]).reshape(-1, 3)    # pos + offset, one rounding: the reference's probes
        st = dm.query(probes)
        hit = (st != 0).view(B, 1 + S, -1).any(-1)
        idx = torch.where(hit[:, 1:].any(1), hit[:, 1:].int().argmax(1) * stride, torch.full((B,), -1, device=DEV))
        state["blocked"], state["first_hit"] = hit[:, 0].int(), idx.int()

    ms_check = timed(run_check)
    ms_query = timed(run_query, max(3, REPS // 4))
    ms_check2 = timed(run_check)
    run_check(); run_query(); torch.cuda.synchronize()
    agree = bool(torch.equal(out.goal_blocked, state["blocked"]) and torch.equal(out.first_hit, state["first_hit"]))
    return dict(B=B, K=K, stride=stride, probes_per_position=int(off.shape[0]), positions=B * (1 + S), map="40x40x5", pillars=25,
                safety_check_ms=ms_check, safety_check_ms_second_pass=ms_check2, query_route_ms=ms_query, query_route_over_safety_check=ms_query / ms_check,
                query_route_note="goal test + path walk only, no goal search; includes generating the probes and reducing the states with torch",
                goal_blocked=int(out.goal_blocked.sum()), goals_moved=int((out.goal_hits > 0).sum()), paths_hit=int((out.first_hit >= 0).sum()),
                routes_agree=agree)


def safety_only():
    rng = np.random.default_rng(0)
    ref_map = solver.OccupancyMap(origin=(-20.0, -20.0, 0.0), map_size=(40.0, 40.0, 5.0), resolution=0.1)
    ref_map.insert_cloud(torch.from_numpy(pillar_cloud(rng, 25, (-18, -18), (18, 18), 3.0)).to(DEV))
    r = safety_bench(ref_map, rng)
    r["device"] = torch.cuda.get_device_name(0); r["reps"] = REPS
    path = os.path.join(ROOT, "profiles", "occmap_bench.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    res["safety"] = r
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(r))


def main():
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "local_view": {}, "insert": {}}
    worlds = {}
    w = workloads.astar_world(2, "pillars", n_obstacles=12)
    worlds["pillars_20x20x4"] = (solver.OccupancyMap(w), None)
    ref_map = solver.OccupancyMap(origin=(-20.0, -20.0, 0.0), map_size=(40.0, 40.0, 5.0), resolution=0.1)
    cloud = pillar_cloud(rng, 25, (-18, -18), (18, 18), 3.0)
    d_cloud = torch.from_numpy(cloud).to(DEV)
    res["insert"] = dict(points=len(cloud), ms=timed(lambda: ref_map.insert_cloud(d_cloud)), map="40x40x5")
    res["reset_ms"] = timed(lambda: (ref_map.reset(), ref_map.insert_cloud(d_cloud))) - res["insert"]["ms"]
    res["refresh_ms"] = timed(ref_map.refresh)
    worlds["reference_40x40x5"] = (ref_map, None)
    for name, (dm, _) in worlds.items():
        lo = np.array(dm.origin) + 1.0; hi = np.array(dm.origin) + np.array(dm.map_size) - 1.0
        occupied = int(dm.occ.sum())
        res["local_view"][name] = {"grid": dm.grid, "occupied_voxels": occupied, "runs": []}
        for B in (1, 1024, 4096):
            c = rng.uniform(lo, hi, (B, 3)); c[:, 2] = rng.uniform(0.5, 2.0, B)
            probe = dm.local_view(c, 0); torch.cuda.synchronize()
            P = int(min(solver.CORRIDOR_MAX_POINTS, max(1, -int(probe.cloud_count.min()))))
            r, _ = view_bench(dm, c, P)
            res["local_view"][name]["runs"].append(r)
            print(name, r, flush=True)
    # corridor: per-planner clouds (local cut, as the reference) vs the shared whole-map cloud + grid
    B, N, F = 4096, 20, 64
    dm = worlds["reference_40x40x5"][0]
    s = np.linspace(0, 5, N)
    path = np.c_[s, 0.4 * np.sin(0.8 * s), 1.0 + 0.1 * np.cos(s)]
    start = np.c_[rng.uniform(-15, 10, B), rng.uniform(-15, 15, B), np.zeros(B)]
    ref = path[None] + start[:, None, :] + rng.normal(0, 0.03, (B, N, 3))
    yaw = np.arctan2(np.gradient(path[:, 1]), np.gradient(path[:, 0]))[None] + rng.normal(0, 0.05, (B, N))
    z = np.zeros((B, N, 17)); z[..., 3] = 7.3; z[..., 8:11] = ref; z[..., 16] = yaw
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)
    mo = torch.zeros((B, N + 1, 17), dtype=torch.float64, device=DEV); mo[:, :N] = up(z)
    E = torch.empty((B, N, 3, 3), dtype=torch.float64, device=DEV)
    solver.tube_batch_device(mo, E)
    d_ref, d_yaw = up(ref), up(yaw)
    out = (torch.zeros((B, N, F, 3), dtype=torch.float64, device=DEV), torch.zeros((B, N, F), dtype=torch.float64, device=DEV),
           torch.zeros((B, N), dtype=torch.int32, device=DEV), torch.zeros((B, N), dtype=torch.int32, device=DEV), torch.zeros((B,), dtype=torch.int32, device=DEV))
    probe = dm.local_view(ref[:, 0], 0); torch.cuda.synchronize()
    P = int(min(solver.CORRIDOR_MAX_POINTS, max(1, -int(probe.cloud_count.min()))))
    rv, view = view_bench(dm, ref[:, 0], P)
    ms_local = timed(lambda: solver.corridor_batch_device(view.cloud, d_ref, d_yaw, E, *out, cloud_count=view.cloud_count), max(3, REPS // 4))
    whole = dm.local_view(None, solver.CORRIDOR_MAX_POINTS); torch.cuda.synchronize()
    nw = int(whole.cloud_count[0])
    cor = {"B": B, "per_planner": {"P": P, "local_view_ms": rv["ms"], "corridor_ms": ms_local,
                                   "bytes": view.cloud.numel() * 8 + view.cloud_count.numel() * 4 + view.local_box.numel() * 4}}
    if nw > 0:
        shared = whole.cloud[0, :nw].contiguous()
        grid = solver.CloudGrid(shared, 0.5, dm.origin, tuple(int(np.ceil(m / 0.5)) for m in dm.map_size))
        ms_grid = timed(lambda: solver.corridor_batch_device(shared, d_ref, d_yaw, E, *out, grid=grid))
        grid_bytes = shared.numel() * 8 + grid.points.numel() * 8 + grid.index.numel() * 4 + grid.start.numel() * 4
        cor["shared_cloud_grid"] = {"points": nw, "corridor_ms": ms_grid, "bytes": grid_bytes,
                                    "note": "no local cut: planners see points the reference hides, other polytopes"}
        cor["per_planner_over_shared"] = ms_local / ms_grid
        # the cut route: per tick the box-only view, then the corridor on the shared cloud + grid cut to each planner's box (same
        # polytopes as per_planner, to the bit); the three corridor timings alternate once more so that none owns a warmer device
        c0 = up(ref[:, 0])
        boxes = dm.local_view(c0, 0)
        ms_boxes = timed(lambda: dm.local_view(c0, 0, out=boxes))
        cut = dm.cut(boxes.local_box)
        run_cut = lambda: solver.corridor_batch_device(shared, d_ref, d_yaw, E, *out, grid=grid, cut=cut)
        ms_cut = timed(run_cut)
        again = {"per_planner": timed(lambda: solver.corridor_batch_device(view.cloud, d_ref, d_yaw, E, *out, cloud_count=view.cloud_count), max(3, REPS // 4)),
                 "shared_cloud_grid": timed(lambda: solver.corridor_batch_device(shared, d_ref, d_yaw, E, *out, grid=grid)),
                 "shared_cut": timed(run_cut)}
        cor["shared_cut"] = {"points": nw, "local_view_ms": ms_boxes, "corridor_ms": ms_cut, "bytes": grid_bytes + boxes.local_box.numel() * 4 + boxes.cloud_count.numel() * 4}
        cor["second_pass_corridor_ms"] = again
        tick = {"per_planner": rv["ms"] + ms_local, "shared_cut": ms_boxes + ms_cut}
        cor["view_plus_corridor_ms"] = tick
        cor["reference_equivalent_winner"] = min(tick, key=tick.get)
    else:
        cor["shared_cloud_grid"] = {"skipped": f"the whole map holds {-nw} occupied voxels, more than FRP_CORRIDOR_MAX_POINTS"}
    res["corridor"] = cor
    res["safety"] = safety_bench(dm, rng)
    print(json.dumps(res["safety"]))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "occmap_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["corridor"]))


if __name__ == "__main__":
    if "safety" in sys.argv[2:]:
        safety_only()
    else:
        main()
