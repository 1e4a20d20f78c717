"""The shared-cloud route beyond FRP_CORRIDOR_MAX_POINTS (include/frp_nmpc_corridor_large.h, a SharedView with cap > 65 536) ->
profiles/corridor_large_bench.json, on the pillars world of tools/shared_view_bench.py (200 x 200 x 40 voxels of 0.1 m), 4096 planners:
  (a) the SOLID world, 100 737 occupied voxels -- a map the shared route could not take before.  Per tick: SharedView.update() + the cut
      corridor through the large view, against ROUTE 1 on the same commit (code this change does not touch): OccupancyMap.local_view(
      centres, P) into per-planner clouds + frp_nmpc_corridor_batch on them, P = the largest local view, at a local radius of
      4 / 4 / 3 m (at the default 6 / 6 / 3 m the largest local view holds more than the 65 536 points route 1 stores).  The bytes each route
      allocates for the clouds are recorded, and the two routes' outputs are compared (they must be equal to the bit);
  (b) the world's SURFACE (38 595 voxels), which both entries can take: frp_nmpc_corridor_batch_large against frp_nmpc_corridor_batch_view
      on the same view buffers at equal capacity (65 536), alternating.
Device events around `reps` back-to-back calls after 3 warm-up calls, `windows` windows, median / min / max (tools/shared_view_bench.py).
Reported, not gated: no ratio was fixed in advance.
   python tools/corridor_large_bench.py [--reps 10] [--windows 5] [--planners 4096] [--out profiles/corridor_large_bench.json]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from forces_resilient_planner_amd import solver, workloads  # noqa: E402
from shared_view_bench import planners, windows_ms  # noqa: E402

DEV = "cuda:0"


def outputs(B, N, F):
    import torch
    return (torch.zeros((B, N, F, 3), dtype=torch.float64, device=DEV), torch.zeros((B, N, F), dtype=torch.float64, device=DEV),
            torch.zeros((B, N), dtype=torch.int32, device=DEV), torch.zeros((B, N), dtype=torch.int32, device=DEV),
            torch.zeros((B,), dtype=torch.int32, device=DEV))


def large_call(view, d_ref, d_yaw, E, out, cut, B, N, F):
    """frp_nmpc_corridor_batch_large on the buffers of a view of ANY capacity (the wrappers route by capacity)."""
    import torch
    c, g = solver.CORRIDOR_DEFAULTS, view.grid
    cr = solver.Corridor(B, N, F, view.cap, view.cloud.data_ptr(), 0, view.count.data_ptr(), d_ref.data_ptr(), d_yaw.data_ptr(), E.data_ptr(),
                         (ctypes.c_double * 3)(*c["bbox"]), c["seed_len"], c["inflation"], c["offset_x"], out[0].data_ptr(), out[1].data_ptr(),
                         out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr())
    cr.grid_origin = (ctypes.c_double * 3)(*g.origin); cr.grid_cell = g.cell; cr.grid_dims = (ctypes.c_int * 3)(*g.dims)
    cr.grid_points = g.points.data_ptr(); cr.grid_index = g.index.data_ptr(); cr.grid_start = g.start.data_ptr()
    ws = torch.zeros((solver.lib().frp_nmpc_corridor_large_workspace_bytes(B),), dtype=torch.uint8, device=DEV)
    ov = torch.zeros((B,), dtype=torch.int32, device=DEV)
    w = solver.CorridorLarge(ws.data_ptr(), ws.numel(), ov.data_ptr())
    keep = (cr, w, ws, ov)

    def fn():
        rc = solver.lib().frp_nmpc_corridor_batch_large(ctypes.byref(keep[0]), ctypes.byref(cut), ctypes.byref(keep[1]),
                                                        ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        assert rc == 0, rc
    return fn, ov


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--planners", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corridor_large_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("corridor_large_bench.py measures on the GPU: no device, nothing is reported")
    B, N, F = a.planners, 20, 64
    w = workloads.astar_world(seed=0, kind="pillars")
    solid = w["occ"] != 0
    p = np.pad(solid, 1, constant_values=True)
    inner = p[2:, 1:-1, 1:-1] & p[:-2, 1:-1, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 1:-1, 2:] & p[1:-1, 1:-1, :-2]
    rng = np.random.default_rng(0)
    ref, yaw = planners(rng, B, N)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(DEV)
    z = np.zeros((B, N, 17)); z[..., 3] = 7.3; z[..., 8:11] = ref; z[..., 16] = yaw
    mo = torch.zeros((B, N + 1, 17), dtype=torch.float64, device=DEV); mo[:, :N] = up(z)
    E = torch.empty((B, N, 3, 3), dtype=torch.float64, device=DEV)
    solver.tube_batch_device(mo, E)
    d_ref, d_yaw, d_c = up(ref), up(yaw), up(ref[:, 0])
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "B": B, "N": N, "F": F,
           "timing": "device events around `reps` back-to-back calls after 3 warm-up calls, `windows` windows, median / min / max"}

    # ---- (a) the solid world: the large view against route 1 ----
    # (at the default local radius 6 / 6 / 3 m the largest local view of this world holds 86 929 points: more than ROUTE 1 stores per
    # planner, so the comparison is made at 4 / 4 / 3 m, which still covers the corridor's 2 / 2 / 1 m box around a stage reference)
    radius = (4.0, 4.0, 3.0)
    dm = solver.OccupancyMap(world=dict(w, occ=solid.astype(np.uint8)), local_radius=radius)
    view = dm.shared_view_device(cap=131072, planners=B)
    view.update(); torch.cuda.synchronize()
    n = int(view.count.item())
    boxes = dm.local_view(d_c, 0)
    cut = dm.cut(boxes.local_box)
    probe = dm.local_view(d_c, 1)                                                # a count that does not fit comes back negated
    P1 = int(probe.cloud_count.abs().max().item())
    assert P1 <= solver.CORRIDOR_MAX_POINTS, P1
    lv = dm.local_view(d_c, P1)
    o_large, o_r1 = outputs(B, N, F), outputs(B, N, F)

    def tick_large():
        view.update()
        solver.corridor_batch_device(None, d_ref, d_yaw, E, *o_large, view=view, cut=cut)

    def tick_route1():
        dm.local_view(d_c, P1, out=lv)
        solver.corridor_batch_device(lv.cloud, d_ref, d_yaw, E, *o_r1, cloud_count=lv.cloud_count)

    tick_large(); tick_route1(); torch.cuda.synchronize()
    equal_a = all(torch.equal(x, y) for x, y in zip(o_large, o_r1))
    case_a = {"world": "workloads.astar_world(seed=0, kind='pillars'), solid", "local_radius": list(radius), "points": n, "view_cap": view.cap, "route1_P": P1,
              "outputs_equal": bool(equal_a), "planners_refused": int(view.overflow[:B].sum().item()),
              "cloud_bytes": {"large_view": int(view.cloud.numel() * 8 + view.grid.points.numel() * 8 + view.grid.index.numel() * 4 +
                                                view.grid.start.numel() * 4 * 2 + view._workspace.numel()),
                              "route1": int(lv.cloud.numel() * 8)},
              "passes": []}
    parts = {"large_update": view.update,
             "large_corridor": lambda: solver.corridor_batch_device(None, d_ref, d_yaw, E, *o_large, view=view, cut=cut),
             "route1_local_view": lambda: dm.local_view(d_c, P1, out=lv),
             "route1_corridor": lambda: solver.corridor_batch_device(lv.cloud, d_ref, d_yaw, E, *o_r1, cloud_count=lv.cloud_count),
             "large_tick": tick_large, "route1_tick": tick_route1}
    for _ in range(2):                                                           # alternating: no route owns a warmer device
        case_a["passes"].append({k: windows_ms(fn, a.reps, a.windows) for k, fn in parts.items()})
    case_a["ms"] = {k: float(np.median([q[k]["median"] for q in case_a["passes"]])) for k in parts}
    case_a["route1_over_large_tick"] = case_a["ms"]["route1_tick"] / case_a["ms"]["large_tick"]
    res["solid_world"] = case_a
    print(json.dumps({k: case_a[k] for k in ("points", "route1_P", "outputs_equal", "planners_refused", "cloud_bytes", "ms")}), flush=True)
    del lv, probe

    # ---- (b) the surface map: _large against _view at equal capacity ----
    ds = solver.OccupancyMap(world=dict(w, occ=(solid & ~inner).astype(np.uint8)))                # (the default radius, as tools/shared_view_bench.py)
    sv = ds.shared_view_device()
    sv.update(); torch.cuda.synchronize()
    cut_s = ds.cut(ds.local_view(d_c, 0).local_box)
    o_view, o_lg = outputs(B, N, F), outputs(B, N, F)
    f_view = lambda: solver.corridor_batch_device(None, d_ref, d_yaw, E, *o_view, view=sv, cut=cut_s)
    f_large, ov = large_call(sv, d_ref, d_yaw, E, o_lg, cut_s, B, N, F)
    f_view(); f_large(); torch.cuda.synchronize()
    equal_b = all(torch.equal(x, y) for x, y in zip(o_view, o_lg))
    case_b = {"world": "the same world's surface voxels", "points": int(sv.count.item()), "cap": sv.cap, "outputs_equal": bool(equal_b),
              "planners_refused": int(ov.sum().item()), "passes": []}
    for _ in range(2):
        case_b["passes"].append({"view": windows_ms(f_view, a.reps, a.windows), "large": windows_ms(f_large, a.reps, a.windows)})
    case_b["ms"] = {k: float(np.median([q[k]["median"] for q in case_b["passes"]])) for k in ("view", "large")}
    case_b["large_over_view"] = case_b["ms"]["large"] / case_b["ms"]["view"]
    res["surface_map"] = case_b
    print(json.dumps({k: case_b[k] for k in ("points", "outputs_equal", "planners_refused", "ms", "large_over_view")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if not (equal_a and equal_b):
        raise SystemExit("the routes' corridors differ")


if __name__ == "__main__":
    main()
