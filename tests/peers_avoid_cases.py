"""Cases of peer avoidance shared by tests/test_peers_avoid_cpu.py (no device) and tests/test_gpu_peers_avoid.py: the overlay searches --
a world, B = 4 queries, every planner's boxes and, for one case, local boxes -- each named after the lookup route of csrc/frp_astar.hip
it is there for, and the scenes of the box kernel (tests/peers_cases.cloud_scene on the 40 x 40 x 20 map).  Worlds and queries come from
forces_resilient_planner_amd.workloads; the route conditions are tests/astar_path_cases.py's, read and not changed."""
import numpy as np

from forces_resilient_planner_amd import workloads

from . import astar_path_cases as AC

B, Q = 4, 4
POOL = 12000
HALF = (0.3, 0.3, 0.4)                  # a peer's box in the box-kernel scenes, metres
OVERLAY = ("empty", "pillars", "wall_gap", "window_edge", "beyond_window", "local_box", "byte_map")


def voxel(w, p):
    return [int(np.floor((p[k] - w["origin"][k]) / w["resolution"])) for k in range(3)]


def box_at(w, centre, half_cells):
    """min_id, max_id of the box of half_cells voxels around the voxel of `centre`, clipped to the map."""
    c, g = voxel(w, centre), w["occ"].shape
    return [max(c[k] - half_cells[k], 0) for k in range(3)] + [min(c[k] + half_cells[k], g[k] - 1) for k in range(3)]


def _on_line(w, q, fractions=((0.5,), (), (0.35, 0.6, 0.8), (0.45, 0.7)), half_cells=(3, 3, 4)):
    """Planner b: boxes on its straight start-goal line at fractions[b] (planner 1: none, next to planners that have some)."""
    bx, cnt = np.zeros((B, Q, 6), dtype=np.int32), np.zeros((B,), dtype=np.int32)
    for b in range(B):
        for j, f in enumerate(fractions[b]):
            bx[b, j] = box_at(w, q["start_pt"][b] + f * (q["end_pt"][b] - q["start_pt"][b]), half_cells)
        cnt[b] = len(fractions[b])
    return bx, cnt


def _ahead(w, q, first, last, half_cells=(0, 6, 6)):
    """Planner b: one box `first` ... `last` columns ahead of its start voxel in x (planner 1: none)."""
    bx, cnt = np.zeros((B, Q, 6), dtype=np.int32), np.zeros((B,), dtype=np.int32)
    g = w["occ"].shape
    for b in (0, 2, 3):
        c = voxel(w, q["start_pt"][b])
        bx[b, 0] = [min(c[0] + first, g[0] - 1), max(c[1] - half_cells[1], 0), max(c[2] - half_cells[2], 0),
                    min(c[0] + last, g[0] - 1), min(c[1] + half_cells[1], g[1] - 1), min(c[2] + half_cells[2], g[2] - 1)]
        cnt[b] = 1
    return bx, cnt


def overlay_case(name):
    """dict(world, q, boxes [B,Q,6], count [B], local_box [B,6] or None)."""
    i = OVERLAY.index(name)
    local = None
    if name in ("empty", "pillars", "wall_gap"):
        w = workloads.astar_world(500 + i, name, allocate_num=POOL, n_obstacles=30)
        q = workloads.astar_queries(B, 500 + i)
        bx, cnt = _on_line(w, q)
    elif name in ("window_edge", "beyond_window"):
        # max_tau = 1.0: a primitive of a node at the velocity bound reaches 35 columns and the window's radius is clamped to WIN_R_MAX = 31,
        # so its samples leave the window (the packed map's own word); the box straddles the edge of the start node's window, or lies
        # wholly beyond it and inside such a primitive's reach
        w = workloads.astar_world(500 + i, "pillars", allocate_num=POOL, n_obstacles=30, max_tau=1.0)
        q = workloads.astar_queries(B, 500 + i)
        q["start_v"][:, 0] = 1.5; q["start_v"][:, 1:] = 0.0; q["f_ext"][:] = 0.0
        bx, cnt = _ahead(w, q, AC.WIN_R_MAX - 2, AC.WIN_R_MAX + 2) if name == "window_edge" else _ahead(w, q, AC.WIN_R_MAX + 1, AC.WIN_R_MAX + 3)
    elif name == "local_box":
        # every planner's local box ends at the y index of its own line: the half of a box at larger y reads free
        w = workloads.astar_world(500 + i, "empty", allocate_num=POOL)
        q = workloads.astar_queries(B, 500 + i)
        q["end_pt"][:, 1] = q["start_pt"][:, 1]
        bx, cnt = _on_line(w, q, half_cells=(2, 5, 5))
        g = w["occ"].shape
        local = np.array([[0, 0, 0, g[0] - 1, voxel(w, q["start_pt"][b])[1], g[2] - 1] for b in range(B)], dtype=np.int32)
    elif name == "byte_map":
        w = workloads.astar_world(500 + i, "pillars", allocate_num=POOL, n_obstacles=30, map_size=(20.0, 20.0, 8.0), origin=(-10.0, -10.0, -4.0))
        q = workloads.astar_queries(B, 500 + i)
        bx, cnt = _on_line(w, q)
    else:
        raise ValueError(name)
    return dict(world=w, q=q, boxes=bx, count=cnt, local_box=local)


def route_of(case):
    """Which lookup routes the case's boxes are read through, from the kernel's own conditions (tests/astar_path_cases.py)."""
    w, q = case["world"], case["q"]
    routes = set()
    if AC.grid_z(w) > 64:
        routes.add("byte_map")
        return routes
    routes.add("window")                                                    # a packed map stages a window at every expansion
    if max(AC.win_r_wanted(w, q["f_ext"][b]) for b in range(B)) > AC.WIN_R_MAX:
        routes.add("fallback")                                              # ... and a sample beyond its clamped radius reads the packed map
    if case["local_box"] is not None:
        routes.add("local_box")
    return routes
