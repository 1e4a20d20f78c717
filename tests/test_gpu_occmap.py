"""GPU tests of the occupancy map (include/frp_nmpc.h (8), solver.OccupancyMap) against its CPU restatement
(tests/occmap_oracle.py).  Every output is an integer, a byte or a double that went through float32: equality is exact
(np.array_equal), nothing here has a tolerance except the comparison with the corridor oracle, which is the existing corridor
test's own."""
import os
import subprocess
import sys

import numpy as np
import pytest

from forces_resilient_planner_amd import layout as L, solver, workloads
from tests import occmap_oracle as OO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEO = dict(origin=(-10.0, -10.0, -1.0), map_size=(20.0, 20.0, 4.0), resolution=0.1)


def _seeded_cloud(rng, n):
    """Points inside the map, outside it on every side, exactly on voxel faces and on the map's faces, NaNs."""
    pts = np.c_[rng.uniform(-11, 11, n), rng.uniform(-11, 11, n), rng.uniform(-1.5, 3.5, n)]
    k = n // 8
    pts[:k] = np.round(pts[:k] * 10) / 10                                 # on faces (as far as float32 has them)
    pts[k:k + 6] = [[-10, 0, 0], [10, 0, 0], [0, -10, 0], [0, 10, 0], [0, 0, -1], [0, 0, 3]]   # the map's own faces: near ones in, far ones out
    pts[k + 6:k + 12] = [[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [np.inf, 0, 0], [-np.inf, 0, 0], [3e38, 1, 1]]
    pts[k + 12] = [-10.00001, 0.05, 0.05]                                 # just below the origin: floor, not truncation
    return pts.astype(np.float32)


def _views_equal(dm, om, centres, P=None):
    """local_box, cloud_count and the first cloud_count points of every planner against the restatement, in order.  P None: the
    restatement's own maximum count, so that no planner overflows."""
    want = [om.local_cloud(c) for c in centres] if centres is not None else [om.local_cloud(None)]
    if P is None:
        P = max(1, max(len(w) for w in want))
    assert P <= solver.CORRIDOR_MAX_POINTS
    v = dm.local_view(None if centres is None else np.asarray(centres, dtype=np.float64), P)
    import torch
    torch.cuda.synchronize()
    box = v.local_box.cpu().numpy(); cnt = v.cloud_count.cpu().numpy()
    assert np.array_equal(box, np.array([om.local_box(c) for c in centres] if centres is not None else [om.local_box(None)], dtype=np.int32))
    assert np.array_equal(cnt, np.array([len(w) for w in want], dtype=np.int32))
    for i0 in range(0, len(want), 256):
        got = v.cloud[i0:i0 + 256].cpu().numpy()
        for j, w in enumerate(want[i0:i0 + 256]):
            assert np.array_equal(got[j, :len(w)], w), i0 + j
    return v, want


def test_insert_reset_clear_box_and_refresh():
    import torch
    rng = np.random.default_rng(41)
    dm = solver.OccupancyMap(**GEO)
    om = OO.OccMapOracle(**GEO)
    assert dm.grid == tuple(om.grid_size) == (200, 200, 40)
    torch.cuda.synchronize()
    assert np.array_equal(dm.log_odds.cpu().numpy(), om.buffer) and not dm.occ.any()
    pts = _seeded_cloud(rng, 20000)
    dm.insert_cloud(pts); om.insert_cloud(pts)
    torch.cuda.synchronize()
    lo1 = dm.log_odds.cpu().numpy()
    assert np.array_equal(lo1, om.buffer) and np.array_equal(dm.occ.cpu().numpy(), om.occ())
    assert 10000 < int(om.occ().sum()) < 20000                                   # points were dropped, voxels were hit
    assert om.buffer[0, 100, 10] == 0.97 and om.occ()[0, 100, 10] == 1          # (-10, 0, 0): the near face is inside
    _views_equal(dm, om, None)                                                   # the bit plane followed (globalOccVisCallback's cloud)
    dm.insert_cloud(pts)                                                         # a second insert of the same cloud changes nothing
    torch.cuda.synchronize()
    assert np.array_equal(dm.log_odds.cpu().numpy(), lo1) and np.array_equal(dm.occ.cpu().numpy(), om.occ())
    _views_equal(dm, om, None)
    for lo, hi in (((-3.0, -12.0, 0.0), (2.5, 1.05, 9.0)), ((8.0, 8.0, 2.0), (30.0, 30.0, 30.0)), ((-30.0, -30.0, -30.0), (-9.95, -9.9, -0.9)),
                   ((20.0, 20.0, 20.0), (30.0, 30.0, 30.0)), ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))):
        dm.clear_box(lo, hi); om.reset_buffer(lo, hi)
        torch.cuda.synchronize()
        assert np.array_equal(dm.log_odds.cpu().numpy(), om.buffer) and np.array_equal(dm.occ.cpu().numpy(), om.occ()), (lo, hi)
    _views_equal(dm, om, None)
    _views_equal(dm, om, [(0.0, 0.0, 1.0), (-2.9, 1.0, 0.4)])
    # the caller writes log_odds itself (its own fusion): values around the threshold, then refresh
    own = rng.choice([0.12, 0.5, 0.80, 0.8000000000000002, 0.97], size=om.buffer.shape, p=[0.9, 0.04, 0.02, 0.02, 0.02])
    dm.log_odds.copy_(torch.from_numpy(own).to(dm.device)); om.buffer[...] = own
    dm.refresh(); torch.cuda.synchronize()
    assert np.array_equal(dm.occ.cpu().numpy(), om.occ()) and int(om.occ().sum()) == int((own > 0.80).sum())
    _views_equal(dm, om, [(0.0, 0.0, 1.0), (9.0, -9.0, 2.5)], P=None)
    dm.reset(); om.reset(); torch.cuda.synchronize()
    assert np.array_equal(dm.log_odds.cpu().numpy(), om.buffer) and not dm.occ.any()
    v, _ = _views_equal(dm, om, None)
    assert int(v.cloud_count[0]) == 0


def _centres(rng, B, om):
    """Random centres in and around the map; near and outside every face; two planners at the same centre."""
    lo, hi = om.min_range, om.max_range
    c = rng.uniform(lo - 2.0, hi + 2.0, (B, 3))
    special = []
    mid = (lo + hi) / 2
    for k in range(3):
        for edge, s in ((lo[k], -1.0), (hi[k], 1.0)):
            for d in (-0.05, 0.05, s * (om.sensor_range[k] + 0.05), s * (om.sensor_range[k] - 0.05), s * 100.0):
                p = mid.copy(); p[k] = edge + d
                special.append(p)
    special = np.array(special)[:max(0, B - 2)]
    c[:len(special)] = special
    if B >= 2:
        c[-1] = c[0] if B == 2 else c[B // 2]
    return c


@pytest.mark.parametrize("B,seed,n_obstacles", [(1, 0, 20), (7, 1, 20), (1024, 2, 12), (4096, 3, 12)])
def test_local_view_matches_the_restatement(B, seed, n_obstacles):
    w = workloads.astar_world(seed, "pillars", n_obstacles=n_obstacles)
    dm = solver.OccupancyMap(w)
    om = OO.from_world(w)
    assert np.array_equal(dm.occ.cpu().numpy(), w["occ"]) and np.array_equal(dm.log_odds.cpu().numpy(), om.buffer)
    rng = np.random.default_rng(100 + seed)
    c = _centres(rng, B, om) if B > 1 else np.array([[0.3, -0.2, 1.0]])
    v, want = _views_equal(dm, om, c)
    n = np.array([len(x) for x in want])
    assert n.max() > 1000 and (B < 7 or n.min() == 0)             # crowded ranges and (from B = 7) ranges with nothing in them
    if B >= 7:
        same = B // 2 if B > 2 else 0
        assert np.array_equal(c[-1], c[same]) and n[-1] == n[same]
        assert np.array_equal(v.cloud[-1, :n[-1]].cpu().numpy(), v.cloud[same, :n[same]].cpu().numpy())
    if B == 1:
        assert np.array_equal(want[0], om.local_cloud_loops(c[0]))   # the vectorised restatement against the loops as written, once at full size
    _views_equal(dm, om, None)                                       # whole-map mode = globalOccVisCallback's restatement


def test_overflow_keeps_the_first_points_and_negates_the_count():
    import torch
    w = workloads.astar_world(1, "pillars", n_obstacles=20)
    dm = solver.OccupancyMap(w); om = OO.from_world(w)
    c = _centres(np.random.default_rng(7), 7, om)
    c[0] = (0.0, 0.0, 1.0); c[6] = c[0]
    want = [om.local_cloud(x) for x in c]
    n = np.array([len(x) for x in want])
    assert n[0] == n.max() and n[0] > 2000
    others = [i for i in range(7) if 0 < n[i] < n[0]]
    assert others
    P = int(max(n[i] for i in others))                               # everyone but planners 0 and 6 fits
    assert P < n[0]
    v = dm.local_view(c, P); torch.cuda.synchronize()
    cnt = v.cloud_count.cpu().numpy(); cl = v.cloud.cpu().numpy()
    for i in range(7):
        if n[i] > P:
            assert cnt[i] == -n[i] and np.array_equal(cl[i], want[i][:P])
        else:
            assert cnt[i] == n[i] and np.array_equal(cl[i, :n[i]], want[i])
    assert cnt[0] < 0 and cnt[6] < 0 and v.overflowed().cpu().tolist() == [bool(x > P) for x in n]
    assert np.array_equal(v.local_box.cpu().numpy(), np.array([om.local_box(x) for x in c], dtype=np.int32))
    # P = 0: counts only; P = 1
    v0 = dm.local_view(c, 0); v1 = dm.local_view(c, 1); torch.cuda.synchronize()
    assert np.array_equal(v0.cloud_count.cpu().numpy(), -n)
    assert np.array_equal(v1.cloud_count.cpu().numpy(), np.where(n > 1, -n, n))
    assert all(np.array_equal(v1.cloud[i, 0].cpu().numpy(), want[i][0]) for i in range(7) if n[i] > 0)


def test_point_query():
    import torch
    w = workloads.astar_world(4, "pillars", n_obstacles=20)
    dm = solver.OccupancyMap(w, local_radius=(3.0, 2.0, 1.0)); om = OO.from_world(w, local_radius=(3.0, 2.0, 1.0))
    rng = np.random.default_rng(9)
    B, Q = 5, 4000
    c = rng.uniform(-6, 6, (B, 3)) * np.array([1, 1, 0.2]) + np.array([0, 0, 1.0])
    occ_idx = np.argwhere(w["occ"] > 0)
    pos = rng.uniform(om.min_range - 0.5, om.max_range + 0.5, (Q, 3))
    k = Q // 2
    pos[:k] = om.origin + (occ_idx[rng.integers(0, len(occ_idx), k)] + rng.uniform(0.01, 0.99, (k, 3))) * 0.1   # inside occupied voxels
    pos[k:k + 4] = [[np.nan, 0, 0], [10.0, 0, 0], [-10.0, 0, 0], [-10.00001, 0, 0]]
    planner = rng.integers(0, B, Q).astype(np.int32)
    v = dm.local_view(c, 0)
    boxes = [om.local_box(x) for x in c]
    got_all = dm.query(pos).cpu().numpy()
    got_box = dm.query(pos, v.local_box, planner).cpu().numpy()
    got_row0 = dm.query(pos, v.local_box).cpu().numpy()
    torch.cuda.synchronize()
    assert np.array_equal(got_all, np.array([om.get_voxel_state(p) for p in pos], dtype=np.int32))
    assert np.array_equal(got_box, np.array([om.get_voxel_state(p, boxes[b]) for p, b in zip(pos, planner)], dtype=np.int32))
    assert np.array_equal(got_row0, np.array([om.get_voxel_state(p, boxes[0]) for p in pos], dtype=np.int32))
    for g in (got_all, got_box):
        assert set(np.unique(g)) == {-1, 0, 1}
    assert (got_all == 1).sum() > (got_box == 1).sum() > 0                       # the local cut hides occupied voxels


# ---- consumers ----
def _tunnel_world(seed, B, N=20, P=6000):
    """tests/test_gpu_parity.py's corridor world, voxelised: its random cloud (a free tunnel along a curved path) is inserted into an
    empty map; planners fly along the tunnel.  Returns the device map, the restatement, ref / yaw / E (host) and the centres."""
    rng = np.random.default_rng(seed)
    cloud = np.c_[rng.uniform(-3, 9, P), rng.uniform(-4, 4, P), rng.uniform(-0.5, 3, P)]
    s = np.linspace(0, 5, N)
    centre = np.c_[s, 0.4 * np.sin(0.8 * s), 1.0 + 0.1 * np.cos(s)]
    cx = np.interp(cloud[:, 0], centre[:, 0], centre[:, 1]); cz = np.interp(cloud[:, 0], centre[:, 0], centre[:, 2])
    cloud = cloud[np.hypot(cloud[:, 1] - cx, cloud[:, 2] - cz) > 0.75].astype(np.float32)
    ref = centre[None] + rng.normal(0, 0.03, (B, N, 3))
    yaw = np.arctan2(np.gradient(centre[:, 1]), np.gradient(centre[:, 0]))[None] + rng.normal(0, 0.05, (B, N))
    z = np.zeros((B, N, 17)); z[..., 3] = 7.3; z[..., 8:11] = ref; z[..., 16] = yaw
    z[..., 11:14] = rng.normal(0, 0.5, (B, N, 3)); z[..., 14:16] = rng.normal(0, 0.1, (B, N, 2))
    E = solver.tube_batch_host(z)
    radius = (4.0, 3.0, 3.0)
    dm = solver.OccupancyMap(local_radius=radius, **GEO); om = OO.OccMapOracle(local_radius=radius, **GEO)
    dm.insert_cloud(cloud); om.insert_cloud(cloud)
    return dm, om, ref, yaw, E, ref[:, 0].copy()


def _corridor(cloud, count, ref, yaw, E, F=64):
    import torch
    dev = "cuda:0"
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    B, N, _ = ref.shape
    A = torch.zeros((B, N, F, 3), dtype=torch.float64, device=dev); b = torch.zeros((B, N, F), dtype=torch.float64, device=dev)
    nf = torch.zeros((B, N), dtype=torch.int32, device=dev); pi = torch.zeros((B, N), dtype=torch.int32, device=dev)
    cnt = torch.zeros((B,), dtype=torch.int32, device=dev)
    solver.corridor_batch_device(cloud, up(ref), up(yaw), up(E), A, b, nf, pi, cnt, cloud_count=count)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (A, b, nf, pi, cnt)]


def _host_clouds(want, P):
    pad = np.full((len(want), P, 3), 1e30)     # storage beyond the count: anything
    for i, w_ in enumerate(want):
        pad[i, :len(w_)] = w_
    return pad, np.array([len(w_) for w_ in want], dtype=np.int32)


def test_corridor_from_the_device_exported_clouds():
    import torch
    B = 48
    dm, om, ref, yaw, E, c = _tunnel_world(61, B)
    v, want = _views_equal(dm, om, c)
    P = v.cloud.shape[1]
    assert min(len(w_) for w_ in want) > 500 and len({len(w_) for w_ in want}) > 1
    dev_out = _corridor(v.cloud, v.cloud_count, ref, yaw, E)
    pad, n = _host_clouds(want, P)
    host_out = _corridor(torch.from_numpy(pad).to("cuda:0"), torch.from_numpy(n).to("cuda:0"), ref, yaw, E)
    for g, h in zip(dev_out, host_out):
        assert np.array_equal(g, h)
    A, b, nf, pi, cnt = dev_out
    assert pi.max() >= 1 and (cnt > 0).all()
    # a small batch against oracle/corridor_oracle.py, under tests/test_gpu_parity.py::_check_corridor's criterion
    sys.path.insert(0, ROOT)
    from oracle import corridor_oracle as C
    for p in range(4):
        idx, polys = C.corridor_one(ref[p], yaw[p], E[p], want[p])
        assert np.array_equal(pi[p], idx), (p, pi[p], idx)
        assert cnt[p] == len(polys)
        for k, (Ao, bo) in enumerate(polys):
            assert nf[p, k] == len(bo), (p, k, nf[p, k], len(bo))
            G = np.c_[A[p, k, :len(bo)], b[p, k, :len(bo)]]; O = np.c_[Ao, bo]
            assert np.max(np.abs(G - O)) < 1e-9, (p, k)
        assert np.all(nf[p, len(polys):] == 0)


def test_astar_planner_built_from_the_map():
    import torch
    w = workloads.astar_world(7, "pillars", allocate_num=12000, n_obstacles=20)
    B = 6
    q = workloads.astar_queries(B, 7)
    radius = (4.0, 4.0, 3.0)                     # shorter than the searches: the local cut changes what they see
    dm = solver.OccupancyMap(w, local_radius=radius); om = OO.from_world(w, local_radius=radius)
    v = dm.local_view(q["start_pt"], 0)
    np_box = np.array([om.local_box(x) for x in q["start_pt"]], dtype=np.int32)
    a = solver.AstarPlanner(dm, B, K=1024, want_path_nodes=True)
    h = solver.AstarPlanner(w, B, K=1024, want_path_nodes=True)
    assert a.occ.data_ptr() == dm.occ.data_ptr()
    for pl, box in ((a, v.local_box), (h, torch.from_numpy(np_box).to("cuda:0"))):
        pl.upload(q["start_pt"], q["start_v"], q["start_a"], q["end_pt"], q["end_v"], q["f_ext"])
        pl.plan(local_box=box)
    torch.cuda.synchronize()
    assert np.array_equal(v.local_box.cpu().numpy(), np_box)
    for name in ("status", "kino_size", "stats", "kino_path", "path_nodes"):
        assert torch.equal(getattr(a, name), getattr(h, name)), name
    assert (a.kino_size > 0).any()
    free = solver.AstarPlanner(w, B, K=1024)
    free.upload(q["start_pt"], q["start_v"], q["start_a"], q["end_pt"], q["end_v"], q["f_ext"]); free.plan(); torch.cuda.synchronize()
    assert not (torch.equal(free.kino_path, a.kino_path) and torch.equal(free.stats, a.stats))   # the box was used
    # the planner searches the map's own buffer: an insert is seen without a new planner
    wall = np.c_[np.full(4000, -5.0), np.random.default_rng(0).uniform(-10, 10, 4000), np.random.default_rng(1).uniform(-1, 3, 4000)]
    dm.insert_cloud(wall); torch.cuda.synchronize()
    assert torch.equal(a.occ, dm.occ) and int(dm.occ.sum()) > int(w["occ"].sum())


def test_fleet_replan_and_full_tick_from_the_map():
    """One replan + one full tick of a fleet fed by the map (device local_box, device per-planner clouds) against the same fleet fed
    by host-prepared arrays (the restatement's boxes and clouds, uploaded): same bits."""
    import torch
    w = workloads.astar_world(21, "pillars", allocate_num=12000, n_obstacles=15)
    B, N = 6, 20
    q = workloads.astar_queries(B, 21)
    radius = (5.0, 5.0, 3.0)
    dm = solver.OccupancyMap(w, local_radius=radius); om = OO.from_world(w, local_radius=radius)
    dev = dm.device
    mpc = np.zeros((B, N + 1, 17)); mpc[:, :, 3] = mpc[:, :, 7] = 7.3
    mpc[:, :, 8:11] = q["start_pt"][:, None, :]
    want = [om.local_cloud(x) for x in q["start_pt"]]
    P = max(len(x) for x in want)
    pad, n = _host_clouds(want, P)
    np_box = np.array([om.local_box(x) for x in q["start_pt"]], dtype=np.int32)
    results = []
    for from_map in (True, False):
        fleet = solver.DeviceFleet(B, N, 30, 64, L.MODEL_NORMAL, (15.0, 3.0, 80.0, 15.0, 0.0))
        fleet.mpc_output.copy_(torch.from_numpy(mpc).to(dev)); fleet.solver.exitflag.fill_(1)
        if from_map:
            v = dm.local_view(fleet.mpc_output[:, 1, 8:11], P)       # centres straight from the plans in HBM
            pl = solver.AstarPlanner(dm, B, K=1024)
            box, cloud, count = v.local_box, v.cloud, v.cloud_count
        else:
            pl = solver.AstarPlanner(w, B, K=1024)
            box, cloud, count = (torch.from_numpy(x).to(dev) for x in (np_box, pad, n))
        toff = torch.full((B,), 0.3, dtype=torch.float64, device=dev)
        flags = torch.ones((B,), dtype=torch.int32, device=dev)
        end = torch.from_numpy(q["end_pt"]).to(dev); fext = torch.from_numpy(q["f_ext"]).to(dev)
        odom = (torch.from_numpy(q["start_pt"]).to(dev), torch.from_numpy(q["start_v"]).to(dev))
        ok = fleet.replan(pl, end, fext, flags, time_offset=toff, odom=odom, local_box=box)
        rp = torch.zeros((B, N, 3), dtype=torch.float64, device=dev); ry = torch.zeros((B, N), dtype=torch.float64, device=dev)
        fleet.full_tick(fext, pl.kino_path, toff, cloud, rp, ry, kino_size=pl.kino_size, cloud_count=count)
        torch.cuda.synchronize()
        results.append([t.cpu().numpy() for t in (ok, pl.status, pl.kino_size, pl.kino_path, toff, rp, ry, fleet.poly_A, fleet.poly_b, fleet.poly_nfaces,
                                                  fleet.poly_index, fleet.poly_count, fleet.solver.exitflag, fleet.solver.iters, fleet.mpc_output)])
    for a, b in zip(*results):
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    ok, status = results[0][0], results[0][1]
    assert ok.any() and (results[0][11] > 0).all() and (results[0][9].sum(axis=1) > 0).all()


def test_local_view_and_corridor_captured_into_a_graph():
    """The local view + a corridor call captured once, replayed twice with centres moved on the device: the eager results."""
    import torch
    B = 16
    dm, om, ref, yaw, E, c0 = _tunnel_world(62, B)
    dev = dm.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    moves = [c0, c0 + np.array([0.35, -0.1, 0.05]), c0 + np.array([-0.6, 0.25, -0.1])]
    P = max(len(om.local_cloud(x)) for m in moves for x in m)
    d_ref, d_yaw, d_E = up(ref), up(yaw), up(E)
    F, N = 64, ref.shape[1]
    def mk():   # storage the corridor leaves unwritten (rows beyond a polytope's faces) holds the same filler in the eager and the replayed runs
        return (torch.full((B, N, F, 3), -7.0, dtype=torch.float64, device=dev), torch.full((B, N, F), -7.0, dtype=torch.float64, device=dev),
                torch.full((B, N), -7, dtype=torch.int32, device=dev), torch.full((B, N), -7, dtype=torch.int32, device=dev),
                torch.full((B,), -7, dtype=torch.int32, device=dev))

    def step(centres, view, out, stream=None):
        dm.local_view(centres, P, out=view, stream=stream)
        solver.corridor_batch_device(view.cloud, d_ref, d_yaw, d_E, *out, cloud_count=view.cloud_count, stream=stream)

    eager = []
    for m in moves:
        out = mk(); view = dm.local_view(up(m), P)
        step(up(m), view, out); torch.cuda.synchronize()
        eager.append([t.clone() for t in (view.local_box, view.cloud_count) + out])
    assert not torch.equal(eager[0][1], eager[1][1])                 # the moves change what is in range
    centres = up(moves[0]); out = mk(); view = dm.local_view(centres, P)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step(centres, view, out, stream=side)                        # warm-up on the capture stream
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step(centres, view, out, stream=torch.cuda.current_stream())
    for k in (1, 2):
        centres.copy_(up(moves[k]))                                  # device-side update: the graph reads the new centres
        for t in out:
            t.fill_(-7)
        view.cloud_count.fill_(-7)
        torch.cuda.synchronize()
        g.replay(); torch.cuda.synchronize()
        got = (view.local_box, view.cloud_count) + out
        for a, b in zip(got, eager[k]):
            assert torch.equal(a, b), k
        n = view.cloud_count.cpu().numpy()
        for i in (0, B - 1):
            assert np.array_equal(view.cloud[i, :n[i]].cpu().numpy(), om.local_cloud(moves[k][i]))


def test_plain_c_program_drives_map_corridor_and_astar(tmp_path):
    """tests/cpp/occmap_harness.c: C99 + HIP runtime + include/frp_nmpc.h only.  Fills a map from a cloud, takes the local view and
    runs corridor + A* from it; same bits as the Python classes on the same input."""
    import torch
    exe = os.path.join(ROOT, "tests", "cpp", "occmap_harness")
    src = exe + ".c"
    libdir = os.path.dirname(solver.LIB_PATH)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(solver.LIB_PATH), os.path.getmtime(os.path.join(ROOT, "include", "frp_nmpc.h"))):
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", src, "-o", exe,
                               "-L" + libdir, "-lfrp_nmpc_amd", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    B, N, K = 5, 20, 512
    dm, om, ref, yaw, E, c = _tunnel_world(63, B)
    w = dm.astar_world()
    pts = om.local_cloud(None).astype(np.float32)                    # the map's own cloud refills an empty map identically
    P = max(len(om.local_cloud(x)) for x in c)
    start = c.copy(); end = ref[:, -1].copy()
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        np.array([B, N, K, len(pts), P, 12000], dtype=np.int32).tofile(f)
        np.array(list(GEO["origin"]) + list(GEO["map_size"]) + [GEO["resolution"]] + list(dm.local_radius), dtype=np.float64).tofile(f)
        pts.tofile(f)
        for a in (c, ref, yaw, E, start, end):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    subprocess.check_call([exe, str(inp), str(out)])
    raw = np.fromfile(out, dtype=np.uint8)
    nd = (B * P * 3 + B * K * 3) * 8
    dbl = raw[:nd].view(np.float64); ints = raw[nd:].view(np.int32)
    cloud_c = dbl[:B * P * 3].reshape(B, P, 3); path_c = dbl[B * P * 3:].reshape(B, K, 3)
    parts = np.split(ints, np.cumsum([6 * B, B, B * N, B * N, B]))
    box_c, cnt_c, pi_c, nf_c, st_c, ks_c = parts[0].reshape(B, 6), parts[1], parts[2].reshape(B, N), parts[3].reshape(B, N), parts[4], parts[5]
    assert len(ks_c) == B
    v, want = _views_equal(dm, om, c, P)
    assert np.array_equal(box_c, v.local_box.cpu().numpy()) and np.array_equal(cnt_c, v.cloud_count.cpu().numpy())
    for i in range(B):
        assert np.array_equal(cloud_c[i, :cnt_c[i]], want[i])
    A, b, nf, pi, cnt = _corridor(v.cloud, v.cloud_count, ref, yaw, E)
    assert np.array_equal(pi_c, pi) and np.array_equal(nf_c, nf)
    pl = solver.AstarPlanner(dm, B, K=K, allocate_num=12000)
    z3 = np.zeros((B, 3))
    pl.upload(start, z3, z3, end, z3, z3); pl.plan(local_box=v.local_box); torch.cuda.synchronize()
    assert np.array_equal(st_c, pl.status.cpu().numpy()) and np.array_equal(ks_c, pl.kino_size.cpu().numpy())
    kp = pl.kino_path.cpu().numpy()
    for i in range(B):
        assert np.array_equal(path_c[i, :ks_c[i]], kp[i, :ks_c[i]])
    assert (ks_c > 0).any()
