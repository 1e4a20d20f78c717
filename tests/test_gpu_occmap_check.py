"""GPU tests of the safety timer's checks on the device occupancy map (include/frp_nmpc_occmap_check.h,
solver.OccupancyMap.check_surround / safety_check) against their CPU restatement (tests/occmap_check_oracle.py).  Every output is
an integer, or a double that is a copy or ONE addition of doubles: every comparison is np.array_equal."""
import functools

import numpy as np
import pytest

from forces_resilient_planner_amd import solver, workloads
from tests import occmap_check_oracle as CO
from tests import occmap_oracle as OO
from tests import test_occmap_check_cpu as CC

pytestmark = pytest.mark.gpu
GEO = dict(origin=(-1.2, -1.0, 0.0), map_size=(2.4, 2.0, 4.0), resolution=0.1)
# rows of local_box (min_id, max_id, tested inclusively): planner 0 does not see z > 30, i.e. the slab; planner 1 sees a box well
# inside the map, so that its six faces cut through probe ranges; planner 2 sees everything
BOXES = np.array([[0, 0, 0, 24, 20, 30], [5, 4, 8, 18, 15, 36], [0, 0, 0, 24, 20, 40]], dtype=np.int32)


def small_world():
    """24 x 20 x 40 voxels (gz = 40: a word boundary inside probe ranges, a ragged last word).  Occupied: two blobs and scattered
    single voxels, about 3 % together, and a slab at z in {31, 32} over the half x < 0.  (Scattered voxels ALONE at 3 % would
    leave no point free: a body of 9 x 9 x 3 voxels is free with probability 0.97^243.)"""
    rng = np.random.default_rng(11)
    m = OO.OccMapOracle(**GEO)
    assert tuple(m.grid_size) == (24, 20, 40)
    occ = np.zeros((24, 20, 40), dtype=bool)
    occ[2:6, 13:18, 2:16] = True
    occ[17:21, 2:6, 14:26] = True
    occ |= rng.random(occ.shape) < 0.0012
    occ[0:12, :, 31:33] = True
    m.buffer[occ] = m.clamp_max_log
    return m


def device_map(om):
    import torch
    dm = solver.OccupancyMap(origin=tuple(om.origin), map_size=tuple(om.map_size), resolution=float(om.resolution))
    dm.log_odds.copy_(torch.from_numpy(om.buffer).to(dm.device))
    dm.refresh()
    return dm


def surround_points():
    """Q = 601 (not a multiple of 64, nor of the 4 wavefronts of a workgroup)."""
    rng = np.random.default_rng(12)
    lo, hi = np.array(GEO["origin"]), np.array(GEO["origin"]) + np.array(GEO["map_size"])
    inner = lambda n: np.c_[rng.uniform(-0.75, 0.75, n), rng.uniform(-0.55, 0.55, n), rng.uniform(0.15, 3.85, n)]
    pts = [inner(379)]
    for a in range(3):                        # within half a body (0.45 m, 0.15 m) of each of the six faces: probes leave the map
        for face, s in ((lo[a], 1.0), (hi[a], -1.0)):
            p = inner(10)
            p[:, a] = face + s * rng.uniform(0.0, 0.3 if a < 2 else 0.08, 10)
            pts.append(p)
    faces = inner(100)                        # exactly on voxel faces: origin + k * res, as the map computes them
    k = np.floor((faces - lo) / 0.1)
    on = lo + k * 0.1
    which = rng.random(faces.shape) < 0.6
    faces[which] = on[which]
    pts.append(faces)
    words = inner(60)                         # the z mask spans words 0 and 1 (indices 30 ... 33), over both halves of the slab's plane
    words[:, 2] = rng.uniform(3.1, 3.3, 60)
    pts.append(words)
    pts.append(np.array([[0.1, np.nan, 1.0], [250.0, -3.0e6, 1.0]]))
    pts = np.concatenate(pts)
    assert pts.shape == (601, 3)
    return pts


@functools.lru_cache(maxsize=None)
def surround_reference():
    """(map, points, planner rows, verdicts without a local box, verdicts with BOXES): computed once, shared, never modified."""
    om = small_world()
    pts = surround_points()
    planner = (np.arange(len(pts)) % 3).astype(np.int32)
    whole = np.array([CO.check_pos_surround(om, p, 1.2) for p in pts], dtype=np.int32)
    local = np.array([CO.check_pos_surround(om, p, 1.2, list(BOXES[planner[i]])) for i, p in enumerate(pts)], dtype=np.int32)
    for a in (pts, planner, whole, local):
        a.setflags(write=False)
    return om, pts, planner, whole, local


def test_check_surround_equals_the_restatement():
    import torch
    om, pts, planner, whole, local = surround_reference()
    occupied = om.occ().mean()
    print(f"occupied {occupied:.4f}; free without a box {whole.mean():.3f}, with the boxes {local.mean():.3f}; differ at {int((whole != local).sum())}")
    assert 0.02 < occupied < 0.09
    for v in (whole, local):
        assert 0.25 <= v.mean() <= 0.75                       # the batch is neither all-collide nor all-free
    hidden_slab = (planner == 0) & (whole == 0) & (local == 1)
    assert hidden_slab.sum() >= 5 and (local[planner == 2] == whole[planner == 2]).all()
    assert ((planner == 1) & (whole != local)).sum() >= 5     # the inner box's faces decide some points
    dm = device_map(om)
    pts, planner = pts.copy(), planner.copy()   # (the shared reference is read-only; torch wants writable arrays)
    got = dm.check_surround(pts, 1.2)
    got_local = dm.check_surround(pts, 1.2, local_box=BOXES, planner=planner)
    row0 = dm.check_surround(pts, 1.2, local_box=BOXES[1:2])  # planner NULL: row 0 for every point
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), whole)
    assert np.array_equal(got_local.cpu().numpy(), local)
    assert np.array_equal(row0.cpu().numpy()[planner == 1], local[planner == 1])
    assert dm.check_surround(np.zeros((0, 3)), 1.2).shape == (0,)


def test_a_body_of_63_offsets_per_axis_and_three_mask_words():
    """The largest body the call takes: half-extent 31 on every axis, 63 lanes per axis, a z mask over three words (z = 19 ... 81 of
    a 96-voxel column).  Known answers from index ranges: every point is a voxel centre, half a voxel away from any face, so its
    probes are the voxels c - 31 ... c + 31 per axis.  (The restatement would take 250 047 probes per free point.)"""
    import torch
    geo = dict(origin=(0.0, 0.0, 0.0), map_size=(7.0, 7.0, 9.6), resolution=0.1)
    om = OO.OccMapOracle(**geo)
    grid = (70, 70, 96)
    assert tuple(om.grid_size) == grid
    dm = solver.OccupancyMap(**geo)
    at = [(34, 35, 50), (34, 35, 64), (31, 35, 50), (39, 38, 33)]   # the last one's probes leave the map (39 + 31 = 70)
    pts = np.array([om.index_to_pos(c) for c in at])
    body = (3.1, 3.1)
    assert CO.half_extents(om, 1.0, body) == (31, 31, 31)
    for vox in ((3, 4, 19), (65, 66, 40), (20, 50, 81), (66, 35, 50), (20, 20, 18), (34, 35, 82), None):
        dm.reset()
        if vox is not None:
            dm.insert_cloud(om.index_to_pos(vox).astype(np.float32)[None, :])
        inside = lambda c: all(c[a] - 31 >= 0 and c[a] + 31 <= grid[a] - 1 for a in range(3))
        want = [int(inside(c) and (vox is None or not all(abs(vox[a] - c[a]) <= 31 for a in range(3)))) for c in at]
        got = dm.check_surround(pts, 1.0, body=body)
        torch.cuda.synchronize()
        assert got.cpu().numpy().tolist() == want, (vox, want)
        if vox == (3, 4, 19):
            assert want == [0, 1, 0, 0]   # 34 - 31 = 3 reaches it, z 64 - 31 = 33 does not
        if vox is None:
            assert want == [1, 1, 1, 0]
    assert CO.check_pos_surround(om, pts[3], 1.0, None, body) is False


@pytest.mark.parametrize("ratio", [1.2, 1.5])
def test_single_voxel_known_answers_on_the_device(ratio):
    import torch
    om = CC.known_map()
    dm = solver.OccupancyMap(**CC.KNOWN_GEO)
    dm.insert_cloud(om.index_to_pos(CC.KNOWN_VOXEL).astype(np.float32)[None, :])
    cases = CC.corner_cases(om, ratio)
    got = dm.check_surround(np.array([p for p, _ in cases]), ratio)
    torch.cuda.synchronize()
    assert got.cpu().numpy().tolist() == [0, 1, 1, 1, 0, 1, 1, 1] == [int(f) for _, f in cases]


def test_paths_known_answers():
    import torch
    om = CC.known_map()
    dm = solver.OccupancyMap(**CC.KNOWN_GEO)
    dm.insert_cloud(om.index_to_pos(CC.KNOWN_VOXEL).astype(np.float32)[None, :])
    cases = CC.corner_cases(om, 1.2)
    hit, free = cases[0][0], cases[1][0]
    K = 16
    rows = []   # (kino_size, colliding samples, have_traj, first_hit)
    for size in (0, 1, 5, 6, 11, 16, 40):                            # 16 = K; 40 > K is cut to K
        rows.append((size, (4,), 1, -1))                             # an obstacle only at sample 4: never looked at
        rows.append((size, (5,), 1, 5 if size > 5 else -1))
        rows.append((size, (5, 10), 1, 5 if size > 5 else -1))
        rows.append((size, (10,), 1, 10 if size > 10 else -1))
        rows.append((size, (15,), 1, 15 if size > 15 else -1))
        rows.append((size, (0, 5), 0, -1))                           # no trajectory
    rows.append((16, (0,), 1, 0))
    rows.append((-3, (0,), 1, -1))
    rows.append((7, (), 1, -1))
    B = len(rows)
    path = np.full((B, K, 3), np.nan)
    for b, (size, at, _, _) in enumerate(rows):
        n = max(0, min(size, K))
        path[b, :n] = free                                           # beyond the size: NaN, which would collide if it were read
        for s in at:
            if s < n:
                path[b, s] = hit
    want = np.array([r[3] for r in rows], dtype=np.int32)
    ref = np.array([CO.check_path(om, path[b], rows[b][0], bool(rows[b][2])) for b in range(B)], dtype=np.int32)
    assert np.array_equal(ref, want)                                 # the restatement agrees with the hand-made answers
    dev = dm.device
    end = torch.from_numpy(np.tile(free, (B, 1))).to(dev)
    r = dm.safety_check(end, torch.from_numpy(path).to(dev), torch.tensor([r[0] for r in rows], dtype=torch.int32, device=dev),
                        have_traj=np.array([r[2] for r in rows], dtype=np.int32))
    torch.cuda.synchronize()
    assert np.array_equal(r.first_hit.cpu().numpy(), want)
    assert not r.goal_blocked.any() and np.array_equal(r.replan.cpu().numpy(), (want >= 0).astype(np.int32))
    # another stride, and have_traj NULL
    r3 = dm.safety_check(end, torch.from_numpy(path).to(dev), torch.tensor([r[0] for r in rows], dtype=torch.int32, device=dev), stride=2)
    torch.cuda.synchronize()
    ref3 = np.array([CO.check_path(om, path[b], rows[b][0], True, stride=2) for b in range(B)], dtype=np.int32)
    assert np.array_equal(r3.first_hit.cpu().numpy(), ref3) and (ref3 != want).any()


def test_goals_equal_the_restatement():
    import torch
    om, goal, tab, A, Bp = CC.two_pocket_map()
    # more room: a third pocket region, so that one goal finds several free groups in a row
    om.buffer[2:14, 2:30, 8:19] = om.clamp_min_log
    dm = device_map(om)
    free_goal = np.array([-1.0, 0.0, 1.35])                          # inside the carved region, clear at ratio 1.2
    ends = np.array([free_goal, goal, [1.2, 1.2, 0.25], A, [-0.9, -1.2, 1.0]])
    have = np.array([1, 1, 1, 0, 1], dtype=np.int32)                 # row 3: no target -- it would be free anyway; row 4: candidates leave the map
    ends[3] = goal
    want = [CO.check_goal(om, e, bool(h)) for e, h in zip(ends, have)]
    w_end = np.array([w[0] for w in want]); w_blocked = np.array([w[1] for w in want], dtype=np.int32); w_hits = np.array([w[2] for w in want], dtype=np.int32)
    print("goal_blocked", w_blocked, "goal_hits", w_hits)
    assert w_blocked.tolist() == [0, 1, 1, 0, 1]
    assert w_hits[1] > 1 and w_hits[2] == 0 and np.array_equal(w_end[2], ends[2]) and np.array_equal(w_end[3], goal) and np.array_equal(w_end[0], free_goal)
    dev = dm.device
    end = torch.from_numpy(ends.copy()).to(dev)
    path = torch.zeros((5, 4, 3), dtype=torch.float64, device=dev)
    r = dm.safety_check(end, path, torch.zeros((5,), dtype=torch.int32, device=dev), have_target=have)
    torch.cuda.synchronize()
    assert np.array_equal(r.goal_blocked.cpu().numpy(), w_blocked) and np.array_equal(r.goal_hits.cpu().numpy(), w_hits)
    assert np.array_equal(end.cpu().numpy(), w_end)                  # bit for bit, moved goals included
    assert np.array_equal(r.first_hit.cpu().numpy(), np.full(5, -1)) and np.array_equal(r.replan.cpu().numpy(), w_blocked)
    # behind a local box that hides everything, every goal is free
    end2 = torch.from_numpy(ends.copy()).to(dev)
    r2 = dm.safety_check(end2, path, torch.zeros((5,), dtype=torch.int32, device=dev), local_box=np.tile(np.array([[40, 40, 40, 40, 40, 40]], dtype=np.int32), (5, 1)))
    torch.cuda.synchronize()
    w2 = [CO.check_goal(om, e, True, [40] * 6) for e in ends]
    assert np.array_equal(r2.goal_blocked.cpu().numpy(), np.array([w[1] for w in w2], dtype=np.int32)) and np.array_equal(end2.cpu().numpy(), np.array([w[0] for w in w2]))


def _fleet_case():
    """Four straight paths of 16 samples through the empty small map, one goal each; the one-voxel cloud that blocks planner 2's path."""
    K = 16
    path = np.zeros((4, K, 3))
    for b in range(4):   # every sample is a voxel centre: x index 4 + s, y index 5 + 3 b, z index 5 + 9 b
        path[b, :, 0] = -0.75 + 0.1 * np.arange(K)
        path[b, :, 1] = -0.45 + 0.3 * b
        path[b, :, 2] = 0.55 + 0.9 * b
    end = path[:, -1, :].copy()
    cloud = np.array([path[2, 5]], dtype=np.float32)   # sample 5 of planner 2: out of reach of its samples 0 and 10 and of its goal
    return path, end, cloud


def test_the_checks_read_the_live_bit_plane():
    import torch
    path, end, cloud = _fleet_case()
    dm = solver.OccupancyMap(**GEO)
    dev = dm.device
    kp = torch.from_numpy(path).to(dev); sz = torch.full((4,), 16, dtype=torch.int32, device=dev); e = torch.from_numpy(end).to(dev)
    r = dm.safety_check(e, kp, sz); torch.cuda.synchronize()
    assert r.replan.cpu().numpy().tolist() == [0, 0, 0, 0]
    dm.insert_cloud(cloud)
    r = dm.safety_check(e, kp, sz); torch.cuda.synchronize()
    assert r.replan.cpu().numpy().tolist() == [0, 0, 1, 0] and r.first_hit.cpu().numpy().tolist() == [-1, -1, 5, -1]
    dm.clear_box(cloud[0] - 0.05, cloud[0] + 0.05)
    r = dm.safety_check(e, kp, sz); torch.cuda.synchronize()
    assert r.replan.cpu().numpy().tolist() == [0, 0, 0, 0] and np.array_equal(e.cpu().numpy(), end)


def test_a_captured_safety_check_follows_the_map():
    import torch
    path, end, cloud = _fleet_case()
    dm = solver.OccupancyMap(**GEO)
    dev = dm.device
    kp = torch.from_numpy(path).to(dev); sz = torch.full((4,), 16, dtype=torch.int32, device=dev); e = torch.from_numpy(end).to(dev)
    out = dm.safety_check(e, kp, sz)   # warm-up: the goal table is uploaded, the output buffers exist
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            dm.safety_check(e, kp, sz, out=out)
    g.replay(); torch.cuda.synchronize()
    assert out.replan.cpu().numpy().tolist() == [0, 0, 0, 0]
    dm.insert_cloud(cloud); torch.cuda.synchronize()
    g.replay(); torch.cuda.synchronize()
    assert out.replan.cpu().numpy().tolist() == [0, 0, 1, 0] and out.first_hit.cpu().numpy().tolist() == [-1, -1, 5, -1]
    dm.reset(); torch.cuda.synchronize()
    g.replay(); torch.cuda.synchronize()
    assert out.replan.cpu().numpy().tolist() == [0, 0, 0, 0]


def astar_case():
    """The empty world of tests/test_gpu_astar.py, four planners flying along x at y = -6, -2, 2, 6, and a block across the paths of
    planners 1 and 2 (small enough to fly around: a fresh search reaches its horizon, tests/astar_lib says so on the CPU)."""
    w = workloads.astar_world(0, "empty", allocate_num=12000)
    a = lambda rows: np.asarray(rows, dtype=float)
    ys = (-6.05, -2.05, 1.95, 5.95)
    q = dict(start_pt=a([(-6.05, y, 1.05) for y in ys]), start_v=np.zeros((4, 3)), start_a=np.zeros((4, 3)),
             end_pt=a([(3.95, y, 1.05) for y in ys]), end_v=np.zeros((4, 3)), f_ext=np.zeros((4, 3)))
    xs, zs = np.arange(-1.05, -0.74, 0.1), np.arange(0.55, 1.66, 0.1)
    block = np.array([(x, y + dy, z) for y in ys[1:3] for x in xs for dy in np.arange(-0.4, 0.41, 0.1) for z in zs], dtype=np.float32)
    return w, q, block


def test_replan_mask_feeds_the_astar():
    import torch
    w, q, block = astar_case()
    dm = solver.OccupancyMap(w)
    pl = solver.AstarPlanner(dm, 4, K=512)
    pl.upload(q["start_pt"], q["start_v"], q["start_a"], q["end_pt"], q["end_v"], q["f_ext"])
    pl.plan(); torch.cuda.synchronize()
    assert (pl.kino_size > 0).all() and (pl.status != solver.ASTAR_NO_PATH).all()
    end = torch.from_numpy(q["end_pt"].copy()).to(dm.device)
    r = dm.safety_check(end, pl.kino_path, pl.kino_size); torch.cuda.synchronize()
    assert r.replan.cpu().numpy().tolist() == [0, 0, 0, 0]
    before = pl.kino_path.clone(); size0 = pl.kino_size.clone()
    dm.insert_cloud(block)
    r = dm.safety_check(end, pl.kino_path, pl.kino_size); torch.cuda.synchronize()
    assert r.replan.cpu().numpy().tolist() == [0, 1, 1, 0] and not r.goal_blocked.any()
    assert (r.first_hit[1:3] > 0).all() and np.array_equal(end.cpu().numpy(), q["end_pt"])
    pl.plan(active=r.replan); torch.cuda.synchronize()
    assert (pl.status != solver.ASTAR_NO_PATH).all()
    for b in (0, 3):
        assert torch.equal(pl.kino_path[b], before[b]) and int(pl.kino_size[b]) == int(size0[b])
    for b in (1, 2):
        assert not torch.equal(pl.kino_path[b], before[b])
    r = dm.safety_check(end, pl.kino_path, pl.kino_size); torch.cuda.synchronize()
    assert r.first_hit.cpu().numpy().tolist() == [-1, -1, -1, -1] and r.replan.cpu().numpy().tolist() == [0, 0, 0, 0]
