"""GPU tests of the device-built shared view (include/frp_nmpc_occmap_view.h, solver.SharedView / OccupancyMap.shared_view_device and
view= of corridor_batch_device / DeviceFleet): the cloud against tests/occmap_oracle.py and OccupancyMap.local_view, the grid against
solver.CloudGrid, and the corridor through the view -- a device-side count WITH the grid -- against the shared_view() route and the
per-planner clouds.  Routes must agree to the bit (np.array_equal on all five outputs, poisoned output buffers); the oracle comparison
is tests/test_gpu_occmap.py::test_corridor_from_the_device_exported_clouds' own criterion (equal indices and row counts, rows <= 1e-9)."""
import functools

import numpy as np
import pytest

from forces_resilient_planner_amd import layout as L, solver
from tests import occmap_fusion_oracle as FO
from tests import occmap_oracle as OO
from tests import occmap_render_cases as RC
from tests.test_corridor_cut_cpu import tunnel_inputs
from tests.test_gpu_corridor_cut import DENSE, POISON, _against_oracle, _outputs, _per_planner, _run, _same, _up, dense_counts
from tests.test_gpu_occmap import GEO, _tunnel_world

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run_view(view, ref, yaw, E, F=64, cut=None, consts=None):
    import torch
    B, N, _ = ref.shape
    out = _outputs(B, N, F)
    solver.corridor_batch_device(None, _up(ref), _up(yaw), _up(E), *out, view=view, cut=cut, consts=consts)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _counts(view):
    import torch
    torch.cuda.synchronize()
    return int(view.count.item()), int(view.total.item())


def _cells(start, index, n):
    """The grid as (start, cloud indices sorted inside every cell): order inside a cell is free."""
    start, index = start.cpu().numpy(), index.cpu().numpy()[:n]
    assert start[0] == 0 and start[-1] == n and (np.diff(start) >= 0).all()
    cell = np.repeat(np.arange(len(start) - 1), np.diff(start))
    return start, index[np.lexsort((index, cell))]


def _same_grid(view, grid, n):
    assert view.grid.origin == grid.origin and view.grid.dims == grid.dims and view.grid.cell == grid.cell
    s0, i0 = _cells(view.grid.start, view.grid.index, n)
    s1, i1 = _cells(grid.start, grid.index, n)
    assert np.array_equal(s0, s1) and np.array_equal(i0, i1)
    assert sorted(i0.tolist()) == list(range(n))
    pts, idx = view.grid.points.cpu().numpy()[:n], view.grid.index.cpu().numpy()[:n]
    assert np.array_equal(pts, view.cloud.cpu().numpy()[idx])                  # every sorted point is the cloud point its index names


@functools.lru_cache(maxsize=None)
def _dense(mode):
    return dense_counts(*DENSE[mode])


def test_cloud_grid_and_corridor_on_the_tunnel_world():
    import torch
    B = 48
    dm, om, ref, yaw, E, c = _tunnel_world(61, B)
    whole = om.local_cloud(None)
    view = dm.shared_view_device()
    view.update()
    n, total = _counts(view)
    assert n == total == len(whole) and not bool(view.overflowed().item())
    assert np.array_equal(view.cloud[:n].cpu().numpy(), whole)
    lv = dm.local_view(None, solver.CORRIDOR_MAX_POINTS)
    assert torch.equal(view.cloud[:n], lv.cloud[0, :n]) and int(lv.cloud_count[0].item()) == n
    shared, grid = dm.shared_view()
    assert grid.dims == (40, 40, 8)
    _same_grid(view, grid, n)
    want = [om.local_cloud(x) for x in c]
    boxes = dm.local_view(c, 0)
    cut = dm.cut(boxes.local_box)
    a = _run_view(view, ref, yaw, E, cut=cut)
    _same(a, _run(shared, ref, yaw, E, grid=grid, cut=cut), "shared_view() + grid + cut")
    v = dm.local_view(c, max(len(w_) for w_ in want))
    _same(a, _run(v.cloud, ref, yaw, E, count=v.cloud_count), "per-planner clouds")
    _same(_run_view(view, ref, yaw, E), _run(shared, ref, yaw, E, grid=grid), "no cut")
    assert a[3].max() >= 1 and (a[4] > 0).all()
    _against_oracle(a, ref, yaw, E, want, range(4))


ODD = dict(origin=(-4.0, -3.0, -1.0), map_size=(9.25, 7.25, 8.25), resolution=0.25)   # 37 x 29 x 33: 1073 columns, a second word of one bit


def test_odd_geometry_partial_tiles_a_partial_last_word_and_a_group_boundary_inside_a_run():
    rng = np.random.default_rng(7)
    dm = solver.OccupancyMap(**ODD); om = OO.OccMapOracle(**ODD)
    assert dm.grid == (37, 29, 33)
    ids = np.c_[rng.integers(0, 37, 300), rng.integers(0, 29, 300), rng.integers(0, 33, 300)]
    forced = [(x, y, z) for (x, y) in ((0, 0), (8, 23), (8, 24), (17, 18), (17, 19), (36, 28)) for z in (0, 1, 30, 31, 32)]   # columns 255 | 256 and 511 | 512
    forced += [(36, 28, z) for z in range(33)] + [(36, y, 32) for y in range(29)]
    ids = np.r_[ids, np.array(forced)]
    pts = (np.array(ODD["origin"]) + (ids + 0.5) * 0.25).astype(np.float32)    # exact in float32: every point is its voxel's centre
    dm.insert_cloud(pts); om.insert_cloud(pts)
    whole = om.local_cloud(None)
    assert len(whole) == len(np.unique(ids, axis=0)) > 300
    for cap in (solver.CORRIDOR_MAX_POINTS, len(whole), len(whole) - 1, 97):
        view = dm.shared_view_device(cap=cap, cell=0.5)
        assert view.dims == (19, 15, 17)
        view.update()
        n, total = _counts(view)
        assert total == len(whole) and n == min(cap, total) and bool(view.overflowed().item()) == (cap < total)
        assert np.array_equal(view.cloud[:n].cpu().numpy(), whole[:n])
        _same_grid(view, solver.CloudGrid(view.cloud[:n].contiguous(), 0.5, origin=dm.origin, dims=view.dims), n)


@pytest.mark.parametrize("mode", ["tile", "list", "cloud"])
def test_every_point_count_regime_under_an_active_cut_through_the_view(mode):
    """The regimes of tests/test_gpu_corridor_cut.py with P = the view's capacity (LDS masks, round bound, first density guess) and the
    count on the device: the per-planner route's bits."""
    om, cloud, ref, yaw, E, counts = _dense(mode)
    lo, hi = {"tile": (1280, 2048), "list": (2048, 8192), "cloud": (8192, 1 << 30)}[mode]
    assert all(lo < n <= hi for n in counts), (mode, counts)
    radius = (1.5, 3.0, 3.0)
    dm = solver.OccupancyMap(local_radius=radius, **GEO)
    dm.insert_cloud(cloud)
    c = ref[:, 0].copy()
    want = [om.local_cloud(x) for x in c]
    whole = om.local_cloud(None)
    assert all(len(w_) < len(whole) for w_ in want)                             # the cut is active
    view = dm.shared_view_device()
    view.update()
    assert _counts(view) == (len(whole), len(whole))
    boxes = dm.local_view(c, 0)
    a = _per_planner(want, ref, yaw, E)
    _same(a, _run_view(view, ref, yaw, E, cut=dm.cut(boxes.local_box)), mode)
    # a capacity near the real count: the same again
    tight = dm.shared_view_device(cap=len(whole) + 1)
    tight.update()
    _same(a, _run_view(tight, ref, yaw, E, cut=dm.cut(boxes.local_box)), mode + ", tight capacity")


def test_a_smaller_update_leaves_no_stale_point_in_reach():
    import torch
    om, cloud, ref, yaw, E, _ = _dense("cloud")
    radius = (1.5, 3.0, 3.0)
    dm = solver.OccupancyMap(local_radius=radius, **GEO)
    dm.insert_cloud(cloud)
    view = dm.shared_view_device()
    view.update()
    n1, _ = _counts(view)
    dm.clear_box((-2.0, -1.2, -0.5), (5.0, 3.0, 2.5))                           # most of it: y >= -1.2 of a world that spans [-2.2, 2.2]
    view.update()
    n2, t2 = _counts(view)
    assert 500 < n2 == t2 < n1 // 2
    assert (view.cloud[n2:n1] != 0).any()                                       # the tail of the first update is still there
    c = ref[:, 0].copy()
    cut = dm.cut(dm.local_view(c, 0).local_box)
    fresh = dm.shared_view_device()
    fresh.update()
    assert _counts(fresh) == (n2, n2) and torch.equal(fresh.cloud[:n2], view.cloud[:n2])
    want = _run_view(fresh, ref, yaw, E, cut=cut)
    lv = dm.local_view(c, n2)
    _same(want, _run(lv.cloud, ref, yaw, E, count=lv.cloud_count), "per-planner clouds of the cleared map")
    _same(want, _run_view(view, ref, yaw, E, cut=cut), "stale tail")
    view.cloud[n2:].fill_(float("nan")); view.grid.points[n2:].fill_(float("nan"))
    _same(want, _run_view(view, ref, yaw, E, cut=cut), "NaN tail")
    decoy = _up(ref.reshape(-1, 3) + np.array([0.0, 0.15, 0.0]))                 # points beside the stage references: in every box, closest of all
    k = view.cap - n2
    tail = decoy.repeat((k + len(decoy) - 1) // len(decoy), 1)[:k]
    view.cloud[n2:].copy_(tail); view.grid.points[n2:].copy_(tail)
    _same(want, _run_view(view, ref, yaw, E, cut=cut), "decoy tail")
    seen = view.cloud[:n2 + len(decoy)].contiguous()                            # ... and they would matter if a kernel looked at them
    differs = _run(seen, ref, yaw, E, cut=cut)
    assert any(not np.array_equal(x, y) for x, y in zip(want, differs))


def test_an_empty_map_gives_an_empty_view_and_the_box_rows():
    import torch
    B = 4
    dm, om, ref, yaw, E, c = _tunnel_world(61, B)
    view = dm.shared_view_device()
    view.update()
    assert _counts(view)[0] > 0
    dm.reset()
    view.update()
    assert _counts(view) == (0, 0) and not bool(view.overflowed().item())
    assert not view.grid.start.any()
    cut = dm.cut(dm.local_view(c, 0).local_box)
    empty = torch.zeros((0, 3), dtype=torch.float64, device=DEV)
    for k in (cut, None):
        a = _run_view(view, ref, yaw, E, cut=k)
        _same(a, _run(empty, ref, yaw, E, cut=k), "empty cloud")
        A, b, nf, pi, cnt = a
        assert (cnt >= 1).all() and all((nf[p][:cnt[p]] == 6).all() for p in range(B))


def test_overflow_keeps_the_first_points_and_writes_nothing_beyond_the_capacity():
    import torch
    dm = solver.OccupancyMap(**GEO); om = OO.OccMapOracle(**GEO)
    x, y, z = np.meshgrid(np.arange(200), np.arange(200), np.array([10, 11]), indexing="ij")
    ids = np.c_[x.ravel(), y.ravel(), z.ravel()]
    pts = (np.array(GEO["origin"]) + (ids + 0.5) * 0.1).astype(np.float32)
    dm.insert_cloud(pts)
    om.buffer[:, :, 10:12] = om.clamp_max_log                                   # (the oracle's insert is a Python loop per point)
    assert np.array_equal(dm.occ.cpu().numpy(), om.occ())
    whole = om.local_cloud(None)
    assert len(whole) == 80000
    view = dm.shared_view_device()
    view.update()
    assert _counts(view) == (solver.CORRIDOR_MAX_POINTS, 80000) and bool(view.overflowed().item())
    assert np.array_equal(view.cloud.cpu().numpy(), whole[:solver.CORRIDOR_MAX_POINTS])
    cap, more = 1000, 1500
    small = dm.shared_view_device(cap=cap)
    big = torch.full((more, 3), float(POISON), dtype=torch.float64, device=DEV)
    big_pts = torch.full((more, 3), float(POISON), dtype=torch.float64, device=DEV)
    big_idx = torch.full((more,), POISON, dtype=torch.int32, device=DEV)
    small.cloud, small.grid.points, small.grid.index = big[:cap], big_pts[:cap], big_idx[:cap]
    small.update()
    assert _counts(small) == (cap, 80000) and bool(small.overflowed().item())
    assert np.array_equal(big[:cap].cpu().numpy(), whole[:cap])
    assert (big[cap:] == POISON).all() and (big_pts[cap:] == POISON).all() and (big_idx[cap:] == POISON).all()
    _same_grid(small, solver.CloudGrid(big[:cap], 0.5, origin=dm.origin, dims=small.dims), cap)


def _padded_points(cloud, P):
    pts = np.full((P, 3), np.nan, dtype=np.float32)                             # a NaN point is outside the map: dropped by insert_cloud
    pts[:len(cloud)] = cloud
    return pts


def test_insert_update_boxes_and_corridor_captured_into_one_graph():
    """insert_cloud from a device buffer -> view.update -> local_view(c, 0) -> corridor through the view, captured on a side stream:
    the capture succeeding shows that nothing synchronises or allocates; a replay on another world gives that world's eager result."""
    import torch
    B = 16
    dm1, om1, ref, yaw, E, c = _tunnel_world(62, B)
    dm2, om2, _, _, _, _ = _tunnel_world(63, B)
    clouds = [tunnel_inputs(62, B)[0], tunnel_inputs(63, B)[0]]                 # _tunnel_world's float32 clouds, draw for draw
    N, F = ref.shape[1], 64
    d_ref, d_yaw, d_E, d_c = _up(ref), _up(yaw), _up(E), _up(c)
    eager = []
    for dm, om, cl in ((dm1, om1, clouds[0]), (dm2, om2, clouds[1])):
        view = dm.shared_view_device(); view.update()
        assert _counts(view)[0] == len(om.local_cloud(None))                     # the rebuilt cloud here is the world's
        eager.append(_run_view(view, ref, yaw, E, cut=dm.cut(dm.local_view(d_c, 0).local_box)))
    assert any(not np.array_equal(x, y) for x, y in zip(*eager))
    dm = solver.OccupancyMap(local_radius=dm1.local_radius, **GEO)
    pts = _up(_padded_points(clouds[0], 6000), np.float32)
    view = dm.shared_view_device()
    boxes = dm.local_view(d_c, 0)
    out = _outputs(B, N, F)

    def step():
        dm.insert_cloud(pts)
        view.update()
        dm.local_view(d_c, 0, out=boxes)
        solver.corridor_batch_device(None, d_ref, d_yaw, d_E, *out, view=view, cut=dm.cut(boxes.local_box))

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        step()                                                                   # warm-up on the capture stream
    side.synchronize()
    _same([t.cpu().numpy() for t in out], eager[0], "eager step")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    for k in (1, 0):
        dm.reset()
        pts.copy_(_up(_padded_points(clouds[k], 6000), np.float32))
        for t in out:
            t.fill_(POISON)
        boxes.local_box.fill_(POISON); view.count.fill_(POISON); view.total.fill_(POISON)
        torch.cuda.synchronize()
        g.replay(); torch.cuda.synchronize()
        _same([t.cpu().numpy() for t in out], eager[k], f"replay on world {k}")
        assert _counts(view)[0] == len((om1, om2)[k].local_cloud(None))


def test_fleet_full_tick_through_the_view_equals_the_shared_view_route():
    import torch
    B, N, K = 16, 20, 200
    dm, om, ref, yaw, E, c0 = _tunnel_world(64, B)
    s = np.arange(K) * 0.05 * 0.4
    path = np.c_[s, 0.4 * np.sin(0.8 * s), 1.0 + 0.1 * np.cos(s)]
    rng = np.random.default_rng(5)
    plan = np.zeros((B, N + 1, 17)); plan[..., 3] = 7.3; plan[..., 7] = 7.3
    plan[..., 8:11] = path[0] + rng.normal(0, 0.02, (B, 1, 3)); plan[..., 16] = 0.2
    fext = _up(rng.normal(0, 0.5, (B, 3))); d_path = _up(path)
    shared, grid = dm.shared_view()
    results = []
    for route in ("shared_view", "view"):
        fleet = solver.DeviceFleet(B, N, 30, 64, L.MODEL_NORMAL, (15.0, 3.0, 80.0, 15.0, 0.0))
        fleet.mpc_output.copy_(_up(plan)); fleet.solver.exitflag.fill_(1)
        toff = torch.zeros((B,), dtype=torch.float64, device=DEV)
        rp = torch.zeros((B, N, 3), dtype=torch.float64, device=DEV); ry = torch.zeros((B, N), dtype=torch.float64, device=DEV)
        view = dm.shared_view_device()
        ticks = []
        for tick in range(2):
            centres = fleet.mpc_output[:, 1, 8:11].contiguous()
            boxes = dm.local_view(centres, 0)
            if route == "shared_view":
                fleet.full_tick(fext, d_path, toff, shared, rp, ry, grid=grid, cut=dm.cut(boxes.local_box))
            else:
                view.update()
                fleet.full_tick(fext, d_path, toff, None, rp, ry, view=view, cut=dm.cut(boxes.local_box))
            torch.cuda.synchronize()
            toff += 0.05
            ticks.append([t.cpu().numpy().copy() for t in (fleet.mpc_output, fleet.solver.exitflag, fleet.poly_A, fleet.poly_b, fleet.poly_nfaces,
                                                           fleet.poly_index, fleet.poly_count)])
        results.append(ticks)
    for tick in range(2):
        for x, y in zip(results[0][tick], results[1][tick]):
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), tick
    assert all((results[0][tick][6] != 0).all() for tick in range(2))          # every planner got its polytopes in both ticks


def test_the_perception_loop_in_miniature():
    """Two ticks of render_depth (2 frames of 48 x 64 of the small pillars world) -> fuse_depth_batch into an empty belief map ->
    view.update -> corridor through the view: after each tick the corridor of shared_view() on the same belief map, and the belief
    grows.  One hit marks a voxel (prob_hit_log 3.0 from clamp_min_log -1.0 passes min_occupancy_log 1.7) and a miss does not unmark
    it (2.0 - 0.1), so the second tick's other poses can only add."""
    import torch
    image, height = "large", "low"
    rows, cols = RC.IMAGES[image]
    world = solver.OccupancyMap(world=RC.world("pillars", height), **FO.LAUNCH_CLAMPS)
    belief = solver.OccupancyMap(local_radius=(1.2, 1.5, 1.0), **RC.GEO[height], **FO.LAUNCH_CLAMPS)
    view = belief.shared_view_device(cap=20000, cell=0.5)
    B, N = 4, 6
    rng = np.random.default_rng(11)
    s = np.linspace(-0.6, 0.6, N)
    ref = np.c_[s, 1.0 + 0.2 * np.sin(s), np.full(N, 1.0)][None] + rng.normal(0, 0.02, (B, N, 3))
    yaw = rng.normal(0.1, 0.05, (B, N))
    E = np.tile(np.diag([0.1, 0.1, 0.05]), (B, N, 1, 1))
    c = _up(ref[:, 0].copy())
    ticks = [["middle", "near_face"], [RC.OUTSIDE, "middle"]]                    # the second tick looks in from outside the -x face
    counts = []
    for keys in ticks:
        T = np.stack([RC.pose_of(k) for k in keys])
        depth = world.render_depth(T, RC.K[image], rows, cols, max_range=RC.MAX_RANGE)
        belief.fuse_depth_batch(depth, RC.K[image], T, prob_hit_log=3.0, prob_miss_log=-0.1)
        view.update()
        cut = belief.cut(belief.local_view(c, 0).local_box)
        a = _run_view(view, ref, yaw, E, cut=cut)
        n, total = _counts(view)
        assert n == total == int(belief.occ.sum().item())
        shared, grid = belief.shared_view(cell=0.5)
        assert torch.equal(view.cloud[:n], shared)
        _same(a, _run(shared, ref, yaw, E, grid=grid, cut=cut), f"tick {len(counts)}")
        counts.append(n)
    print("belief points per tick:", counts)
    assert 50 < counts[0] < counts[1]
