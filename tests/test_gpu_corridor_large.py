"""GPU tests of the shared-cloud route beyond FRP_CORRIDOR_MAX_POINTS (include/frp_nmpc_corridor_large.h; solver.SharedView with
cap > CORRIDOR_MAX_POINTS and view= of corridor_batch_device / DeviceFleet).  The oracle for polytopes is ROUTE 1 on the same map --
OccupancyMap.local_view(centres, P) + frp_nmpc_corridor_batch on per-planner clouds, code this feature does not touch -- and the
comparison is bit for bit on all five outputs, with poisoned output buffers.  The view's cloud is held against tests/occmap_oracle.py.

The world: a 96 x 96 x 32 map at 0.1 m with a solid block (x < 3.0 m), a 0.4 m wall and a few isolated voxels.  Which kernel a planner
ends in is decided by two counts (frp_corridor.hip, frp_corridor_wave.inc): more than 448 points inside a SEED ellipsoid make the
one-wavefront kernel hand the planner on, and more than 8192 points in a local box make the grid kernel hand it on to the new
fallback.  seed_len = 2 m (a seed sphere of radius 1 m) and the placements below fix both counts, and the tests assert them, stage
by stage, from the occupancy oracle's clouds."""
import ctypes
import functools

import numpy as np
import pytest

from forces_resilient_planner_amd import layout as L, solver
from tests import occmap_oracle as OO
from tests.test_gpu_corridor_cut import POISON, _outputs, _run, _same, _up, dense_counts, DENSE
from tests.test_gpu_occmap import GEO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 20
CONSTS = dict(bbox=(1.5, 1.5, 1.0), seed_len=2.0)
WAVE_TILE, GRID_LIST, REG_TILE = 448, 8192, 1280      # CW_CAP, CR_LIST, CR_TILE * CR_THREADS
INT_MIN = -2 ** 31


def _world(gx=96, block=30, wall=True, radius=(3.0, 3.0, 1.6), res=0.1, gy=96, gz=32, sprinkles=60):
    """(device map, oracle map) of a solid block x < block voxels, the wall and the isolated voxels."""
    geo = dict(origin=(0.0, 0.0, 0.0), map_size=((gx - 0.5) * res, (gy - 0.5) * res, (gz - 0.5) * res), resolution=res)   # (ceil(size / res) voxels)
    occ = np.zeros((gx, gy, gz), dtype=bool)
    occ[:block] = True
    if wall:
        occ[70:74, 20:80, :] = True
    rng = np.random.default_rng(3)
    if sprinkles:
        occ[rng.integers(block + 7, block + 33, sprinkles), rng.integers(0, gy, sprinkles), rng.integers(0, gz, sprinkles)] = True
    dm = solver.OccupancyMap(local_radius=radius, **geo); om = OO.OccMapOracle(local_radius=radius, **geo)
    assert dm.grid == (gx, gy, gz)
    ids = np.argwhere(occ)
    dm.insert_cloud((ids + 0.5).astype(np.float64) * res)
    om.buffer[occ] = om.clamp_max_log
    assert np.array_equal(dm.occ.cpu().numpy(), om.occ())
    return dm, om


def _planners(starts):
    """ref [B,N,3], yaw [B,N], E for planners that creep 2 cm per stage along their heading from (x, y, z, yaw)."""
    s = np.asarray(starts, dtype=np.float64)
    step = 0.02 * np.arange(N)[None, :, None]
    d = np.stack([np.cos(s[:, 3]), np.sin(s[:, 3]), np.zeros(len(s))], 1)
    ref = s[:, None, :3] + step * d[:, None, :]
    yaw = np.repeat(s[:, 3:4], N, 1)
    E = np.tile(np.diag([0.1, 0.1, 0.05]), (len(s), N, 1, 1))
    return ref, yaw, E


def _box_counts(vis, ref_p, yaw_p, consts=CONSTS):
    """Per stage: (points of `vis` in the local box of a decomposition seeded there, those inside its seed sphere)."""
    bb, sl = consts["bbox"], consts["seed_len"]
    out = []
    for p1, y in zip(ref_p, yaw_p):
        d = np.array([np.cos(y), np.sin(y), 0.0]); dh = np.array([d[1], -d[0], 0.0]); dv = np.cross(d, dh)
        e = vis - p1
        h, t, v = e @ dh, e @ d, e @ dv
        inb = (np.abs(h) <= bb[1]) & (t >= -bb[0]) & (t <= sl + bb[0]) & (np.abs(v) <= bb[2])
        ins = inb & (((vis - (p1 + d * sl / 2)) ** 2).sum(1) <= (sl / 2) ** 2)
        out.append((int(inb.sum()), int(ins.sum())))
    return np.array(out).reshape(-1, 2)


HALF = np.pi / 2
# (x, y, z, yaw): 0-1 free space (one-wavefront kernel), 2-3 beside the wall (grid kernel), 4-6 beside the block (the new fallback),
# 7 outside the map (an empty cut row, min > max)
STARTS = [(5.013, 3.021, 1.57, HALF + 0.03), (5.107, 5.513, 1.33, HALF - 0.05),
          (6.553, 2.531, 1.61, HALF + 0.02), (6.521, 3.017, 1.43, HALF - 0.04),
          (3.3537, 2.523, 1.59, HALF + 0.03), (3.4011, 4.017, 1.27, HALF - 0.06), (3.3279, 6.541, 1.81, -HALF + 0.05),
          (30.0, 5.0, 1.6, 0.1)]
WAVE, GRID, FALLBACK, EMPTY = (0, 1), (2, 3), (4, 5, 6), (7,)


@functools.lru_cache(maxsize=None)
def _main_case():
    """The world, the planners, the per-planner visible clouds of the oracle, and ROUTE 1's result -- computed once, never modified."""
    dm, om = _world()
    ref, yaw, E = _planners(STARTS)
    c = ref[:, 0].copy()
    whole = om.local_cloud(None)
    vis = [om.local_cloud(x) for x in c]
    assert 70000 <= len(whole) <= 120000 and len(whole) > solver.CORRIDOR_MAX_POINTS
    assert max(len(v) for v in vis) < solver.CORRIDOR_MAX_POINTS and all(len(v) < len(whole) for v in vis)   # route 1 can hold them; the cut is active
    counts = [_box_counts(v, ref[p], yaw[p]) for p, v in enumerate(vis)]
    print("whole map", len(whole), "local views", [len(v) for v in vis])
    print("in-box / in-seed counts, stage 0 .. last:", [(k[0].tolist(), k[-1].tolist()) for k in counts])
    for p in WAVE:      # never more than the one-wavefront kernel's tile in a seed ellipsoid: it finishes the planner itself
        assert counts[p][:, 0].max() < 200 and counts[p][:, 1].max() < WAVE_TILE // 4
    for p in GRID:      # handed on by the one-wavefront kernel at stage 0, finished by the grid kernel: a box never holds more than its list
        assert counts[p][0, 1] > WAVE_TILE + 100 and REG_TILE < counts[p][:, 0].min() and counts[p][:, 0].max() < GRID_LIST - 500
    for p in FALLBACK:  # handed on twice: the stage-0 box holds more than the grid kernel's list, and no box more than the fallback's
        assert counts[p][0, 1] > WAVE_TILE + 100 and counts[p][0, 0] > GRID_LIST + 500 and counts[p][:, 0].max() < solver.CORRIDOR_LARGE_LIST
    for p in EMPTY:
        box = om.local_box(c[p])
        assert box[0] > box[3] and len(vis[p]) == 0
    lv = dm.local_view(c, solver.CORRIDOR_MAX_POINTS)
    assert [int(n) for n in lv.cloud_count.cpu().numpy()] == [len(v) for v in vis]
    want = _run(lv.cloud, ref, yaw, E, count=lv.cloud_count, consts=CONSTS)
    assert (want[4][list(WAVE + GRID + FALLBACK)] >= 1).all() and (want[2][list(EMPTY), 0] == 6).all()
    return dm, om, ref, yaw, E, c, whole, want


def _counts(view):
    import torch
    torch.cuda.synchronize()
    return int(view.count.item()), int(view.total.item())


def _run_view(view, ref, yaw, E, cut=None, consts=CONSTS):
    import torch
    B = ref.shape[0]
    out = _outputs(B, N, 64)
    if view.overflow is not None:
        view.overflow.fill_(POISON)
    solver.corridor_batch_device(None, _up(ref), _up(yaw), _up(E), *out, view=view, cut=cut, consts=consts)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _run_large_raw(view, ref, yaw, E, cut=None, consts=CONSTS, with_count=True, P=None):
    """frp_nmpc_corridor_batch_large called directly on a view's buffers (any capacity; the device count or none).  Returns the five
    outputs and overflow [B]."""
    import torch
    B, N = ref.shape[:2]
    out = _outputs(B, N, 64)
    c = dict(solver.CORRIDOR_DEFAULTS); c.update(consts or {})
    d_ref, d_yaw, d_E = _up(ref), _up(yaw), _up(E)
    g = view.grid
    cr = solver.Corridor(B, N, 64, view.cap if P is None else P, view.cloud.data_ptr(), 0, view.count.data_ptr() if with_count else None,
                         d_ref.data_ptr(), d_yaw.data_ptr(), d_E.data_ptr(), (ctypes.c_double * 3)(*c["bbox"]), c["seed_len"], c["inflation"],
                         c["offset_x"], out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr())
    cr.grid_origin = (ctypes.c_double * 3)(*g.origin); cr.grid_cell = g.cell; cr.grid_dims = (ctypes.c_int * 3)(*g.dims)
    cr.grid_points = g.points.data_ptr(); cr.grid_index = g.index.data_ptr(); cr.grid_start = g.start.data_ptr()
    ws = torch.zeros((solver.lib().frp_nmpc_corridor_large_workspace_bytes(B),), dtype=torch.uint8, device=DEV)
    ov = torch.full((B,), POISON, dtype=torch.int32, device=DEV)
    w = solver.CorridorLarge(ws.data_ptr(), ws.numel(), ov.data_ptr())
    rc = solver.lib().frp_nmpc_corridor_batch_large(ctypes.byref(cr), ctypes.byref(cut) if cut is not None else None, ctypes.byref(w),
                                                    ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out], ov.cpu().numpy()


def test_large_view_equals_the_whole_map_cloud():
    import torch
    dm, om, ref, yaw, E, c, whole, want = _main_case()
    total = len(whole)
    for cap in (131072, total, total - 1):
        view = dm.shared_view_device(cap=cap, cell=0.5, planners=8)
        assert view.large and view.dims == (20, 20, 7)
        for t in (view.cloud, view.grid.points):
            t.fill_(float("nan"))                                               # poisoned buffers: nothing beyond the count is written
        view.grid.index.fill_(POISON); view.count.fill_(POISON); view.total.fill_(POISON)
        view.update()
        n, tot = _counts(view)
        assert tot == total and n == min(cap, total) and bool(view.overflowed().item()) == (cap < total)
        assert np.array_equal(view.cloud[:n].cpu().numpy(), whole[:n])           # x, y, z order, bit for bit; on overflow the first cap points
        assert torch.isnan(view.cloud[n:]).all() and torch.isnan(view.grid.points[n:]).all() and (view.grid.index[n:] == POISON).all()
        start, index = view.grid.start.cpu().numpy(), view.grid.index.cpu().numpy()[:n]
        assert start[0] == 0 and start[-1] == n and (np.diff(start) >= 0).all() and np.array_equal(np.sort(index), np.arange(n))
        assert np.array_equal(view.grid.points.cpu().numpy()[:n], whole[index])
        cell = np.repeat(np.arange(len(start) - 1), np.diff(start))
        ix = np.minimum(np.floor(whole[index] / 0.5).astype(int), np.array(view.dims) - 1)
        assert np.array_equal(cell, (ix[:, 2] * view.dims[1] + ix[:, 1]) * view.dims[0] + ix[:, 0])


@pytest.mark.parametrize("cap", ["131072", "total"])
def test_corridor_through_the_large_view_equals_route_1_with_the_cut(cap):
    dm, om, ref, yaw, E, c, whole, want = _main_case()
    view = dm.shared_view_device(cap=131072 if cap == "131072" else len(whole), cell=0.5, planners=8)
    view.update()
    assert _counts(view) == (len(whole), len(whole))
    cut = dm.cut(dm.local_view(c, 0).local_box)
    a = _run_view(view, ref, yaw, E, cut=cut)
    _same(want, a, "large view, device count")
    assert np.array_equal(view.overflow.cpu().numpy(), np.zeros(8, dtype=np.int32))
    if cap == "total":                                                           # cloud_count = NULL: P points are live
        b, ov = _run_large_raw(view, ref, yaw, E, cut=cut, with_count=False)
        _same(want, b, "large entry, no count")
        assert not ov.any()
    else:                                                                        # a NaN tail, then a decoy tail beyond the count: out of reach
        n = len(whole)
        view.cloud[n:].fill_(float("nan")); view.grid.points[n:].fill_(float("nan"))
        _same(want, _run_view(view, ref, yaw, E, cut=cut), "NaN tail")
        decoy = _up(ref.reshape(-1, 3) + np.array([0.0, 0.15, 0.0]))
        k = view.cap - n
        tail = decoy.repeat((k + len(decoy) - 1) // len(decoy), 1)[:k]
        view.cloud[n:].copy_(tail); view.grid.points[n:].copy_(tail)
        _same(want, _run_view(view, ref, yaw, E, cut=cut), "decoy tail")


def test_corridor_without_a_cut_on_a_map_whose_local_views_are_the_whole_map():
    """cut = NULL: every planner sees the whole cloud.  Route 1 can say the same only where a local view IS the whole map (and holds at
    most 65 536 points): a 64 x 96 x 32 map with a 2 m block and a local radius beyond the map."""
    dm, om = _world(gx=64, block=20, wall=False, radius=(20.0, 20.0, 20.0))
    starts = [(2.3537, 2.523, 1.59, HALF + 0.03), (2.4011, 4.017, 1.27, HALF - 0.06), (2.3279, 6.541, 1.81, -HALF + 0.05),
              (4.613, 3.021, 1.57, HALF + 0.03), (4.707, 5.513, 1.33, HALF - 0.05)]
    ref, yaw, E = _planners(starts)
    c = ref[:, 0].copy()
    whole = om.local_cloud(None)
    assert 60000 < len(whole) <= solver.CORRIDOR_MAX_POINTS
    for p, x in enumerate(c):
        assert np.array_equal(om.local_cloud(x), whole)                          # no box is cut
        k = _box_counts(whole, ref[p], yaw[p])
        if p < 3:
            assert k[0, 1] > WAVE_TILE + 100 and k[0, 0] > GRID_LIST + 500 and k[:, 0].max() < solver.CORRIDOR_LARGE_LIST
        else:
            assert k[:, 0].max() < 200
    lv = dm.local_view(c, solver.CORRIDOR_MAX_POINTS)
    want = _run(lv.cloud, ref, yaw, E, count=lv.cloud_count, consts=CONSTS)
    view = dm.shared_view_device(cap=131072, cell=0.5, planners=5)
    view.update()
    assert _counts(view) == (len(whole), len(whole))
    _same(want, _run_view(view, ref, yaw, E, cut=None), "no cut, device count")
    tight = dm.shared_view_device(cap=len(whole), cell=0.5, planners=5)          # (at or below the old limit: filled by the existing update)
    tight.update()
    b, ov = _run_large_raw(tight, ref, yaw, E, cut=None, with_count=False)
    _same(want, b, "no cut, no count")
    assert not ov.any()


def test_at_or_below_the_old_limit_nothing_differs():
    """The surface map of tests/test_gpu_occmap_shared_view.py's "cloud" regime (more than 8192 points in the boxes): the large entries at
    cap = 65 536 against the existing ones, bit for bit."""
    import torch
    om, cloud, ref, yaw, E, counts = dense_counts(*DENSE["cloud"])
    dm = solver.OccupancyMap(local_radius=(1.5, 3.0, 3.0), **GEO)
    dm.insert_cloud(cloud)
    old = dm.shared_view_device()
    old.update()
    new = dm.shared_view_device()
    assert new.cap == solver.CORRIDOR_MAX_POINTS and not new.large and new.overflow is None
    a = new._args()
    dm._call("frp_nmpc_occmap_shared_view_update_large", ctypes.byref(a))
    n, total = _counts(new)
    assert (n, total) == _counts(old) and n == len(om.local_cloud(None))
    assert torch.equal(new.cloud[:n], old.cloud[:n]) and torch.equal(new.grid.start, old.grid.start)
    cut = dm.cut(dm.local_view(ref[:, 0].copy(), 0).local_box)
    for k in (cut, None):
        B = ref.shape[0]
        out = _outputs(B, ref.shape[1], 64)
        solver.corridor_batch_device(None, _up(ref), _up(yaw), _up(E), *out, view=old, cut=k)
        torch.cuda.synchronize()
        want = [t.cpu().numpy() for t in out]
        got, ov = _run_large_raw(new, ref, yaw, E, cut=k, consts=None)
        _same(want, got, "large entry at cap = 65536")
        assert not ov.any()


def test_update_and_corridor_captured_into_a_graph_and_replayed_after_the_map_changed():
    import torch
    dm, om = _world()
    ref, yaw, E = _planners(STARTS)
    c = ref[:, 0].copy()
    cutbox = dm.local_view(c, 0).local_box
    d_ref, d_yaw, d_E = _up(ref), _up(yaw), _up(E)

    def eager():
        v = dm.shared_view_device(cap=131072, cell=0.5, planners=8)
        v.update()
        return _run_view(v, ref, yaw, E, cut=dm.cut(cutbox)), _counts(v)

    first, n1 = eager()
    view = dm.shared_view_device(cap=131072, cell=0.5, planners=8)
    out = _outputs(8, N, 64)

    def step():
        view.update()
        solver.corridor_batch_device(None, d_ref, d_yaw, d_E, *out, view=view, cut=dm.cut(cutbox), consts=CONSTS)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        step()                                                                   # warm-up on the capture stream
    side.synchronize()
    _same([t.cpu().numpy() for t in out], first, "eager step")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                                       # succeeds: nothing in the two calls synchronises or allocates
        step()
    dm.clear_box((2.0, 2.0, 0.0), (3.0, 5.0, 3.2))                               # a bite out of the block's face, beside planners 4 and 5
    second, n2 = eager()
    assert n2[0] < n1[0] and any(not np.array_equal(x, y) for x, y in zip(first, second))
    for t in out:
        t.fill_(POISON)
    view.count.fill_(POISON); view.total.fill_(POISON); view.overflow.fill_(POISON)
    torch.cuda.synchronize()
    g.replay(); torch.cuda.synchronize()
    _same([t.cpu().numpy() for t in out], second, "replay on the changed map")
    assert _counts(view) == n2 and not view.overflow.cpu().numpy().any()


def test_a_box_beyond_the_fallback_list_is_refused_and_the_other_planners_are_unaffected():
    """128 x 128 x 64 voxels of 0.05 m, the half x < 3.2 m solid: the box of the planner 0.35 m from the face holds more than 65 536
    points."""
    dm, om = _world(gx=128, block=64, wall=False, res=0.05, gy=128, gz=64, sprinkles=0)
    whole = om.local_cloud(None)
    assert len(whole) == 64 * 128 * 64
    starts = [(3.5537, 1.523, 1.59, HALF + 0.03),                                # 0: refused
              (3.9011, 1.517, 2.87, HALF - 0.02), (3.9279, 4.941, 2.91, -HALF + 0.05),   # 1-2: the fallback, fitting its list
              (5.213, 1.021, 1.57, HALF + 0.03)]                                 # 3: free space
    ref, yaw, E = _planners(starts)
    k = [_box_counts(whole, ref[p], yaw[p]) for p in range(4)]
    print("in-box / in-seed counts at stage 0:", [x[0].tolist() for x in k])
    assert k[0][0, 0] > solver.CORRIDOR_LARGE_LIST + 2000 and k[0][0, 1] > WAVE_TILE + 100
    for p in (1, 2):
        assert k[p][0, 1] > WAVE_TILE + 100 and k[p][0, 0] > GRID_LIST + 500 and k[p][:, 0].max() < solver.CORRIDOR_LARGE_LIST - 2000
    assert k[3][:, 0].max() == 0
    view = dm.shared_view_device(cap=len(whole), cell=0.5, planners=4)
    view.update()
    assert _counts(view) == (len(whole), len(whole))
    a = _run_view(view, ref, yaw, E)
    A, b, nf, pi, cnt = a
    assert view.overflow.cpu().numpy().tolist() == [1, 0, 0, 0]
    assert cnt[0] == INT_MIN and not nf[0].any() and not pi[0].any()            # the documented marker
    rest = _run_view(view, ref[1:], yaw[1:], E[1:])
    assert view.overflow[:3].cpu().numpy().tolist() == [0, 0, 0] and (rest[4] >= 1).all()
    _same([x[1:] for x in a], rest, "the batch without the refused planner")


def test_fleet_full_tick_through_the_large_view_equals_route_1():
    import torch
    B, K = 8, 200
    dm, om, _, _, _, _, whole, _ = _main_case()
    s = np.arange(K) * 0.05 * 0.4
    path = np.c_[3.3537 + 0.05 * np.sin(0.8 * s), 2.0 + s, 1.6 + 0.1 * np.cos(s)]   # along the block's face
    rng = np.random.default_rng(5)
    plan = np.zeros((B, N + 1, 17)); plan[..., 3] = 7.3; plan[..., 7] = 7.3
    plan[..., 8:11] = path[0] + rng.normal(0, 0.02, (B, 1, 3)); plan[..., 16] = HALF
    fext = _up(rng.normal(0, 0.5, (B, 3))); d_path = _up(path)
    results = []
    for route in ("per-planner clouds", "large view"):
        fleet = solver.DeviceFleet(B, N, 30, 64, L.MODEL_NORMAL, (15.0, 3.0, 80.0, 15.0, 0.0))
        fleet.mpc_output.copy_(_up(plan)); fleet.solver.exitflag.fill_(1)
        toff = torch.zeros((B,), dtype=torch.float64, device=DEV)
        rp = torch.zeros((B, N, 3), dtype=torch.float64, device=DEV); ry = torch.zeros((B, N), dtype=torch.float64, device=DEV)
        view = dm.shared_view_device(cap=131072, cell=0.5, planners=B)
        ticks = []
        for tick in range(2):
            centres = fleet.mpc_output[:, 1, 8:11].contiguous()
            if route == "large view":
                view.update()
                fleet.full_tick(fext, d_path, toff, None, rp, ry, view=view, cut=dm.cut(dm.local_view(centres, 0).local_box), corridor_consts=CONSTS)
            else:
                lv = dm.local_view(centres, solver.CORRIDOR_MAX_POINTS)
                assert (lv.cloud_count >= 0).all()
                fleet.full_tick(fext, d_path, toff, lv.cloud, rp, ry, cloud_count=lv.cloud_count, corridor_consts=CONSTS)
            torch.cuda.synchronize()
            toff += 0.05
            ticks.append([t.cpu().numpy().copy() for t in (fleet.mpc_output, fleet.solver.exitflag, fleet.poly_A, fleet.poly_b, fleet.poly_nfaces,
                                                           fleet.poly_index, fleet.poly_count)])
            if route == "large view":
                assert not view.overflow.cpu().numpy().any()
                k = _box_counts(om.local_cloud(centres[0].cpu().numpy()), rp[0].cpu().numpy(), ry[0].cpu().numpy())
                print("tick", tick, "planner 0, in-box / in-seed counts at stage 0:", k[0].tolist())
        results.append(ticks)
    for tick in range(2):
        for x, y in zip(results[0][tick], results[1][tick]):
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), tick
    assert all((results[0][tick][6] > 0).all() for tick in range(2))
