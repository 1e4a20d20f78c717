"""GPU tests of point-scan fusion (include/frp_nmpc_occmap_fuse_points.h, solver.OccupancyMap.fuse_points) against the serial oracle
applied scan after scan (tests/occmap_fuse_points_cases.py on tests/occmap_fusion_oracle.py: FusionOracle.raycast over each scan's
points with the non-finite rows removed).  Everything compared is a double that both sides compute with the same IEEE operations, a
byte or an integer: equality is exact, nothing here has a tolerance.  Scans of at most 713 points on the 64 x 64 x 32 map;
tests/test_occmap_fuse_points_cpu.py checks that these inputs can tell a right implementation from a wrong one."""
import ctypes

import numpy as np
import pytest

from forces_resilient_planner_amd import solver
from tests import occmap_check_oracle as CO
from tests import occmap_fuse_points_cases as C
from tests import occmap_fusion_batch_cases as BC
from tests import occmap_fusion_oracle as FO

pytestmark = pytest.mark.gpu
FRP_ERR_ARG = -1003


def _device(poison=0xFF):
    """The oracle's start map on the device.  poison: the byte the fusion workspace is filled with before the first call."""
    import torch
    dm = solver.OccupancyMap(**FO.TEST_GEO, **FO.LAUNCH_CLAMPS)
    _reset(dm)
    if poison is not None:
        dm.fuse_points_ws = torch.full((32 << 20,), poison, dtype=torch.uint8, device=dm.device)   # larger than the calls of up to a dozen scans need: the method keeps it
    return dm


def _reset(dm):
    import torch
    dm.log_odds.copy_(torch.from_numpy(BC.start_values()).to(dm.device))
    dm.refresh()


def _assert_same(dm, om, what=""):
    """log_odds to the bit, occ, and the whole-map cloud of local_view -- which is read from the bit plane."""
    import torch
    torch.cuda.synchronize()
    assert dm.log_odds.cpu().numpy().tobytes() == om.buffer.tobytes(), what
    assert dm.occ.cpu().numpy().tobytes() == om.occ().astype(np.uint8).tobytes(), what
    want = om.local_cloud(None)
    assert 0 < len(want) <= solver.CORRIDOR_MAX_POINTS
    v = dm.local_view(None, len(want))
    torch.cuda.synchronize()
    assert int(v.cloud_count[0]) == len(want) and np.array_equal(v.cloud[0].cpu().numpy(), want), what


def _upload(dm, scans, dtype=np.float64, P=None, poisoned=True):
    import torch
    pts, count, origin = C.pack(scans, P=P)
    if poisoned:
        pts = C.poison(pts, count)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dm.device)
    return to(pts.astype(dtype)), to(count), to(origin)


def _fuse(dm, scans, dtype=np.float64, P=None, **kw):
    """The scans in one call, each with its own count, the storage beyond it poisoned.  Returns the status as a list."""
    pts, count, origin = _upload(dm, scans, dtype, P)
    return dm.fuse_points(pts, origin, count=count, **kw).cpu().numpy().tolist()


# ---- 1. realistic scans ----
@pytest.mark.parametrize("as_float", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("scene,placement", C.REALISTIC)
def test_one_realistic_scan(scene, placement, as_float):
    import torch
    pts, origin = C.realistic(scene, placement)
    om, status = C.realistic_chain(scene, placement, as_float)
    dm = _device()
    p = torch.from_numpy(pts.astype(np.float32 if as_float else np.float64)).to(dm.device)      # [P, 3] and [3]: one scan without its leading dimension
    st = dm.fuse_points(p, np.array(origin)).cpu().numpy().tolist()
    assert st == status and st[0][0] >= 2 and st[0][1] > 100, (st, status)
    _assert_same(dm, om, (scene, placement))


@pytest.mark.parametrize("as_float", [False, True], ids=["double", "float"])
def test_a_scan_that_rounding_to_float_changes(as_float):
    om, status = C.float_sensitive_chain(as_float)
    dm = _device()
    assert _fuse(dm, [C.float_sensitive()], np.float32 if as_float else np.float64) == status
    _assert_same(dm, om)
    assert dm.log_odds.cpu().numpy().tobytes() != C.float_sensitive_chain(not as_float)[0].buffer.tobytes()


def test_the_realistic_scans_as_one_batch():
    om, status = C.realistic_batch_chain()
    dm = _device()
    assert _fuse(dm, C.realistic_scans()) == status
    _assert_same(dm, om)


# ---- 2. same rays, two routes ----
def test_the_depth_route_and_the_point_route_agree():
    """fuse_depth_batch(frames) against fuse_points(project(frames), T[:3, 3]): the same rays in the same order through the existing
    kernel and through the new one, without the oracle's ray caster in between."""
    import torch
    frames = BC.six_frames()
    depth, T = BC.stack(frames)
    by_depth, by_points = _device(poison=None), _device()
    st_d = by_depth.fuse_depth_batch(depth, BC.K, T).cpu().numpy().tolist()
    st_p = _fuse(by_points, C.six_scans())
    torch.cuda.synchronize()
    assert st_p == st_d and all(s[0] >= 2 and s[1] > 100 for s in st_p), (st_p, st_d)
    assert by_points.log_odds.cpu().numpy().tobytes() == by_depth.log_odds.cpu().numpy().tobytes()
    assert by_points.occ.cpu().numpy().tobytes() == by_depth.occ.cpu().numpy().tobytes()
    words = by_depth.ws_bytes // 4                                                                   # the bit plane (the tensor has a word of padding behind it)
    assert by_points.ws[:words].cpu().numpy().tobytes() == by_depth.ws[:words].cpu().numpy().tobytes()
    assert by_points.log_odds.cpu().numpy().tobytes() != BC.start_values().tobytes()


# ---- 3. edge sets ----
@pytest.mark.parametrize("name", C.EDGE_NAMES)
def test_an_edge_set_alone(name):
    om, status = C.edge_chain(name)
    scan = C.edge_sets()[name]
    for tail in (300, 1):
        dm = _device(poison=0x5A)
        st = _fuse(dm, [scan], P=len(scan[0]) + tail)                                                 # count < P, the tail poisoned
        assert st == status, (name, st, status)
        _assert_same(dm, om, name)
    if name == "count 0":                                                                             # ... and no storage at all
        import torch
        dm = _device()
        st = dm.fuse_points(torch.zeros((1, 0, 3), dtype=torch.float64, device=dm.device), np.array([scan[1]])).cpu().numpy().tolist()
        assert st == [[1, 0]]
        _assert_same(dm, C.oracle(), "P = 0")


def test_the_result_does_not_depend_on_the_tail():
    import torch
    scan, origin = C.edge_sets()["count below P"]                                                    # the first 401 points of a scan of 670
    om, status = C.edge_chain("count below P")
    real = C.realistic("random", "middle")[0]
    count = np.array([len(scan)], dtype=np.int32)
    for tail in (None, C.POISON[0], C.POISON[3], 0.0):                                                # None: the rest of the real scan
        p = real.copy()[None]
        assert np.array_equal(p[0, :len(scan)], scan) and len(real) > len(scan) + 200
        if tail is not None:
            p[0, len(scan):] = tail
        dm = _device(poison=0x00)
        st = dm.fuse_points(torch.from_numpy(p).to(dm.device), np.array(origin), count=count).cpu().numpy().tolist()
        assert st == status, tail
        _assert_same(dm, om, tail)
    # ... and with count = None the whole capacity is the scan: another map
    full, status_full = C.realistic_chain("random", "middle", False)
    dm = _device()
    assert dm.fuse_points(torch.from_numpy(real.copy()[None]).to(dm.device), np.array(origin)).cpu().numpy().tolist() == status_full != status
    _assert_same(dm, full)


def test_the_edge_sets_as_one_batch():
    om, status = C.edge_batch_chain()
    scans = [C.edge_sets()[n] for n in C.EDGE_NAMES]
    dm = _device(poison=0xA5)
    assert _fuse(dm, scans) == status
    _assert_same(dm, om)
    # a count beyond the capacity is clamped to it, a negative one to 0
    import torch
    dm = _device()
    pts, count, origin = _upload(dm, scans, poisoned=False)
    k, full = C.EDGE_NAMES.index("count 0"), int(np.argmax([len(p) for p, _ in scans]))
    count[k] = -3; count[full] = 1 << 30
    assert dm.fuse_points(pts, origin, count=count).cpu().numpy().tolist() == status
    _assert_same(dm, om)


# ---- 4. order across scans ----
def test_the_scans_order_is_kept():
    fwd, st = C.order_chain(False)
    rev, _ = C.order_chain(True)
    dm = _device()
    assert _fuse(dm, C.order_scans()) == st
    _assert_same(dm, fwd)
    assert dm.log_odds.cpu().numpy().tobytes() != rev.buffer.tobytes()
    _reset(dm)
    assert _fuse(dm, C.order_scans()[::-1]) == st[::-1]
    _assert_same(dm, rev)


# ---- 5. status and containment ----
def test_inactive_and_refused_scans_stop_nothing():
    import torch
    scans = [C.realistic("wall", "middle"), C.realistic("random", "near_face"), C.realistic("steps", "middle")]
    om, status = C.chain(scans, skip={1})
    dm = _device()
    st = _fuse(dm, scans, active=np.array([1, 0, 1], dtype=np.int32))
    assert st == C.want(status) and st[1] == [0, 0], (st, status)
    _assert_same(dm, om)
    for bad in (float("nan"), float("inf"), -float("inf")):
        dm = _device()
        pts, count, origin = _upload(dm, scans)
        origin[1, 2] = bad
        st = dm.fuse_points(pts, origin, count=count).cpu().numpy().tolist()
        assert st == [status[0], [solver.OCCMAP_FUSE_REFUSED, 0], status[2]] and solver.OCCMAP_FUSE_REFUSED == -256, (st, status)
        _assert_same(dm, om, bad)
    # everything off: the map, occ and the bit plane are untouched
    dm = _device()
    torch.cuda.synchronize()
    before = (dm.log_odds.cpu().numpy().tobytes(), dm.occ.cpu().numpy().tobytes(), dm.ws.cpu().numpy().tobytes())
    assert _fuse(dm, scans, active=np.zeros(3, dtype=np.int32)) == [[0, 0]] * 3
    torch.cuda.synchronize()
    assert (dm.log_odds.cpu().numpy().tobytes(), dm.occ.cpu().numpy().tobytes(), dm.ws.cpu().numpy().tobytes()) == before


def test_a_scan_that_does_not_converge_is_left_out():
    om, status = C.cap_chain()
    dm = _device()
    st = _fuse(dm, C.cap_scans(), max_rounds=1)
    assert st == status and st[1][0] == -1 and st[1][1] > 100 and [s[0] for s in st] == [1, -1, 1, 1], (st, status)
    _assert_same(dm, om)
    # with the default cap it converges and the map is the full chain's
    full, status_full = C.chain(C.cap_scans())
    _reset(dm)
    assert _fuse(dm, C.cap_scans()) == status_full
    _assert_same(dm, full)


def test_64_scans_are_accepted_and_65_are_not():
    import torch
    om, status = C.many_chain(64)
    dm = _device()
    assert _fuse(dm, C.many_scans(64)) == status
    _assert_same(dm, om)
    # 65: FRP_ERR_ARG from the library, before anything is launched -- the map stays what it is
    pts, count, origin = _upload(dm, C.many_scans(64) + [C.single_ray(0)])
    st = torch.full((65, 2), -7, dtype=torch.int32, device=dm.device)
    f = solver.OccMapFusePoints()
    f.scans, f.P = 65, int(pts.shape[1])
    f.points, f.points_f32, f.count, f.origin, f.active, f.status = pts.data_ptr(), None, count.data_ptr(), origin.data_ptr(), None, st.data_ptr()
    for k in solver.OCCMAP_FUSE_POINTS_PARAMS:
        setattr(f, k, solver.OCCMAP_FUSE_DEFAULTS[k])
    m = dm._map()
    assert solver.lib().frp_nmpc_occmap_fuse_points_workspace_bytes(ctypes.byref(m), ctypes.byref(f)) == 0
    rc = solver.lib().frp_nmpc_occmap_fuse_points_batch(ctypes.byref(m), ctypes.byref(f), ctypes.c_void_p(dm.ws.data_ptr()), dm.ws_bytes,
                                                        ctypes.c_void_p(dm.fuse_points_ws.data_ptr()), int(dm.fuse_points_ws.numel()), None)
    assert rc == FRP_ERR_ARG
    with pytest.raises(ValueError):
        dm.fuse_points(pts, origin, count=count)
    assert (st.cpu().numpy() == -7).all()
    _assert_same(dm, om)
    f.scans = 64
    assert solver.lib().frp_nmpc_occmap_fuse_points_workspace_bytes(ctypes.byref(m), ctypes.byref(f)) > 0


def test_arguments_of_another_kind_are_value_errors():
    import torch
    dm = _device(poison=None)
    p = torch.zeros((2, 5, 3), dtype=torch.float64, device=dm.device)
    o = np.zeros((2, 3))
    for bad in (p.cpu(), p.to(torch.float16), p.to(torch.int32), p[:, :, :2], p.reshape(2, 15), p.transpose(0, 1), np.zeros((2, 5, 3))):
        with pytest.raises(ValueError):
            dm.fuse_points(bad, o)
    for kw in (dict(origin=np.zeros((3, 3))), dict(origin=torch.zeros((2, 3), dtype=torch.float32, device=dm.device)), dict(count=np.zeros(3, dtype=np.int32)),
               dict(active=torch.zeros((2,), dtype=torch.int64, device=dm.device)), dict(status=torch.zeros((2, 2), dtype=torch.int64, device=dm.device))):
        with pytest.raises(ValueError):
            dm.fuse_points(p, kw.pop("origin", o), **kw)
    with pytest.raises(ValueError):
        dm.fuse_points(p, o, max_ray_length=0.05)              # below min_ray_length: the library refuses the description
    with pytest.raises(TypeError):
        dm.fuse_points(p, o, skip_pixel=2)                     # a depth camera's parameter


# ---- 6. device-read inputs ----
def test_a_captured_call_replays_with_new_scans():
    """As tests/test_gpu_occmap_fusion_batch.py replays its call: captured on one stream, no parallel branches.  Between the
    replays points, count, origin and active are overwritten in place; the struct and both workspaces are the captured ones."""
    import torch
    dm = _device()
    first = [C.realistic("wall", "middle"), C.realistic("random", "near_face"), C.realistic("steps", "middle")]
    pts, count, origin = _upload(dm, first, P=713)
    active = torch.ones((3,), dtype=torch.int32, device=dm.device)
    status = torch.zeros((3, 2), dtype=torch.int32, device=dm.device)
    # plain calls first: the same tensors, overwritten in place between two calls
    om, want = C.chain(first)
    assert dm.fuse_points(pts, origin, count=count, active=active, status=status) is status
    _assert_same(dm, om)
    assert status.cpu().numpy().tolist() == want
    second = [C.realistic("steps", "near_face"), C.edge_sets()["NaN and inf rows"], C.edge_sets()["sensor outside the map"]]
    p2, c2, o2 = _upload(dm, second, P=713)
    pts.copy_(p2); count.copy_(c2); origin.copy_(o2); active.copy_(torch.tensor([1, 1, 0], dtype=torch.int32))
    _reset(dm)
    dm.fuse_points(pts, origin, count=count, active=active, status=status)
    om2, want2 = C.chain(second, skip={2})
    _assert_same(dm, om2)
    assert status.cpu().numpy().tolist() == C.want(want2)
    # captured
    p1, c1, o1 = _upload(dm, first, P=713)
    pts.copy_(p1); count.copy_(c1); origin.copy_(o1); active.fill_(1)
    side = torch.cuda.Stream(dm.device)
    side.wait_stream(torch.cuda.current_stream(dm.device))
    with torch.cuda.stream(side):
        dm.fuse_points(pts, origin, count=count, active=active, status=status, stream=side)          # warm-up on the capture stream
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        dm.fuse_points(pts, origin, count=count, active=active, status=status, stream=torch.cuda.current_stream())
    replays = [(second, {2}), ([first[2], first[0], C.edge_sets()["count 0"]], set()), (first, {0})]
    for rep, (given, off) in enumerate(replays):
        p, c, o = _upload(dm, given, P=713)
        pts.copy_(p); count.copy_(c); origin.copy_(o)
        active.copy_(torch.tensor([0 if k in off else 1 for k in range(3)], dtype=torch.int32))
        _reset(dm)
        dm.fuse_points_ws.fill_(0xA5 if rep == 0 else 0x3C); status.fill_(-7)
        torch.cuda.synchronize()
        g.replay()
        om_r, want_r = C.chain(given, skip=off)
        _assert_same(dm, om_r, rep)
        assert status.cpu().numpy().tolist() == C.want(want_r), rep
        assert om_r.buffer.tobytes() != om.buffer.tobytes()                                          # not the result of the captured scans


# ---- 7. downstream sees it ----
def test_query_local_view_and_check_surround_see_the_fused_scans_without_a_refresh():
    import torch
    scans = [C.realistic("wall", "middle"), C.realistic("steps", "near_face")]
    om, status = C.chain(scans)
    dm = _device()
    assert _fuse(dm, scans) == status
    changed = np.argwhere(om.occ() != C.oracle().occ())
    assert len(changed) >= 60                                                                        # voxels that became occupied or free
    rng = np.random.default_rng(8)
    pick = changed[rng.choice(len(changed), 60, replace=False)]
    pos = np.array(FO.TEST_GEO["origin"]) + (pick + rng.uniform(0.1, 0.9, pick.shape)) * 0.1
    pos = np.r_[pos, rng.uniform(-3.3, 3.3, (40, 3)) * np.array([1, 1, 0.5]) + np.array([0, 0, 1.6])]
    centres = np.array([[0.5, 0.2, 1.5], [-2.0, 2.5, 1.0]])
    boxes = [om.local_box(c) for c in centres]
    planner = (np.arange(len(pos)) % 2).astype(np.int32)
    v = dm.local_view(centres, 40000)
    got = dm.query(pos).cpu().numpy()
    got_box = dm.query(pos, v.local_box, planner).cpu().numpy()
    torch.cuda.synchronize()
    assert np.array_equal(got, np.array([om.get_voxel_state(p) for p in pos], dtype=np.int32)) and set(np.unique(got[:60])) == {0, 1}
    assert np.array_equal(got_box, np.array([om.get_voxel_state(p, boxes[b]) for p, b in zip(pos, planner)], dtype=np.int32))
    assert np.array_equal(v.local_box.cpu().numpy(), np.array(boxes, dtype=np.int32))
    for b, c in enumerate(centres):
        want = om.local_cloud(c)
        assert int(v.cloud_count[b]) == len(want) > 0 and np.array_equal(v.cloud[b, :len(want)].cpu().numpy(), want)
    probes = pos[:30]
    free = dm.check_surround(probes, 1.2).cpu().numpy()
    want_free = np.array([CO.check_pos_surround(om, p, 1.2) for p in probes], dtype=np.int32)
    before = np.array([CO.check_pos_surround(C.oracle(), p, 1.2) for p in probes], dtype=np.int32)
    assert np.array_equal(free, want_free)
    print("check_surround verdicts that the scans changed:", int((want_free != before).sum()))
