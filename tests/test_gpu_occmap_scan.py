"""GPU tests of the point-scan renderer (include/frp_nmpc_occmap_render_scan.h, solver.OccupancyMap.render_scan) against its
specification (tests/occmap_scan_oracle.py through tests/occmap_scan_cases.py).  Points and ranges are doubles that both sides
compute with the same IEEE operations in the same order, voxels, counts and status are integers derived from them: equality is
exact, nothing here has a tolerance.  Maps of 40 x 40 x 20 and 40 x 40 x 33 voxels (a second word of the bit plane per column), a
table of 1160 beams (18 wavefronts and 8 lanes), max_range 6 m.  tests/test_occmap_scan_cpu.py checks the specification itself."""
import numpy as np
import pytest

from forces_resilient_planner_amd import solver
from tests import occmap_fusion_oracle as FO
from tests import occmap_render_cases as RC
from tests import occmap_scan_cases as C

pytestmark = pytest.mark.gpu
POISON, VOX_POISON, INT_POISON = -777.25, -7, -9


def _world_map(scene, height):
    return solver.OccupancyMap(world=C.world(scene, height), **FO.LAUNCH_CLAMPS)


def _buffers(dm, S, P, both=True):
    """Every output tensor holding poison: whatever a call does not write is seen."""
    import torch
    f = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device=dm.device)
    return dict(points=f((S, P, 3), torch.float64, POISON), points_f32=f((S, P, 3), torch.float32, POISON) if both else None,
                origin=f((S, 3), torch.float64, POISON), count=f((S,), torch.int32, INT_POISON), range=f((S, P), torch.float64, POISON),
                voxel=f((S, P), torch.int32, VOX_POISON), status=f((S, 2), torch.int32, INT_POISON))


def _scan(dm, T, beams, both=True, **kw):
    """One call into poisoned buffers; returns them as numpy arrays."""
    import torch
    buf = _buffers(dm, len(T), len(beams), both)
    out = dm.render_scan(T, beams, max_range=C.MAX_RANGE, **{k: v for k, v in buf.items() if v is not None}, **kw)
    torch.cuda.synchronize()
    assert out[0] is buf["points"] and out[1] is buf["origin"] and out[2] is buf["count"] and out[3] is buf["status"]
    return {k: v.cpu().numpy() for k, v in buf.items() if v is not None}


def _same_points(got, want, what=""):
    """Bit-equal where finite, NaN exactly where the specification has NaN."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got[~nan].view(np.uint64), np.ascontiguousarray(want[~nan]).view(np.uint64)), what


def _assert_scan(got, s, want, what=""):
    """Scan s of a call against the specification's dict."""
    _same_points(got["points"][s], want["points"], what)
    if "points_f32" in got:
        f, w = got["points_f32"][s], got["points"][s].astype(np.float32)
        assert np.array_equal(np.isnan(f), np.isnan(w)) and np.array_equal(f[~np.isnan(w)], w[~np.isnan(w)]), what
    assert np.array_equal(got["range"][s].view(np.uint64), want["range"].view(np.uint64)), what
    assert np.array_equal(got["voxel"][s], want["voxel"]), what
    assert np.array_equal(got["origin"][s], want["origin"]), what
    assert int(got["count"][s]) == want["count"] and got["status"][s].tolist() == want["status"], (what, got["status"][s], want["status"])


def _assert_six(got, scene, height, **kw):
    """The six scans of C.six_poses: four against the specification, the inactive one untouched, the NaN pose refused."""
    T, keys = C.six_poses(scene, height)
    P = len(C.beams())
    for s, key in enumerate(keys):
        _assert_scan(got, s, C.scanned(scene, height, key, **kw), (scene, height, s))
    st = got["status"].tolist()
    assert st[0][1] > 100 and st[1][1] > 100 and st[2][1] > 100           # middle, near_face and the sensor outside all see the pillars
    assert st[3] == [1, 0] and (got["voxel"][3] == -1).all() and int(got["count"][3]) == P       # inside an occupied voxel
    # inactive: nothing of the scan is written but count = 0
    assert st[4] == [0, 0] and int(got["count"][4]) == 0
    assert (got["points"][4] == POISON).all() and (got["points_f32"][4] == np.float32(POISON)).all() and (got["origin"][4] == POISON).all()
    assert (got["range"][4] == POISON).all() and (got["voxel"][4] == VOX_POISON).all()
    # a NaN pose: refused, points NaN, range 0, voxel -1, count 0, origin as it stands
    assert st[5] == [solver.OCCMAP_FUSE_REFUSED, 0] and int(got["count"][5]) == 0
    assert np.isnan(got["points"][5]).all() and np.isnan(got["points_f32"][5]).all() and not got["range"][5].any() and (got["voxel"][5] == -1).all()
    assert np.array_equal(got["origin"][5], T[5, :3, 3])
    return st


@pytest.mark.parametrize("height", ["low", "tall"])
def test_six_scans_in_one_call_equal_the_specification(height):
    T, _ = C.six_poses("pillars", height)
    dm = _world_map("pillars", height)
    got = _scan(dm, T, C.beams(), active=C.ACTIVE6)
    _assert_six(got, "pillars", height)
    # the beams that are not fired give NaN, the others of a far_range-less scan NaN exactly where there is no return
    P = len(C.beams())
    assert np.isnan(got["points"][0][P - 8:P - 5]).all()
    assert np.array_equal(np.isnan(got["points"][0]).any(axis=1), got["voxel"][0] < 0)
    if height == "tall":
        assert (got["voxel"][:3][got["voxel"][:3] >= 0] % 33 >= 20).any()  # returns above the low map's top
    # without the mask the fifth scan is the first again; fresh tensors and float32 points alone are accepted
    import torch
    pts, origin, count, status = dm.render_scan(T, C.beams(), max_range=C.MAX_RANGE, dtype=torch.float32)
    torch.cuda.synchronize()
    assert pts.dtype == torch.float32 and count.cpu().numpy().tolist() == [P, P, P, P, P, 0]
    h = pts.cpu().numpy()
    for a, b in ((h[4], got["points_f32"][0]), (h[:4], got["points_f32"][:4])):
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
    assert status.cpu().numpy().tolist()[4] == got["status"].tolist()[0] and np.array_equal(origin.cpu().numpy()[4], got["origin"][0])


def test_far_range_puts_a_point_on_every_fired_beam_without_a_return():
    T, _ = C.six_poses("pillars", "low")
    dm = _world_map("pillars", "low")
    got = _scan(dm, T, C.beams(), active=C.ACTIVE6, far_range=8.0)
    st = _assert_six(got, "pillars", "low", far_range=8.0)
    P = len(C.beams())
    for s in range(4):
        finite = np.isfinite(got["points"][s]).all(axis=1)
        assert finite.sum() == P - C.N_UNFIRED and (got["voxel"][s] >= 0).sum() == st[s][1] < finite.sum()    # far points are no returns
    assert np.isfinite(got["points"][3][:P - 8]).all()                     # inside an occupied voxel: every fired beam gives the far point


def test_min_range_drops_the_near_returns():
    T, keys = C.six_poses("pillars", "low")
    dm = _world_map("pillars", "low")
    got = _scan(dm, T, C.beams(), active=C.ACTIVE6, min_range=1.0)
    st = _assert_six(got, "pillars", "low", min_range=1.0)
    for s in range(3):
        all_ = C.scanned("pillars", "low", keys[s])
        assert (all_["range"][all_["voxel"] >= 0] < 1.0).sum() == all_["status"][1] - st[s][1], s
        assert (got["range"][s][got["voxel"][s] >= 0] >= 1.0).all()
    assert C.scanned("pillars", "low", "near_face")["status"][1] - st[1][1] > 50         # near_face stands less than 1 m from a pillar


def test_an_axis_aligned_sensor_on_the_lattice():
    """Direction components that are exactly zero, and a sensor on voxel faces: the exact axis beams run along the faces."""
    keys = [("axis", -1.0, 1.0, 1.05), ("axis", -1.0, 1.0, 1.0)]
    dm = _world_map("wall", "low")
    T = np.stack([C.pose_of(k) for k in keys])
    assert set(np.unique(T[:, :3, :3])) == {0.0, 1.0}
    got = _scan(dm, T, C.beams())
    for s, key in enumerate(keys):
        want = C.scanned("wall", "low", key)
        _assert_scan(got, s, want, s)
        assert want["status"][1] > 100 and want["voxel"][len(C.beams()) - 5] >= 0     # the +x beam returns from the wall


@pytest.mark.parametrize("P", [1, 65])
def test_one_beam_and_one_lane_of_a_second_wavefront(P):
    T, keys = C.six_poses("pillars", "low")
    dm = _world_map("pillars", "low")
    got = _scan(dm, T[:2], C.beams()[:P])
    for s in range(2):
        want = C.scanned("pillars", "low", keys[s], table=P)
        _assert_scan(got, s, want, (P, s))
    assert got["status"][:, 1].sum() > 0


def test_the_pinhole_table_gives_the_voxel_image_of_render_depth():
    import torch
    rows, cols = RC.IMAGES["large"]
    Km = RC.K["large"]
    T = np.stack([RC.pose_of(k) for k in ("middle", "near_face", RC.OUTSIDE)])
    dm = _world_map("pillars", "low")
    vox = torch.full((3, rows, cols), VOX_POISON, dtype=torch.int32, device=dm.device)
    st = torch.zeros((3, 2), dtype=torch.int32, device=dm.device)
    dm.render_depth(T, Km, rows, cols, max_range=C.MAX_RANGE, voxel=vox, status=st)
    got = _scan(dm, T, C.pinhole_beams(Km, rows, cols), both=False)
    assert np.array_equal(got["voxel"].reshape(3, rows, cols), vox.cpu().numpy())
    assert got["status"].tolist() == st.cpu().numpy().tolist() and all(s[1] > 100 for s in got["status"].tolist())


# ---- the closed loop: render_scan of the world, fuse_points into an empty belief ----
def _belief(height):
    return solver.OccupancyMap(**C.GEO[height], **FO.LAUNCH_CLAMPS)


@pytest.mark.parametrize("as_float", [False, True], ids=["double", "float"])
def test_a_rendered_scan_fused_into_an_empty_map_rebuilds_the_world(as_float):
    import torch
    scene, height, keys = "pillars", "low", ["middle", "near_face"]
    T = np.stack([C.pose_of(k) for k in keys])
    world, belief = _world_map(scene, height), _belief(height)
    pts, origin, count, status = world.render_scan(T, C.beams(), max_range=C.MAX_RANGE, dtype=torch.float32 if as_float else torch.float64)
    for _ in range(3):                                                     # -1 -> 0.2 -> 1.4 -> 2.0 crosses min_occupancy_log = 1.7
        st = belief.fuse_points(pts, origin, count=count)
    torch.cuda.synchronize()
    assert all(s[0] > 0 and s[1] > 100 for s in st.cpu().numpy().tolist()), st   # both scans converged and cast rays
    # log_odds to the bit of the serial oracle fusing the ORACLE's points scan after scan
    want = [C.scanned(scene, height, k) for k in keys]
    cast = (lambda p: p.astype(np.float32).astype(np.float64)) if as_float else (lambda p: p)
    om = C.fuse_chain(height, [(cast(w["points"]), w["origin"]) for w in want], times=3)
    assert belief.log_odds.cpu().numpy().tobytes() == om.buffer.tobytes()
    assert belief.occ.cpu().numpy().tobytes() == om.occ().astype(np.uint8).tobytes()
    # the two containment statements of the CPU round trip, on the device result
    log = belief.log_odds.cpu().numpy().reshape(-1)
    occ = C.world_occ(scene, height).reshape(-1) != 0
    margin = C.MARGIN[np.float32 if as_float else np.float64]
    allowed = occ.copy()
    fo = C.fusion_oracle(height)
    h = pts.cpu().numpy().astype(np.float64)
    for s, w in enumerate(want):
        ret = w["voxel"] >= 0
        ex = C.excluded(h[s], ret, height, margin)
        assert ex.sum() <= 0.01 * ret.sum()
        assert (log[w["voxel"][ret & ~ex]] > belief.clamp_min_log).all()    # every kept hit voxel has a raised log-odds
        for p in np.flatnonzero(ex):
            id_ = fo._index([float(v) for v in h[s][p]])
            if id_ is not None:
                allowed[C.linear(id_, height)] = True
    got = log > belief.min_occupancy_log
    assert got.sum() > 50 and not (got & ~allowed).any(), (int(got.sum()), int((got & ~allowed).sum()))


def _states(rows):
    """Planner states [B, 9] (position, velocity, roll, pitch, yaw) from (x, y, z, yaw) rows, a small roll and pitch on each."""
    st = np.zeros((len(rows), 9))
    for k, (x, y, z, yaw) in enumerate(rows):
        st[k, 0:3] = (x, y, z); st[k, 3:6] = (0.1, -0.2, 0.05); st[k, 6:9] = (0.03 * (k + 1), -0.05, yaw)
    return st


T_BS = C.sensor_pose((0.05, -0.02, 0.1), yaw=0.1, pitch=-0.2)              # the LiDAR on the body


def test_a_captured_poses_scan_and_fuse_chain_replays_with_new_states():
    import torch
    from tests import occmap_render_oracle as RO
    scene, height = "pillars", "low"
    first = _states([FO.PLACEMENTS["middle"] + (0.3,), FO.PLACEMENTS["near_face"] + (-0.4,)])
    second = _states([(-2.6, 1.0, 1.2, 0.2), FO.PLACEMENTS["middle"] + (2.0,)])
    world, belief = _world_map(scene, height), _belief(height)
    beams = torch.from_numpy(np.array(C.beams())).to(world.device)
    P = len(C.beams())
    state = torch.from_numpy(first).to(world.device)
    T = torch.zeros((2, 4, 4), dtype=torch.float64, device=world.device)
    buf = _buffers(world, 2, P)
    fstatus = torch.full((2, 2), INT_POISON, dtype=torch.int32, device=world.device)

    def tick(stream):
        world.camera_poses(state, T_BS, out=T, stream=stream)
        world.render_scan(T, beams, max_range=C.MAX_RANGE, far_range=8.0, stream=stream, **buf)
        belief.fuse_points(buf["points"], buf["origin"], count=buf["count"], status=fstatus, stream=stream)

    def poison():
        for k, v in buf.items():
            v.fill_(POISON if v.dtype.is_floating_point else INT_POISON)
        T.fill_(POISON); fstatus.fill_(INT_POISON)
        belief.reset()
        if belief.fuse_points_ws is not None:
            belief.fuse_points_ws.fill_(0xA5)
        torch.cuda.synchronize()

    def result():
        torch.cuda.synchronize()
        return ([buf[k].cpu().numpy().tobytes() for k in sorted(buf)] +
                [T.cpu().numpy().tobytes(), fstatus.cpu().numpy().tolist(), belief.log_odds.cpu().numpy().tobytes(), belief.occ.cpu().numpy().tobytes()])

    def check(states):
        """The chain's result against the specification on the poses of the numpy statement."""
        torch.cuda.synchronize()
        want_T = RO.camera_poses(states, T_BS)
        got = {k: v.cpu().numpy() for k, v in buf.items()}
        o = C.oracle(scene, height)
        scans = []
        for s in range(2):
            w = o.scan(T.cpu().numpy()[s], C.beams(), C.MAX_RANGE, far_range=8.0)
            # (the poses: the device's sin and cos against numpy's, a few ulp of entries below 4 -- tests/test_gpu_occmap_render.py
            # compares them; the scan is compared to the bit on the pose the device computed)
            assert np.abs(T.cpu().numpy()[s] - want_T[s]).max() <= 1e-14
            _assert_scan(got, s, w, s)
            assert w["status"][1] > 100
            scans.append((w["points"], w["origin"]))
        assert all(s[0] > 0 and s[1] > 100 for s in fstatus.cpu().numpy().tolist())
        assert belief.log_odds.cpu().numpy().tobytes() == C.fuse_chain(height, scans).buffer.tobytes()

    side = torch.cuda.Stream(world.device)
    side.wait_stream(torch.cuda.current_stream(world.device))
    poison()
    with torch.cuda.stream(side):
        tick(side)                                                          # eager, on the capture stream (also the warm-up)
    side.synchronize()
    eager = result()
    check(first)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        tick(torch.cuda.current_stream())
    poison()
    g.replay()
    assert result() == eager
    # new states written on the device: the replay computes their poses, renders and fuses them
    state.copy_(torch.from_numpy(second).to(world.device))
    poison()
    g.replay()
    replayed = result()
    check(second)
    poison()
    tick(None)
    assert result() == replayed
    assert replayed[-2] != eager[-2]                                        # not the map of the captured states
