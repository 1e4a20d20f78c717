"""GPU tests of the depth renderer (include/frp_nmpc_occmap_render.h, solver.OccupancyMap.render_depth / camera_poses) against its
specification (tests/occmap_render_oracle.py through tests/occmap_render_cases.py).  depth, voxel and status are integers that both
sides derive from doubles computed with the same IEEE operations: equality is exact.  Maps of 40 x 40 x 20 and 40 x 40 x 33 voxels
(a second word of the bit plane per column), images of 24 x 32 and 48 x 64 pixels -- neither a multiple of the 16 x 16 pixels of a
workgroup in both directions --, max_range 6 m.  tests/test_occmap_render_cpu.py checks the specification itself."""
import numpy as np
import pytest

from forces_resilient_planner_amd import solver
from tests import occmap_fusion_oracle as FO
from tests import occmap_render_cases as C
from tests import occmap_render_oracle as RO

pytestmark = pytest.mark.gpu
SENTINEL, VOX_SENTINEL = 0xBEEF, -7


def _world_map(scene, height):
    return solver.OccupancyMap(world=C.world(scene, height), **FO.LAUNCH_CLAMPS)


def _buffers(dm, F, image):
    """depth, voxel and status tensors holding sentinels: whatever a call does not write is seen."""
    import torch
    rows, cols = C.IMAGES[image]
    depth = torch.full((F, rows, cols), SENTINEL - 65536, dtype=torch.int16, device=dm.device).view(torch.uint16)
    voxel = torch.full((F, rows, cols), VOX_SENTINEL, dtype=torch.int32, device=dm.device)
    status = torch.full((F, 2), -9, dtype=torch.int32, device=dm.device)
    return depth, voxel, status


def _host16(depth):
    import torch
    return depth.view(torch.int16).cpu().numpy().view(np.uint16)


def _render(dm, T, image, Km=None, **kw):
    import torch
    rows, cols = C.IMAGES[image]
    depth, voxel, status = _buffers(dm, len(T), image)
    out = dm.render_depth(T, C.K[image] if Km is None else Km, rows, cols, max_range=C.MAX_RANGE, out=depth, voxel=voxel, status=status, **kw)
    torch.cuda.synchronize()
    assert out is depth
    return _host16(depth), voxel.cpu().numpy(), status.cpu().numpy().tolist()


@pytest.mark.parametrize("image", ["small", "large"])
@pytest.mark.parametrize("height", ["low", "tall"])
def test_six_frames_in_one_call_equal_the_specification(height, image):
    T, keys = C.six_poses("pillars", height)
    dm = _world_map("pillars", height)
    d, vox, st = _render(dm, T, image, active=np.array([1, 1, 1, 1, 0, 1], dtype=np.int32))
    for f, key in enumerate(keys):
        wd, wv, _, wst, _ = C.rendered("pillars", height, image, key)
        assert st[f] == wst, (f, st[f], wst)
        assert np.array_equal(d[f], wd) and np.array_equal(vox[f], wv), f
    assert st[0][1] > 100 and st[1][1] > 100 and st[2][1] > 100          # middle, near_face and the camera outside all see the pillars
    assert st[3] == [1, 0] and not d[3].any() and (vox[3] == -1).all()     # inside an occupied voxel
    assert st[4] == [0, 0] and (d[4] == SENTINEL).all() and (vox[4] == VOX_SENTINEL).all()   # inactive: its image is not written
    assert st[5] == [solver.OCCMAP_FUSE_REFUSED, 0] and not d[5].any() and (vox[5] == -1).all()   # a NaN pose: zeroed
    # without the mask the fifth frame is the first again, and a NULL voxel array is accepted
    import torch
    rows, cols = C.IMAGES[image]
    out = dm.render_depth(T, C.K[image], rows, cols, max_range=C.MAX_RANGE)
    torch.cuda.synchronize()
    h = _host16(out)
    assert np.array_equal(h[4], d[0]) and np.array_equal(h[:4], d[:4]) and not h[5].any()


@pytest.mark.parametrize("height", ["low", "tall"])
def test_an_axis_aligned_camera_with_an_integer_principal_point(height):
    """Direction components that are exactly zero: the central pixel's ray has two, its row and column one each."""
    scene = "wall" if height == "low" else "ceiling"
    keys = [("axis", -1.0, 1.0, 1.05), ("axis", -1.0, 1.0, 2.65 if height == "tall" else 1.61)]
    dm = _world_map(scene, height)
    for image in ("small", "large"):
        T = np.stack([C.pose_of(k) for k in keys])
        assert set(np.unique(T[:, :3, :3])) == {-1.0, 0.0, 1.0}
        d, vox, st = _render(dm, T, image, Km=C.K_INT[image])
        for f, key in enumerate(keys):
            wd, wv, _, wst, _ = C.rendered(scene, height, image, key, int_k=True)
            assert st[f] == wst and wst[1] > 100, (f, st[f], wst)
            assert np.array_equal(d[f], wd) and np.array_equal(vox[f], wv), (image, f)
        v0, u0 = int(C.K_INT[image][1, 2]), int(C.K_INT[image][0, 2])
        assert d[0, v0, u0] != 0                                          # the central ray returns from the wall
        if height == "tall":
            assert (vox[1][d[1] != 0] % 33 == 32).any()                    # returns from the second word of a column


def test_a_rendered_image_fused_into_an_empty_map_rebuilds_the_world():
    import torch
    image, height = "large", "low"
    rows, cols = C.IMAGES[image]
    keys = ["middle", "near_face"]
    T = np.stack([C.pose_of(k) for k in keys])
    world = _world_map("pillars", height)
    depth = world.render_depth(T, C.K[image], rows, cols, max_range=C.MAX_RANGE)
    belief = solver.OccupancyMap(**C.GEO[height], **FO.LAUNCH_CLAMPS)
    for _ in range(3):                                                     # -1 -> 0.2 -> 1.4 -> 2.0 crosses min_occupancy_log = 1.7
        st = belief.fuse_depth_batch(depth, C.K[image], T)
    torch.cuda.synchronize()
    assert all(s[0] > 0 and s[1] > 0 for s in st.cpu().numpy().tolist()), st   # both frames converged and cast rays
    got = belief.occ.cpu().numpy().reshape(-1) != 0
    allowed = C.world_occ("pillars", height).reshape(-1) != 0
    assert got.sum() > 50
    h = _host16(depth)
    for f, key in enumerate(keys):
        wd, _, seg, _, _ = C.rendered("pillars", height, image, key)
        assert np.array_equal(h[f], wd)
        ex = C.excluded(wd, seg)                                           # the 2 mm rule: these may re-project into a neighbour
        back = C.projected_voxels(wd, C.K[image], T[f], height)
        allowed[back[ex & (back >= 0)]] = True
    assert not (got & ~allowed).any(), int((got & ~allowed).sum())
    print(f"fused map: {int(got.sum())} occupied voxels, {int((got & (C.world_occ('pillars', height).reshape(-1) == 0)).sum())} of them outside the world")


def test_a_captured_render_and_fuse_replays_with_new_poses():
    import torch
    image, height = "small", "low"
    rows, cols = C.IMAGES[image]
    first, second = ["middle", "near_face"], [C.OUTSIDE, "middle"]
    world = _world_map("pillars", height)
    belief = solver.OccupancyMap(**C.GEO[height], **FO.LAUNCH_CLAMPS)
    T = torch.from_numpy(np.stack([C.pose_of(k) for k in first])).to(world.device)
    depth, voxel, status = _buffers(world, 2, image)
    fstatus = torch.full((2, 2), -9, dtype=torch.int32, device=world.device)

    def tick(stream):
        world.render_depth(T, C.K[image], rows, cols, max_range=C.MAX_RANGE, out=depth, voxel=voxel, status=status, stream=stream)
        belief.fuse_depth_batch(depth, C.K[image], T, status=fstatus, stream=stream)

    def poison():
        depth.view(torch.int16).fill_(SENTINEL - 65536); voxel.fill_(VOX_SENTINEL); status.fill_(-9); fstatus.fill_(-9)
        belief.reset()
        if belief.fuse_batch_ws is not None:
            belief.fuse_batch_ws.fill_(0xA5)
        torch.cuda.synchronize()

    def result():
        torch.cuda.synchronize()
        return (_host16(depth).copy(), voxel.cpu().numpy(), status.cpu().numpy().tolist(), fstatus.cpu().numpy().tolist(),
                belief.log_odds.cpu().numpy().tobytes(), belief.occ.cpu().numpy().tobytes())

    def check(res, keys):
        for f, key in enumerate(keys):
            wd, wv, _, wst, _ = C.rendered("pillars", height, image, key)
            assert np.array_equal(res[0][f], wd) and np.array_equal(res[1][f], wv) and res[2][f] == wst and wst[1] > 50, f
        assert all(s[0] > 0 and s[1] > 0 for s in res[3]), res[3]

    side = torch.cuda.Stream(world.device)
    side.wait_stream(torch.cuda.current_stream(world.device))
    poison()
    with torch.cuda.stream(side):
        tick(side)                                                          # eager, on the capture stream (also the warm-up)
    side.synchronize()
    eager = [result()]
    check(eager[0], first)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        tick(torch.cuda.current_stream())
    poison()
    g.replay()
    replayed = result()
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(replayed, eager[0]))
    # new poses written on the device: the replay renders and fuses them
    new_T = torch.from_numpy(np.stack([C.pose_of(k) for k in second])).to(world.device)
    T.copy_(new_T)
    poison()
    g.replay()
    replayed = result()
    check(replayed, second)
    poison()
    tick(None)
    again = result()
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(replayed, again))
    assert replayed[4] != eager[0][4]                                       # not the map of the captured poses


def _states(B, seed=11):
    """Planner states inside the test map: position, velocity, (roll, pitch, yaw)."""
    rng = np.random.default_rng(seed)
    st = np.zeros((B, 9))
    st[:, 0] = rng.uniform(-2.0, 2.0, B); st[:, 1] = rng.uniform(-0.8, 3.2, B); st[:, 2] = rng.uniform(0.5, 1.8, B)
    st[:, 3:6] = rng.uniform(-1, 1, (B, 3))
    st[:, 6:8] = rng.uniform(-0.4, 0.4, (B, 2))
    st[:, 8] = rng.uniform(-np.pi, np.pi, B)
    return st


T_BC = FO.pose((0.05, -0.02, 0.1), yaw=0.1, pitch=-0.2)


def test_camera_poses_equal_the_numpy_statement():
    import torch
    dm = _world_map("wall", "low")
    st = _states(64)
    got = dm.camera_poses(st, T_BC)
    torch.cuda.synchronize()
    want = RO.camera_poses(st, T_BC)
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"camera_poses: max |device - numpy| = {err:.3e}")
    assert err <= 1e-15
    assert np.array_equal(got.cpu().numpy()[:, 3], np.tile(T_BC[3], (64, 1)))
    # B = 0 launches nothing, and a device tensor is used in place
    assert tuple(dm.camera_poses(np.zeros((0, 9)), T_BC).shape) == (0, 4, 4)
    out = torch.zeros((64, 4, 4), dtype=torch.float64, device=dm.device)
    assert dm.camera_poses(torch.from_numpy(st).to(dm.device), T_BC, out=out) is out
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), got.cpu().numpy())


def test_camera_poses_feed_the_renderer_without_the_host():
    import torch
    image = "small"
    rows, cols = C.IMAGES[image]
    dm = _world_map("wall", "low")
    st = _states(3, seed=12)
    st[:, 0] = (-1.0, 0.03, -0.5); st[:, 1] = (1.0, -0.02, 2.0); st[:, 2] = (1.05, 1.61, 1.2); st[:, 8] = (0.0, 0.3, -0.4)   # facing the wall
    T_dev = dm.camera_poses(torch.from_numpy(st).to(dm.device), T_BC)
    chained = dm.render_depth(T_dev, C.K[image], rows, cols, max_range=C.MAX_RANGE)
    host = dm.render_depth(RO.camera_poses(st, T_BC), C.K[image], rows, cols, max_range=C.MAX_RANGE)
    torch.cuda.synchronize()
    a, b = _host16(chained), _host16(host)
    assert np.array_equal(a, b) and all((a[f] != 0).sum() > 100 for f in range(3))
    want = RO.RenderOracle(C.world_occ("wall", "low"), C.GEO["low"]["origin"], 0.1).render(RO.camera_poses(st, T_BC)[1], C.K[image], rows, cols, C.MAX_RANGE)[0]
    assert np.array_equal(b[1], want)
