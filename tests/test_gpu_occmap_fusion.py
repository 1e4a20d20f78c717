"""GPU tests of depth-image fusion (include/frp_nmpc_occmap_fuse.h, solver.OccupancyMap.fuse_depth) against the serial restatement
of the reference (tests/occmap_fusion_oracle.py).  Everything compared is a double that both sides compute with the same IEEE
operations, a byte or an integer: equality is exact, nothing here has a tolerance.  The frames are 64 x 48 pixels on a
64 x 64 x 32 map (a few hundred rays, several workgroups, rays that leave the map); each oracle frame is computed once."""
import ctypes
import functools

import numpy as np
import pytest

from forces_resilient_planner_amd import solver
from tests import occmap_fusion_oracle as FO

pytestmark = pytest.mark.gpu


def _start_values(seed=3):
    """Values at both clamps, around the occupancy threshold and in between (at clamp_min alone a miss would change nothing)."""
    return np.random.default_rng(seed).choice([-1.0, 0.3, 1.65, 1.75, 2.0], size=(64, 64, 32), p=[0.4, 0.3, 0.1, 0.1, 0.1])


def _oracle(**kw):
    om = FO.FusionOracle(**FO.TEST_GEO, **FO.LAUNCH_CLAMPS, **kw)
    om.buffer[...] = _start_values()
    return om


def _device(poison=None):
    """The same map on the device.  poison: the byte the fusion workspace is filled with before the first call."""
    import torch
    dm = solver.OccupancyMap(**FO.TEST_GEO, **FO.LAUNCH_CLAMPS)
    dm.log_odds.copy_(torch.from_numpy(_start_values()).to(dm.device))
    dm.refresh()
    if poison is not None:
        dm.fuse_ws = torch.full((8 << 20,), poison, dtype=torch.uint8, device=dm.device)   # larger than these frames need: fuse_depth keeps it
    return dm


def _assert_same(dm, om, what=""):
    """log_odds to the bit, occ, and the whole-map cloud of local_view -- which is read from the bit plane."""
    import torch
    torch.cuda.synchronize()
    assert dm.log_odds.cpu().numpy().tobytes() == om.buffer.tobytes(), what
    assert np.array_equal(dm.occ.cpu().numpy(), om.occ()), what
    want = om.local_cloud(None)
    assert 0 < len(want) <= solver.CORRIDOR_MAX_POINTS
    v = dm.local_view(None, len(want))
    torch.cuda.synchronize()
    assert int(v.cloud_count[0]) == len(want) and np.array_equal(v.cloud[0].cpu().numpy(), want), what


@functools.lru_cache(maxsize=None)
def _single(name, placement):
    """One frame through the serial oracle and through its round-based form: (map after, rounds, rays)."""
    a, b = _oracle(), _oracle()
    T = FO.pose(FO.PLACEMENTS[placement])
    a.fuse(FO.scene(name), FO.TEST_K, T)
    _, rounds = b.fuse(FO.scene(name), FO.TEST_K, T, relaxed=True)
    assert a.buffer.tobytes() == b.buffer.tobytes() and a.box_skips == 0
    return a, rounds, a.stats["rays"]


@pytest.mark.parametrize("placement", sorted(FO.PLACEMENTS))
@pytest.mark.parametrize("name", FO.SCENES)
def test_one_frame_equals_the_serial_scan(name, placement):
    om, rounds, rays = _single(name, placement)
    dm = _device(poison=0xFF)
    st = dm.fuse_depth(FO.scene(name), FO.TEST_K, FO.pose(FO.PLACEMENTS[placement]))
    _assert_same(dm, om, (name, placement))
    st = st.cpu().numpy()
    assert rounds >= 2 and st[0] == rounds and st[1] == rays and rays > 100, (st, rounds, rays)


def test_the_fusion_workspace_needs_no_initialisation():
    om, rounds, rays = _single("random", "middle")
    for poison in (0x00, 0xFF, 0x5A):
        dm = _device(poison=poison)
        st = dm.fuse_depth(FO.scene("random"), FO.TEST_K, FO.pose(FO.PLACEMENTS["middle"]))
        _assert_same(dm, om, poison)
        assert st.cpu().numpy().tolist() == [rounds, rays]
        # ... nor preserving: a second frame after the workspace was overwritten equals a second frame of the oracle
        dm.fuse_ws.fill_(0xFF - poison)
        dm.fuse_depth(FO.scene("steps"), FO.TEST_K, FO.pose(FO.PLACEMENTS["middle"]))
        o2 = _oracle(); o2.buffer[...] = om.buffer
        o2.fuse(FO.scene("steps"), FO.TEST_K, FO.pose(FO.PLACEMENTS["middle"]))
        _assert_same(dm, o2, poison)


@pytest.mark.parametrize("shift_filter", [False, True])
def test_six_frames_with_a_moving_camera(shift_filter):
    om, orx = _oracle(), _oracle()
    dm = _device(poison=0xFF)
    start = om.buffer.copy()
    for k in range(6):
        T = FO.pose((-0.6 + 0.22 * k, 0.4 - 0.1 * k, 1.5 + 0.03 * k), yaw=0.25 - 0.06 * k, pitch=-0.1 + 0.02 * k)
        d = FO.scene(("wall", "random", "steps")[k % 3], seed=k)
        if k >= 3:
            d = (d.astype(np.int32) + 40 * (k - 2)).astype(np.uint16)        # a slow change the filter lets through, next to the scene changes it drops
        om.fuse(d, FO.TEST_K, T, shift_filter=shift_filter)
        _, rounds = orx.fuse(d, FO.TEST_K, T, shift_filter=shift_filter, relaxed=True)
        st = dm.fuse_depth(d, FO.TEST_K, T, shift_filter=shift_filter)
        _assert_same(dm, om, k)
        st = st.cpu().numpy().tolist()
        if shift_filter and k == 0:
            assert st == [0, 0] and np.array_equal(om.buffer, start)         # the first filtered frame fuses nothing
        else:
            assert st == [rounds, om.stats["rays"]], (k, st, rounds, om.stats["rays"])
        if not shift_filter or k > 0:
            assert om.stats["rays"] > 0, k
    assert om.box_skips == 0 and orx.buffer.tobytes() == om.buffer.tobytes()
    moved = om.buffer != start
    # values accumulated over the frames and reached both clamps from elsewhere
    assert (om.buffer[moved] == om.clamp_max_log).any() and (om.buffer[moved] == om.clamp_min_log).any()
    assert ((om.buffer[moved] > om.clamp_min_log) & (om.buffer[moved] < om.clamp_max_log)).any()


def test_a_frame_that_does_not_converge_leaves_the_map_untouched():
    import torch
    om = _oracle()
    T = FO.pose(FO.PLACEMENTS["middle"])
    pts = om.project(FO.scene("steps"), FO.TEST_K, T)
    assert om.raycast_relaxed(pts, T[:3, 3], max_rounds=1) == (None, -1)      # the oracle needs at least two rounds on this frame
    dm = _device(poison=0xFF)
    torch.cuda.synchronize()
    before = (dm.log_odds.cpu().numpy().tobytes(), dm.occ.cpu().numpy().tobytes(), dm.ws.cpu().numpy().tobytes())
    st = dm.fuse_depth(FO.scene("steps"), FO.TEST_K, T, max_rounds=1)
    torch.cuda.synchronize()
    assert st.cpu().numpy()[0] == -1 and st.cpu().numpy()[1] == _single("steps", "middle")[2]
    assert (dm.log_odds.cpu().numpy().tobytes(), dm.occ.cpu().numpy().tobytes(), dm.ws.cpu().numpy().tobytes()) == before
    _assert_same(dm, om)
    # the cap exactly at the oracle's count converges, one below it does not
    rounds = _single("steps", "middle")[1]
    assert dm.fuse_depth(FO.scene("steps"), FO.TEST_K, T, max_rounds=rounds - 1).cpu().numpy()[0] == -(rounds - 1)
    _assert_same(dm, om)
    assert dm.fuse_depth(FO.scene("steps"), FO.TEST_K, T, max_rounds=rounds).cpu().numpy()[0] == rounds
    _assert_same(dm, _single("steps", "middle")[0])


def test_a_captured_frame_replays_on_a_fresh_map():
    import torch
    om, rounds, rays = _single("random", "near_face")
    dm = _device(poison=0xFF)
    T = FO.pose(FO.PLACEMENTS["near_face"])
    depth = torch.from_numpy(FO.scene("random").view(np.int16)).to(dm.device).view(torch.uint16)
    status = torch.zeros((2,), dtype=torch.int32, device=dm.device)
    side = torch.cuda.Stream(dm.device)
    side.wait_stream(torch.cuda.current_stream(dm.device))
    with torch.cuda.stream(side):
        dm.fuse_depth(depth, FO.TEST_K, T, status=status, stream=side)       # warm-up on the capture stream
    side.synchronize()
    _assert_same(dm, om)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        dm.fuse_depth(depth, FO.TEST_K, T, status=status, stream=torch.cuda.current_stream())
    for rep in range(2):
        dm.log_odds.copy_(torch.from_numpy(_start_values()).to(dm.device))   # a fresh copy of the map in the captured buffers
        dm.refresh()
        dm.fuse_ws.fill_(0xA5); status.fill_(-7)
        torch.cuda.synchronize()
        g.replay()
        _assert_same(dm, om, rep)
        assert status.cpu().numpy().tolist() == [rounds, rays]


def test_queries_see_the_frame_without_a_refresh():
    import torch
    om = _oracle()
    start = om.buffer.copy()
    T = FO.pose(FO.PLACEMENTS["middle"])
    om.fuse(FO.scene("wall"), FO.TEST_K, T)
    thr = om.min_occupancy_log
    freed = np.argwhere((start > thr) & (om.buffer <= thr)); occupied = np.argwhere((start <= thr) & (om.buffer > thr))
    assert len(freed) > 0 and len(occupied) > 0
    pos = np.array([om.index_to_pos(freed[0]), om.index_to_pos(occupied[0])])
    dm = _device()
    assert dm.query(pos).cpu().numpy().tolist() == [1, 0]
    dm.fuse_depth(FO.scene("wall"), FO.TEST_K, T)
    state = torch.zeros((2,), dtype=torch.int32, device=dm.device)
    q = torch.from_numpy(pos).to(dm.device)
    m = dm._map()
    rc = solver.lib().frp_nmpc_occmap_query(ctypes.byref(m), 2, ctypes.c_void_p(q.data_ptr()), None, None, ctypes.c_void_p(state.data_ptr()),
                                            ctypes.c_void_p(dm.ws.data_ptr()), dm.ws_bytes, ctypes.c_void_p(torch.cuda.current_stream(dm.device).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert state.cpu().numpy().tolist() == [0, 1]
    assert dm.query(pos).cpu().numpy().tolist() == [0, 1]
