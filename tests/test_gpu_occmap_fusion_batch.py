"""GPU tests of batched depth fusion (include/frp_nmpc_occmap_fuse_batch.h, solver.OccupancyMap.fuse_depth_batch) against the serial
oracle applied frame after frame (tests/occmap_fusion_batch_cases.py on tests/occmap_fusion_oracle.py).  Everything compared is a
double that both sides compute with the same IEEE operations, a byte or an integer: equality is exact, nothing here has a
tolerance.  64 x 48 frames on the 64 x 64 x 32 map, at most six frames per call; tests/test_occmap_fusion_batch_cpu.py checks that
these inputs can tell a right implementation from a wrong one."""
import numpy as np
import pytest

from forces_resilient_planner_amd import solver
from tests import occmap_fusion_batch_cases as C
from tests import occmap_fusion_oracle as FO

pytestmark = pytest.mark.gpu


def _device(poison=None):
    """The oracle's start map on the device.  poison: the byte the batch's fusion workspace is filled with before the first call."""
    import torch
    dm = solver.OccupancyMap(**FO.TEST_GEO, **FO.LAUNCH_CLAMPS)
    _reset(dm)
    if poison is not None:
        dm.fuse_batch_ws = torch.full((16 << 20,), poison, dtype=torch.uint8, device=dm.device)   # larger than six frames need: the method keeps it
    return dm


def _reset(dm):
    import torch
    dm.log_odds.copy_(torch.from_numpy(C.start_values()).to(dm.device))
    dm.refresh()


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


def _fuse(dm, frames, **kw):
    depth, T = C.stack(frames)
    st = dm.fuse_depth_batch(depth, C.K, T, **kw)
    return st.cpu().numpy().tolist()


def _want(status):
    return [[0, 0] if s is None else s for s in status]


@pytest.mark.parametrize("placement", ["middle", "near_face"])
def test_one_frame_equals_the_single_frame_call(placement):
    frame = (FO.scene("random"), FO.pose(FO.PLACEMENTS[placement]))
    om, status = C.chain([frame])
    single, batch = _device(), _device(poison=0xFF)
    st1 = single.fuse_depth(frame[0], C.K, frame[1]).cpu().numpy().tolist()
    stb = _fuse(batch, [frame])
    assert stb == [st1] == status and st1[0] >= 2 and st1[1] > 100, (stb, st1, status)
    _assert_same(single, om, placement)
    _assert_same(batch, om, placement)


def test_six_frames_in_order():
    om, status = C.six_in_order()
    dm = _device(poison=0xFF)
    assert _fuse(dm, C.six_frames()) == status
    _assert_same(dm, om)
    assert dm.log_odds.cpu().numpy().tobytes() != C.six_reversed()[0].buffer.tobytes()   # the frames' order is kept


def test_six_frames_with_the_shift_filter():
    import torch
    om, status = C.six_filtered()
    frames = C.six_frames()
    dm = _device(poison=0xFF)
    depth, T = C.stack(frames)
    last_depth, last_T = np.roll(depth, 1, axis=0), np.roll(T, 1, axis=0)      # [k] = frame k - 1; [0] is never read: frame 0 is off
    active = torch.tensor([0, 1, 1, 1, 1, 1], dtype=torch.int32, device=dm.device)
    st = dm.fuse_depth_batch(depth, C.K, T, last_depth=last_depth, last_T_wc=last_T, active=active).cpu().numpy().tolist()
    assert st[0] == [0, 0] and st == _want(status), (st, status)
    _assert_same(dm, om)
    _assert_same(dm, C.six_by_fuse(True))                                      # the oracle's own shift_filter=True chain


def test_a_frame_that_does_not_converge_is_left_out():
    cap = C.STRADDLE_CAP
    om, status = C.chain(C.six_frames(), cap=cap)
    dm = _device(poison=0xFF)
    st = _fuse(dm, C.six_frames(), max_rounds=cap)
    assert st == status and sorted(s[0] for s in st) == [-cap, -cap, -cap, 10, 10, 11], (st, status)
    _assert_same(dm, om)
    # with the cap at the largest count every frame converges
    full, status_full = C.six_in_order()
    top = max(s[0] for s in status_full)
    _reset(dm)
    assert _fuse(dm, C.six_frames(), max_rounds=top) == status_full
    _assert_same(dm, full)


def test_a_refused_pose_stops_nothing():
    import torch
    frames = C.six_frames()[:3]
    om, status = C.chain(frames, skip={1})
    depth, T = C.stack(frames)
    bad = T.copy(); bad[1, 2, 1] = float("nan")
    dm = _device(poison=0xFF)
    st = dm.fuse_depth_batch(depth, C.K, bad).cpu().numpy().tolist()
    assert st[1] == [solver.OCCMAP_FUSE_REFUSED, 0] and solver.OCCMAP_FUSE_REFUSED == -256 and st[0] == status[0] and st[2] == status[2], (st, status)
    _assert_same(dm, om)
    # with the filter: an all-zero rotation in last_T_wc[2] (its inverse is not finite) refuses frame 2; frame 0 has no predecessor
    lasts = C.filter_lasts(frames)
    om, status = C.chain(frames, lasts=lasts, skip={0, 2})
    last_depth, last_T = np.roll(depth, 1, axis=0), np.roll(T, 1, axis=0)
    last_T[2, :3, :3] = 0.0
    dm = _device(poison=0xFF)
    active = torch.tensor([0, 1, 1], dtype=torch.int32, device=dm.device)
    st = dm.fuse_depth_batch(depth, C.K, T, last_depth=last_depth, last_T_wc=last_T, active=active).cpu().numpy().tolist()
    assert st == [[0, 0], status[1], [-256, 0]] and status[1][1] > 0, (st, status)
    _assert_same(dm, om)
    # a non-finite last_T_wc is refused as well, and only with the filter: without last_depth it is not read
    last_T[2] = T[1]; last_T[1, 0, 3] = float("inf")
    _reset(dm)
    st = dm.fuse_depth_batch(depth, C.K, T, last_depth=last_depth, last_T_wc=last_T, active=active).cpu().numpy().tolist()
    assert st[0] == [0, 0] and st[1] == [-256, 0] and st[2][0] > 0, st
    _assert_same(dm, C.chain(frames, lasts=lasts, skip={0, 1})[0])


def test_nothing_to_fuse_poison_and_an_empty_ray_box():
    import torch
    frames = C.six_frames()
    depth, T = C.stack(frames)
    # all frames off: the map, occ and the bit plane are untouched
    dm = _device(poison=0x5A)
    torch.cuda.synchronize()
    before = (dm.log_odds.cpu().numpy().tobytes(), dm.occ.cpu().numpy().tobytes(), dm.ws.cpu().numpy().tobytes())
    st = dm.fuse_depth_batch(depth, C.K, T, active=np.zeros(6, dtype=np.int32))
    torch.cuda.synchronize()
    assert st.cpu().numpy().tolist() == [[0, 0]] * 6
    assert (dm.log_odds.cpu().numpy().tobytes(), dm.occ.cpu().numpy().tobytes(), dm.ws.cpu().numpy().tobytes()) == before
    # the fusion workspace arrives uninitialised, whatever it holds
    om, status = C.six_in_order()
    for poison in (0x00, 0xFF, 0x5A):
        dm = _device(poison=poison)
        assert _fuse(dm, frames) == status, poison
        _assert_same(dm, om, poison)
    # a camera far outside the map between two ordinary frames: an empty ray box, rays through no voxel
    trio = [frames[0], (frames[1][0], C.FAR_POSE), frames[2]]
    om, status = C.chain(trio)
    single = _device()
    alone = single.fuse_depth(trio[1][0], C.K, C.FAR_POSE).cpu().numpy().tolist()
    dm = _device(poison=0xFF)
    st = _fuse(dm, trio)
    assert st[1] == alone == status[1] and alone[0] == 1 and alone[1] > 100 and st == status, (st, alone, status)
    _assert_same(dm, om)
    _assert_same(single, C.oracle())                                           # ... and alone it changes nothing


def test_a_captured_batch_replays_with_new_frames_and_poses():
    import torch
    frames = C.six_frames()
    dm = _device(poison=0xFF)

    def dev16(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dm.device).view(torch.uint16)

    first = frames[:3]
    depth_h, T_h = C.stack(first)
    depth, T = dev16(depth_h), torch.from_numpy(T_h).to(dm.device)
    active = torch.ones((3,), dtype=torch.int32, device=dm.device)
    status = torch.zeros((3, 2), dtype=torch.int32, device=dm.device)
    side = torch.cuda.Stream(dm.device)
    side.wait_stream(torch.cuda.current_stream(dm.device))
    with torch.cuda.stream(side):
        dm.fuse_depth_batch(depth, C.K, T, active=active, status=status, stream=side)     # warm-up on the capture stream
    side.synchronize()
    om, want = C.chain(first)
    _assert_same(dm, om)
    assert status.cpu().numpy().tolist() == want
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        dm.fuse_depth_batch(depth, C.K, T, active=active, status=status, stream=torch.cuda.current_stream())
    # other frames at other poses, then the first images at the poses of the last three with the middle frame switched off
    replays = [(frames[3:], set()), ([(frames[0][0], frames[5][1]), (frames[1][0], frames[4][1]), (frames[2][0], frames[3][1])], {1})]
    for rep, (given, off) in enumerate(replays):
        d_h, t_h = C.stack(given)
        depth.copy_(dev16(d_h)); T.copy_(torch.from_numpy(t_h).to(dm.device))
        active.copy_(torch.tensor([0 if k in off else 1 for k in range(3)], dtype=torch.int32))
        _reset(dm)
        dm.fuse_batch_ws.fill_(0xA5 if rep == 0 else 0x3C); status.fill_(-7)
        torch.cuda.synchronize()
        g.replay()
        om, want = C.chain(given, skip=off)
        _assert_same(dm, om, rep)
        assert status.cpu().numpy().tolist() == _want(want), rep
        assert om.buffer.tobytes() != C.chain(first)[0].buffer.tobytes()       # not the result of the captured poses
