"""The frames and expected results that tests/test_occmap_fusion_batch_cpu.py and tests/test_gpu_occmap_fusion_batch.py share: batches
of the synthetic frames of tests/occmap_fusion_oracle.py (imported, not changed), and the serial oracle applied frame after frame --
which is what frp_nmpc_occmap_fuse_depth_batch has to equal to the bit.  Every chain is computed once per process."""
import functools

import numpy as np

from tests import occmap_fusion_oracle as FO

K = FO.TEST_K


def start_values(seed=3):
    """tests/test_gpu_occmap_fusion.py::_start_values: values at both clamps, around the occupancy threshold and in between."""
    return np.random.default_rng(seed).choice([-1.0, 0.3, 1.65, 1.75, 2.0], size=(64, 64, 32), p=[0.4, 0.3, 0.1, 0.1, 0.1])


def oracle():
    om = FO.FusionOracle(**FO.TEST_GEO, **FO.LAUNCH_CLAMPS)
    om.buffer[...] = start_values()
    return om


@functools.lru_cache(maxsize=None)
def six_frames():
    """The six frames of tests/test_gpu_occmap_fusion.py::test_six_frames_with_a_moving_camera: [(depth, T_wc)]."""
    out = []
    for k in range(6):
        T = FO.pose((-0.6 + 0.22 * k, 0.4 - 0.1 * k, 1.5 + 0.03 * k), yaw=0.25 - 0.06 * k, pitch=-0.1 + 0.02 * k)
        d = FO.scene(("wall", "random", "steps")[k % 3], seed=k)
        if k >= 3:
            d = (d.astype(np.int32) + 40 * (k - 2)).astype(np.uint16)
        out.append((d, T))
    return out


# A camera 30 m beside the 6.4 m map with rays of at most 6 m: posToIndex(t -/+ max_ray_length) lies beyond the +x face on both
# sides, the ray box is empty, every point ends outside the map and every ray is cast (no dedup for INVALID_IDX) through no voxel.
FAR_POSE = FO.pose((30.0, 0.1, 1.5))

# The six frames need 12, 11, 14, 10, 10 and 12 relaxation rounds (the CPU test checks it): with this cap frames 1, 3 and 4 converge and
# frames 0, 2 and 5 do not.
STRADDLE_CAP = 11


def chain(frames, lasts=None, skip=(), cap=None):
    """The serial oracle over `frames` [(depth, T_wc)] in the given order, from the start values.  lasts[k] = (last_depth,
    last_T_wc) of frame k (the shift filter) or None; frames whose index is in `skip` are left out (status None); with `cap`, a
    frame that needs more relaxation rounds is left out as well (status [-cap, rays]).  Returns (oracle, [status per frame])."""
    om, counter = oracle(), oracle()
    status = []
    for k, (d, T) in enumerate(frames):
        if k in skip:
            status.append(None)
            continue
        pts = om.project(d, K, T, last=None if lasts is None else lasts[k])
        _, rounds = counter.raycast_relaxed(pts, T[:3, 3])        # the round count does not depend on the map's values
        rays = counter.stats["rays"]
        if cap is not None and rounds > cap:
            status.append([-cap, rays])
            continue
        om.raycast(pts, T[:3, 3])
        status.append([rounds, rays])
    assert om.box_skips == 0
    return om, status


@functools.lru_cache(maxsize=None)
def six_in_order():
    return chain(six_frames())


@functools.lru_cache(maxsize=None)
def six_reversed():
    return chain(six_frames()[::-1])


def filter_lasts(frames):
    """last_depth[k] = depth[k - 1], last_T_wc[k] = T[k - 1]; frame 0 has no predecessor (it is switched off)."""
    return [None] + [frames[k - 1] for k in range(1, len(frames))]


@functools.lru_cache(maxsize=None)
def six_filtered():
    """The six frames with the shift filter, frame 0 switched off: (oracle, status)."""
    f = six_frames()
    return chain(f, lasts=filter_lasts(f), skip={0})


@functools.lru_cache(maxsize=None)
def six_by_fuse(shift_filter):
    """The same through FusionOracle.fuse, the oracle's own per-frame entry: the map after all six."""
    om = oracle()
    for d, T in six_frames():
        om.fuse(d, K, T, shift_filter=shift_filter)
    return om


def stack(frames):
    """([F, rows, cols] uint16, [F, 4, 4] float64) of [(depth, T_wc)]."""
    return np.ascontiguousarray(np.stack([d for d, _ in frames])), np.ascontiguousarray(np.stack([T for _, T in frames]))
