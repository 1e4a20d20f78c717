"""CPU tests of depth-image fusion: the round-based form equals the serial restatement (tests/occmap_fusion_oracle.py), hand-computed
known answers for the restatement, and the boundary of include/frp_nmpc_occmap_fuse.h as far as it exists without a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from forces_resilient_planner_amd import solver
from tests import occmap_fusion_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRP_ERR_NO_DEVICE, FRP_ERR_ARG = -1001, -1003


def _start_values(shape, seed=3):
    """A map that is not all at clamp_min (where a miss changes nothing): values at both clamps, around the threshold, in between."""
    return np.random.default_rng(seed).choice([-1.0, 0.3, 1.65, 1.75, 2.0], size=shape, p=[0.4, 0.3, 0.1, 0.1, 0.1])


@pytest.mark.parametrize("placement", sorted(FO.PLACEMENTS))
@pytest.mark.parametrize("name", FO.SCENES)
def test_relaxed_equals_serial(name, placement):
    a = FO.FusionOracle(**FO.TEST_GEO, **FO.LAUNCH_CLAMPS); b = FO.FusionOracle(**FO.TEST_GEO, **FO.LAUNCH_CLAMPS)
    assert tuple(a.grid_size) == (64, 64, 32) and a.skip_pixel == 2 and a.depth_filter_margin == 1
    a.buffer[...] = _start_values(a.buffer.shape); b.buffer[...] = a.buffer
    before = a.buffer.copy()
    T = FO.pose(FO.PLACEMENTS[placement])
    d = FO.scene(name)
    stops = a.fuse(d, FO.TEST_K, T)
    stops_r, rounds = b.fuse(d, FO.TEST_K, T, relaxed=True)
    assert stops_r == stops and len(stops) > 100
    assert a.buffer.tobytes() == b.buffer.tobytes()
    print(f"{name} {placement}: {rounds} rounds, {a.stats['rays']} rays, {b.stats['serial_steps']} of {b.stats['full_steps']} cells")
    assert rounds >= 2 and a.stats["rays"] == b.stats["rays"] and a.stats["serial_steps"] == b.stats["serial_steps"] < b.stats["full_steps"]
    assert a.box_skips == 0 and b.box_skips == 0                       # the ray box hid no voxel of the map from a ray
    changed = a.buffer != before
    assert changed.sum() > 100 and (a.buffer[changed] > before[changed]).any() and (a.buffer[changed] < before[changed]).any()
    if placement == "near_face":                                       # rays did leave the map: some ends are outside it
        pts = a.project(d, FO.TEST_K, T)
        assert any(not a._in_map_f(a.pos_to_index_f(p)) for p in pts) and any(a._in_map_f(a.pos_to_index_f(p)) for p in pts)


def small(**kw):
    """8 x 4 x 2 voxels of 0.5 m from the origin; hit + 0.5, miss - 0.25, clamps 0 and 1: every number below is exact in binary."""
    m = FO.FusionOracle(origin=(0.0, 0.0, 0.0), map_size=(4.0, 2.0, 1.0), resolution=0.5, clamp_min_log=0.0, clamp_max_log=1.0, min_occupancy_log=0.75,
                        prob_hit_log=0.5, prob_miss_log=-0.25, min_ray_length=0.1, max_ray_length=kw.pop("max_ray_length", 3.5), **kw)
    assert tuple(m.grid_size) == (8, 4, 2)
    m.buffer[...] = 0.5
    return m


CAM = (0.25, 0.25, 0.25)   # the centre of voxel (0, 0, 0)


def _row(m):
    return [float(m.buffer[x, 0, 0]) for x in range(8)]


@pytest.mark.parametrize("relaxed", [False, True])
def test_two_rays_that_share_voxels_known_answer(relaxed):
    m = small()
    A, B = (2.25, 0.25, 0.25), (1.75, 0.25, 0.25)   # voxels (4, 0, 0) and (3, 0, 0), both seen along -x from the camera
    run = (lambda: m.raycast_relaxed([A, B], CAM)) if relaxed else (lambda: (m.raycast([A, B], CAM), None))
    # ray A (first in scan order): start cell 4 skipped, cells 3, 2, 1 counted and marked, the camera's cell 0 is the end (never counted)
    # ray B: cell 2 counted, found marked by A: break (cell 1 not counted again)
    #   voxel 4: all 1 hit 1 -> hit;  3: all 2 (A's traversal, B's end) hit 1 -> 1 >= 1: hit;  2: all 2 hit 0 -> miss;  1: all 1 hit 0 -> miss
    stops, rounds = run()
    assert stops == {0: 3, 1: 1} and rounds in (None, 2)
    assert m.last_counts == {(4, 0, 0): (1, 1), (3, 0, 0): (2, 1), (2, 0, 0): (2, 0), (1, 0, 0): (1, 0)}    # {voxel: (all, hit)}
    assert _row(m) == [0.5, 0.25, 0.25, 1.0, 1.0, 0.5, 0.5, 0.5]
    assert np.all(np.delete(m.buffer.reshape(8, -1), 0, axis=1) == 0.5)          # nothing outside the row y = z = 0
    run()   # again: 3 and 4 sit at clamp_max with a hit: skipped (:516); 1 and 2 reach clamp_min exactly
    assert _row(m) == [0.5, 0.0, 0.0, 1.0, 1.0, 0.5, 0.5, 0.5]
    run()   # and stay there (:517)
    assert _row(m) == [0.5, 0.0, 0.0, 1.0, 1.0, 0.5, 0.5, 0.5]
    assert list(m.occ()[:, 0, 0]) == [0, 0, 0, 1, 1, 0, 0, 0]


def test_end_voxel_dedup_and_an_end_outside_the_map():
    m = small()
    # two points in voxel (4, 0, 0): both count as hits there, only the first casts its ray
    m.raycast([(2.25, 0.25, 0.25), (2.4, 0.3, 0.2)], CAM)
    assert m.stats["rays"] == 1 and m.stats["stops"] == {0: 3}
    assert m.last_counts == {(4, 0, 0): (2, 2), (3, 0, 0): (1, 0), (2, 0, 0): (1, 0), (1, 0, 0): (1, 0)}
    assert _row(m) == [0.5, 0.25, 0.25, 0.25, 1.0, 0.5, 0.5, 0.5]
    # two points beyond the map's +y face (y = 2.25, 2.3: index 4 = grid_size): INVALID_IDX, no dedup, both rays are cast (:470);
    # from cell (0, 4, 0) down to the camera's (0, 0, 0): cells y = 3, 2, 1; the second ray counts y = 3 and breaks there
    m = small()
    m.raycast([(0.25, 2.25, 0.25), (0.25, 2.3, 0.25)], CAM)
    assert m.stats["rays"] == 2 and m.stats["stops"] == {0: 3, 1: 1}
    assert m.last_counts == {(0, 3, 0): (2, 0), (0, 2, 0): (1, 0), (0, 1, 0): (1, 0)}
    assert [float(m.buffer[0, y, 0]) for y in range(4)] == [0.5, 0.25, 0.25, 0.25]   # y = 3: all 2, hit 0 -> one miss update, like the others
    r = small()
    assert r.raycast_relaxed([(0.25, 2.25, 0.25), (0.25, 2.3, 0.25)], CAM) == ({0: 3, 1: 1}, 2) and np.array_equal(r.buffer, m.buffer)


def test_ray_length_limits_and_depth_zero():
    m = small(max_ray_length=2.0)
    # 3 m away along x, max_ray_length 2: clipped to x = 0.25 + 2 = 2.25 -> voxel 4 gets a MISS (occ = 0, :463-464), the ray runs from there
    m.raycast([(3.25, 0.25, 0.25)], CAM)
    assert _row(m) == [0.5, 0.25, 0.25, 0.25, 0.25, 0.5, 0.5, 0.5] and m.stats["stops"] == {0: 3}
    # 0.05 m away, min_ray_length 0.1: dropped before anything is counted (:459)
    m = small()
    m.raycast([(0.3, 0.25, 0.25)], CAM)
    assert np.all(m.buffer == 0.5) and m.stats["rays"] == 0
    # 0.125 m away is not below min_ray_length: the point counts as a hit in the camera's own voxel, no ray (start cell = end cell, :306)
    m.raycast([(0.25, 0.25, 0.375)], CAM)
    assert m.stats["rays"] == 1 and m.stats["stops"] == {} and float(m.buffer[0, 0, 0]) == 1.0 and np.count_nonzero(m.buffer != 0.5) == 1
    # depth 0 (no return): below depth_filter_mindist, never projected (:334); an image of zeros fuses nothing
    K = np.array([[4.0, 0, 4.0], [0, 4.0, 4.0], [0, 0, 1.0]])
    d = np.zeros((8, 8), dtype=np.uint16)
    m = small(depth_filter_margin=0, skip_pixel=1)
    assert m.project(d, K, FO.pose(CAM, 0.0, 0.0)) == []
    d[3, 5] = 1500
    pts = m.project(d, K, FO.pose(CAM, 0.0, 0.0))
    # p_cam = ((5 - 4) * 1.5 / 4, (3 - 4) * 1.5 / 4, 1.5) = (0.375, -0.375, 1.5); world = (z, -x, -y) + t
    assert pts == [(1.75, -0.125, 0.625)]
    m.fuse(np.zeros((8, 8), dtype=np.uint16), K, FO.pose(CAM, 0.0, 0.0))
    assert np.all(m.buffer == 0.5) and m.stats["rays"] == 0


def test_shift_filter():
    K = np.array([[4.0, 0, 4.0], [0, 4.0, 4.0], [0, 0, 1.0]])
    m = small(depth_filter_margin=0, skip_pixel=1, depth_filter_tolerance=0.2)
    T = FO.pose(CAM, 0.0, 0.0)
    cur = np.zeros((8, 8), dtype=np.uint16); cur[3, 5] = 1500; cur[2, 2] = 1000
    last = cur.copy(); last[2, 2] = 1300          # pixel (2, 2): 1.0 m now, 1.3 m before: drift 0.3 >= 0.2
    both = m.project(cur, K, T)
    assert len(both) == 2
    # same pose: every point reprojects onto its own pixel; (3, 5) agrees with the last frame, (2, 2) drifted
    assert m.project(cur, K, T, last=(last, T)) == [both[1]]
    last[2, 2] = 1100                             # drift 0.1 < 0.2: kept
    assert m.project(cur, K, T, last=(last, T)) == both
    # the last camera stood 4 m further along +x... the points are BEHIND it: z < 0 there, uu = x * fx / z + cx; with the last camera
    # 10 m to the side they reproject far outside the image: "new point", kept (:404-407) whatever the last image holds
    Tl = FO.pose((CAM[0], CAM[1] + 10.0, CAM[2]), 0.0, 0.0)
    assert m.project(cur, K, T, last=(np.full((8, 8), 9000, dtype=np.uint16), Tl)) == both
    # the first filtered frame projects nothing and is only remembered (:360-361, :423-424); the second is filtered against it
    m.fuse(cur, K, T, shift_filter=True)
    assert np.all(m.buffer == 0.5) and m.stats["rays"] == 0 and m.has_first_depth and np.array_equal(m.last[0], cur)
    m.fuse(cur, K, T, shift_filter=True)
    assert m.stats["rays"] == 2 and np.count_nonzero(m.buffer != 0.5) > 2
    assert FO.inverse3([[2.0, 0, 0], [0, 4.0, 0], [0, 0, 0.5]]) == [[0.5, 0, 0], [0, 0.25, 0], [0, 0, 2.0]]
    assert FO.inverse3([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0, 0, 1.0]]) is None


def test_the_steps_scene_needs_more_than_one_round():
    """What tests/test_gpu_occmap_fusion.py relies on for its max_rounds = 1 case."""
    m = FO.FusionOracle(**FO.TEST_GEO, **FO.LAUNCH_CLAMPS)
    before = m.buffer.copy()
    T = FO.pose(FO.PLACEMENTS["middle"])
    pts = m.project(FO.scene("steps"), FO.TEST_K, T)
    assert m.raycast_relaxed(pts, T[:3, 3], max_rounds=1) == (None, -1) and np.array_equal(m.buffer, before)
    assert m.raycast_relaxed(pts, T[:3, 3])[1] >= 2


# ---- the boundary ----
def _map_desc():
    m = solver.OccMap()
    m.origin[:] = (-20.0, -20.0, -1.0); m.map_size[:] = (40.0, 40.0, 5.0); m.resolution = 0.1; m.grid[:] = (400, 400, 50)
    m.clamp_min_log, m.clamp_max_log, m.min_occupancy_log = -1.0, 2.0, 1.70
    m.local_radius[:] = (6.0, 6.0, 3.0)
    m.log_odds = 0x1000; m.occ = 0x2000   # never dereferenced on the host; nothing is launched in these tests
    return m


def _fuse_desc(**kw):
    f = solver.OccMapFuse()
    f.rows, f.cols = 480, 640
    f.depth, f.last_depth, f.status = 0x3000, None, 0x4000
    f.K[:] = (380.0, 0.0, 320.0, 0.0, 380.0, 240.0, 0.0, 0.0, 1.0)
    f.T_wc[:] = [float(v) for v in FO.pose((0.0, 0.0, 1.0)).ravel()]
    f.last_T_wc[:] = [float(v) for v in FO.pose((0.1, 0.0, 1.0)).ravel()]
    for k, v in solver.OCCMAP_FUSE_DEFAULTS.items():
        setattr(f, k, v)
    for k, v in kw.items():
        if isinstance(v, dict):
            for i, x in v.items():
                getattr(f, k)[i] = x
        else:
            setattr(f, k, v)
    return f


def _fuse(lib, m, f, ws_bytes, fws_bytes, ws=0x5000, fws=0x100000):
    return lib.frp_nmpc_occmap_fuse_depth(ctypes.byref(m) if m is not None else None, ctypes.byref(f) if f is not None else None,
                                          ctypes.c_void_p(ws), ws_bytes, ctypes.c_void_p(fws), fws_bytes, None)


def test_symbols_struct_layout_and_abi_version(tmp_path):
    lib = solver.lib()
    for n in ("frp_nmpc_occmap_fuse_workspace_bytes", "frp_nmpc_occmap_fuse_depth"):
        assert hasattr(lib, n) and n in solver.FUSE_EXPORTS
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    assert '#include "frp_nmpc_occmap_fuse.h"' in hdr and "#define FRP_NMPC_ABI_VERSION 7" in hdr   # no existing struct changed
    lines = [f'_Static_assert(sizeof(frp_nmpc_occmap_fuse) == {ctypes.sizeof(solver.OccMapFuse)}, "size");']
    for fld, _ in solver.OccMapFuse._fields_:
        lines.append(f'_Static_assert(offsetof(frp_nmpc_occmap_fuse, {fld}) == {getattr(solver.OccMapFuse, fld).offset}, "{fld}");')
    lines.append('_Static_assert(FRP_OCCMAP_FUSE_DEFAULT_ROUNDS == 128, "default rounds");')
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "frp_nmpc.h"\n' + "\n".join(lines) + "\nint main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "layout.o")])


NAN, INF = float("nan"), float("inf")
REFUSED = {
    "non-finite K": dict(K={0: NAN}), "infinite K": dict(K={5: INF}), "non-finite T_wc": dict(T_wc={3: NAN}), "infinite T_wc": dict(T_wc={0: -INF}),
    "singular last rotation": dict(last_depth=0x6000, last_T_wc={0: 0.0, 1: 0.0, 2: 0.0}),
    "non-finite last_T_wc": dict(last_depth=0x6000, last_T_wc={7: NAN}),
    "skip_pixel 0": dict(skip_pixel=0), "negative margin": dict(depth_filter_margin=-1), "depth_scale 0": dict(depth_scale=0.0),
    "negative depth_scale": dict(depth_scale=-1000.0), "NaN depth_scale": dict(depth_scale=NAN),
    "max_ray_length below min_ray_length": dict(min_ray_length=2.0, max_ray_length=1.0),
    "step bound above 4096": dict(max_ray_length=136.5),          # 3 * (ceil(136.5 / 0.1) + 2) = 4101
    "max_rounds negative": dict(max_rounds=-1), "max_rounds above 255": dict(max_rounds=256), "no rows": dict(rows=0),
    "NaN tolerance": dict(depth_filter_tolerance=NAN),
}


def test_argument_errors_come_before_any_launch():
    lib = solver.lib()
    m, good = _map_desc(), _fuse_desc()
    ws = lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    need = lib.frp_nmpc_occmap_fuse_workspace_bytes(ctypes.byref(m), ctypes.byref(good))
    # 239 x 319 scanned pixels (3 doubles + 3 ints each) and four int arrays over the largest ray box, (2 * 60 + 8)^2 x 50 voxels
    N, nb = 239 * 319, 128 * 128 * 50
    assert N * 36 + nb * 16 <= need <= N * 36 + nb * 16 + 264 * 4 + 9 * 256
    assert lib.frp_nmpc_occmap_fuse_workspace_bytes(ctypes.byref(m), ctypes.byref(_fuse_desc(max_ray_length=136.0))) > need   # step bound 4092: accepted
    for what, kw in REFUSED.items():
        f = _fuse_desc(**kw)
        assert lib.frp_nmpc_occmap_fuse_workspace_bytes(ctypes.byref(m), ctypes.byref(f)) == 0, what
        assert _fuse(lib, m, f, ws, need) == FRP_ERR_ARG, what
    assert lib.frp_nmpc_occmap_fuse_workspace_bytes(None, ctypes.byref(good)) == 0 and lib.frp_nmpc_occmap_fuse_workspace_bytes(ctypes.byref(m), None) == 0
    bad_map = _map_desc(); bad_map.grid[2] = 51
    assert lib.frp_nmpc_occmap_fuse_workspace_bytes(ctypes.byref(bad_map), ctypes.byref(good)) == 0
    assert _fuse(lib, bad_map, good, ws, need) == FRP_ERR_ARG and _fuse(lib, None, good, ws, need) == FRP_ERR_ARG and _fuse(lib, m, None, ws, need) == FRP_ERR_ARG
    assert _fuse(lib, m, good, ws - 1, need) == FRP_ERR_ARG and _fuse(lib, m, good, ws, need - 1) == FRP_ERR_ARG      # short workspaces
    assert _fuse(lib, m, good, ws, need, ws=0) == FRP_ERR_ARG and _fuse(lib, m, good, ws, need, fws=0) == FRP_ERR_ARG
    assert _fuse(lib, m, _fuse_desc(depth=None), ws, need) == FRP_ERR_ARG and _fuse(lib, m, _fuse_desc(status=None), ws, need) == FRP_ERR_ARG
    # a singular last_T_wc is only looked at with last_depth
    assert lib.frp_nmpc_occmap_fuse_workspace_bytes(ctypes.byref(m), ctypes.byref(_fuse_desc(last_T_wc={0: NAN}))) == need


def _has_gpu():
    try:
        return solver.lib().frp_nmpc_device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the behaviour of a machine WITHOUT a device")
def test_fuse_reports_no_device():
    lib = solver.lib()
    m = _map_desc()
    ws = lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    for f in (_fuse_desc(), _fuse_desc(last_depth=0x6000), _fuse_desc(max_rounds=1)):
        need = lib.frp_nmpc_occmap_fuse_workspace_bytes(ctypes.byref(m), ctypes.byref(f))
        assert need > 0 and _fuse(lib, m, f, ws, need) == FRP_ERR_NO_DEVICE
