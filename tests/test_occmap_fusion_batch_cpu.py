"""CPU tests of batched depth fusion (include/frp_nmpc_occmap_fuse_batch.h): the boundary as far as it exists without a device, and
the conditions on the inputs of tests/test_gpu_occmap_fusion_batch.py, checked with the oracle so that the GPU tests cannot pass
for the wrong reason."""
import ctypes
import os
import subprocess

import pytest

from forces_resilient_planner_amd import solver
from tests import occmap_fusion_batch_cases as C
from tests import occmap_fusion_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRP_ERR_NO_DEVICE, FRP_ERR_ARG = -1001, -1003
NAN, INF = float("nan"), float("inf")
F = 4


def _map_desc():
    m = solver.OccMap()
    m.origin[:] = (-20.0, -20.0, -1.0); m.map_size[:] = (40.0, 40.0, 5.0); m.resolution = 0.1; m.grid[:] = (400, 400, 50)
    m.clamp_min_log, m.clamp_max_log, m.min_occupancy_log = -1.0, 2.0, 1.70
    m.local_radius[:] = (6.0, 6.0, 3.0)
    m.log_odds = 0x1000; m.occ = 0x2000   # never dereferenced on the host; nothing is launched in these tests
    return m


def _params(f, **kw):
    f.rows, f.cols = 480, 640
    f.K[:] = (380.0, 0.0, 320.0, 0.0, 380.0, 240.0, 0.0, 0.0, 1.0)
    for k, v in solver.OCCMAP_FUSE_DEFAULTS.items():
        setattr(f, k, v)
    for k, v in kw.items():
        if isinstance(v, dict):
            for i, x in v.items():
                getattr(f, k)[i] = x
        else:
            setattr(f, k, v)
    return f


def _batch_desc(**kw):
    """F frames behind fake device pointers: nothing behind them is ever read on the host."""
    f = solver.OccMapFuseBatch()
    f.frames = F
    f.depth, f.last_depth, f.T_wc, f.last_T_wc, f.active, f.status = 0x3000000, None, 0x7000, None, None, 0x4000
    return _params(f, **kw)


def _single_desc(**kw):
    f = solver.OccMapFuse()
    f.depth, f.last_depth, f.status = 0x3000000, None, 0x4000
    f.T_wc[:] = [float(v) for v in FO.pose((0.0, 0.0, 1.0)).ravel()]
    return _params(f, **kw)


def _fuse(lib, m, f, ws_bytes, fws_bytes, ws=0x5000, fws=0x10000000):
    return lib.frp_nmpc_occmap_fuse_depth_batch(ctypes.byref(m) if m is not None else None, ctypes.byref(f) if f is not None else None,
                                                ctypes.c_void_p(ws), ws_bytes, ctypes.c_void_p(fws), fws_bytes, None)


def _need(lib, m, f):
    return lib.frp_nmpc_occmap_fuse_batch_workspace_bytes(ctypes.byref(m) if m is not None else None, ctypes.byref(f) if f is not None else None)


@pytest.mark.parametrize("header", ["frp_nmpc.h", "frp_nmpc_occmap_fuse_batch.h"])
def test_symbols_struct_layout_and_abi_version(tmp_path, header):
    lib = solver.lib()
    assert solver.FUSE_BATCH_EXPORTS == ["frp_nmpc_occmap_fuse_batch_workspace_bytes", "frp_nmpc_occmap_fuse_depth_batch"]
    for n in solver.FUSE_BATCH_EXPORTS:
        assert hasattr(lib, n)
    assert solver.FUSE_EXPORTS == ["frp_nmpc_occmap_fuse_workspace_bytes", "frp_nmpc_occmap_fuse_depth"]
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    assert '#include "frp_nmpc_occmap_fuse_batch.h"' in hdr and "#define FRP_NMPC_ABI_VERSION 7" in hdr and lib.frp_nmpc_abi_version() == 7
    lines = [f'_Static_assert(sizeof(frp_nmpc_occmap_fuse_batch) == {ctypes.sizeof(solver.OccMapFuseBatch)}, "size");']
    for fld, _ in solver.OccMapFuseBatch._fields_:
        lines.append(f'_Static_assert(offsetof(frp_nmpc_occmap_fuse_batch, {fld}) == {getattr(solver.OccMapFuseBatch, fld).offset}, "{fld}");')
    lines.append(f'_Static_assert(FRP_OCCMAP_FUSE_REFUSED == {solver.OCCMAP_FUSE_REFUSED} && FRP_OCCMAP_FUSE_REFUSED == -256, "refused");')
    lines.append(f'_Static_assert(FRP_OCCMAP_FUSE_MAX_FRAMES == {solver.OCCMAP_FUSE_MAX_FRAMES}, "frames cap");')
    lines.append('_Static_assert(FRP_NMPC_ABI_VERSION == 7 && FRP_OCCMAP_FUSE_DEFAULT_ROUNDS == 128, "version, default rounds");')
    # the single-frame struct did not change, through either header
    lines.append(f'_Static_assert(sizeof(frp_nmpc_occmap_fuse) == {ctypes.sizeof(solver.OccMapFuse)}, "single-frame size");')
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stddef.h>\n#include "{header}"\n' + "\n".join(lines) + "\nint main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "layout.o")])


# everything the single-frame call refuses that does not involve a pose, and what the batch adds
REFUSED = {
    "non-finite K": dict(K={0: NAN}), "infinite K": dict(K={5: INF}),
    "skip_pixel 0": dict(skip_pixel=0), "negative margin": dict(depth_filter_margin=-1), "depth_scale 0": dict(depth_scale=0.0),
    "negative depth_scale": dict(depth_scale=-1000.0), "NaN depth_scale": dict(depth_scale=NAN),
    "max_ray_length below min_ray_length": dict(min_ray_length=2.0, max_ray_length=1.0),
    "step bound above 4096": dict(max_ray_length=136.5),          # 3 * (ceil(136.5 / 0.1) + 2) = 4101
    "max_rounds negative": dict(max_rounds=-1), "max_rounds above 255": dict(max_rounds=256), "no rows": dict(rows=0), "no cols": dict(cols=0),
    "NaN tolerance": dict(depth_filter_tolerance=NAN), "NaN hit": dict(prob_hit_log=NAN),
    "no frames": dict(frames=0), "negative frames": dict(frames=-1), "frames above the cap": dict(frames=solver.OCCMAP_FUSE_MAX_FRAMES + 1),
}
# refused by the call for a pointer; the size function does not look at pointers
REFUSED_POINTERS = {"null depth": dict(depth=None), "null T_wc": dict(T_wc=None), "null status": dict(status=None),
                    "last_depth without last_T_wc": dict(last_depth=0x6000000, last_T_wc=None)}


def test_argument_errors_come_before_any_launch():
    lib = solver.lib()
    m, good = _map_desc(), _batch_desc()
    ws = lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    need = _need(lib, m, good)
    assert need > 0
    for what, kw in REFUSED.items():
        f = _batch_desc(**kw)
        assert _need(lib, m, f) == 0, what
        assert _fuse(lib, m, f, ws, 1 << 40) == FRP_ERR_ARG, what
    for what, kw in REFUSED_POINTERS.items():
        f = _batch_desc(**kw)
        assert _need(lib, m, f) == need, what
        assert _fuse(lib, m, f, ws, need) == FRP_ERR_ARG, what
    assert _need(lib, None, good) == 0 and _need(lib, m, None) == 0
    bad_map = _map_desc(); bad_map.grid[2] = 51
    assert _need(lib, bad_map, good) == 0
    assert _fuse(lib, bad_map, good, ws, need) == FRP_ERR_ARG and _fuse(lib, None, good, ws, need) == FRP_ERR_ARG and _fuse(lib, m, None, ws, need) == FRP_ERR_ARG
    assert _fuse(lib, m, good, ws - 1, need) == FRP_ERR_ARG and _fuse(lib, m, good, ws, need - 1) == FRP_ERR_ARG      # short workspaces
    assert _fuse(lib, m, good, ws, need, ws=0) == FRP_ERR_ARG and _fuse(lib, m, good, ws, need, fws=0) == FRP_ERR_ARG
    assert _fuse(lib, m, good, ws, need + 8, fws=0x10000004) == FRP_ERR_ARG                                            # misaligned
    # the cap itself, and the filtered form with both of its arrays, are accepted as descriptions
    assert _need(lib, m, _batch_desc(frames=solver.OCCMAP_FUSE_MAX_FRAMES)) > need
    assert _need(lib, m, _batch_desc(last_depth=0x6000000, last_T_wc=0x8000)) == need


def test_a_nan_pose_is_not_a_host_refusal(tmp_path):
    """The poses live on the device: the host must not (and cannot) look at them.  A real host array holding NaN poses stands behind
    the pointer here -- a host that read it would refuse, as the single-frame call does for its host poses."""
    lib = solver.lib()
    m = _map_desc()
    need = _need(lib, m, _batch_desc())
    poses = (ctypes.c_double * (16 * F))(*([NAN] * (16 * F)))
    addr = ctypes.addressof(poses)
    assert _need(lib, m, _batch_desc(T_wc=addr)) == need
    assert _need(lib, m, _batch_desc(T_wc=addr, last_depth=0x6000000, last_T_wc=addr)) == need
    single = _single_desc(T_wc={3: NAN})                               # ... which the single-frame call refuses on the host
    assert lib.frp_nmpc_occmap_fuse_workspace_bytes(ctypes.byref(m), ctypes.byref(single)) == 0


def test_workspace_grows_with_the_frames():
    lib = solver.lib()
    m = _map_desc()
    one = lib.frp_nmpc_occmap_fuse_workspace_bytes(ctypes.byref(m), ctypes.byref(_single_desc()))
    assert one > 0
    prev = 0
    for frames in (1, 2, 3, 16, solver.OCCMAP_FUSE_MAX_FRAMES):
        need = _need(lib, m, _batch_desc(frames=frames))
        assert need > prev and need >= frames * one, frames
        assert need <= frames * (one + 1024) + 256, frames             # F slices and a descriptor of a few hundred bytes per frame
        prev = need
    # the size does not depend on the filter, the mask or max_rounds, as for the single-frame call
    assert _need(lib, m, _batch_desc(max_rounds=7, active=0x9000)) == _need(lib, m, _batch_desc())


def _has_gpu():
    try:
        return solver.lib().frp_nmpc_device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the behaviour of a machine WITHOUT a device")
def test_fuse_batch_reports_no_device():
    lib = solver.lib()
    m = _map_desc()
    ws = lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    for f in (_batch_desc(), _batch_desc(last_depth=0x6000000, last_T_wc=0x8000), _batch_desc(max_rounds=1, active=0x9000, frames=1)):
        need = _need(lib, m, f)
        assert need > 0 and _fuse(lib, m, f, ws, need) == FRP_ERR_NO_DEVICE


def test_the_python_binding_exists():
    assert callable(solver.OccupancyMap.fuse_depth_batch)
    assert ctypes.sizeof(solver.OccMapFuseBatch) > 0 and solver.OccMapFuseBatch._fields_[0][0] == "frames"


# ---- the conditions the GPU tests rely on ----
def test_the_order_of_the_six_frames_matters():
    """Test 2 of the GPU file tells an ordered update from an unordered one only if the order changes the result."""
    fwd, st = C.six_in_order()
    rev, st_rev = C.six_reversed()
    assert fwd.buffer.tobytes() != rev.buffer.tobytes()
    assert st_rev == st[::-1]                                          # rounds and rays are a frame's own, whatever came before it
    assert all(s[0] >= 2 and s[1] > 100 for s in st)
    # the chain of this file's helper is the oracle's own fuse(), frame after frame
    assert C.six_by_fuse(False).buffer.tobytes() == fwd.buffer.tobytes()
    filt, st_f = C.six_filtered()
    assert C.six_by_fuse(True).buffer.tobytes() == filt.buffer.tobytes()
    assert st_f[0] is None and all(s[1] > 0 for s in st_f[1:]) and filt.buffer.tobytes() != fwd.buffer.tobytes()


def test_the_round_counts_straddle_the_cap():
    _, st = C.six_in_order()
    rounds = [s[0] for s in st]
    print("rounds of the six frames:", rounds)
    assert rounds == [12, 11, 14, 10, 10, 12]
    assert min(rounds) <= C.STRADDLE_CAP < max(rounds)
    capped, st_c = C.chain(C.six_frames(), cap=C.STRADDLE_CAP)
    assert [s[0] for s in st_c] == [-11, 11, -11, 10, 10, -11]
    assert [s[1] for s in st_c] == [s[1] for s in st]
    only, _ = C.chain(C.six_frames(), skip={0, 2, 5})
    assert capped.buffer.tobytes() == only.buffer.tobytes() != C.six_in_order()[0].buffer.tobytes()


def test_the_far_camera_has_an_empty_ray_box_and_still_casts_rays():
    om = C.oracle()
    assert om.ray_box([float(v) for v in C.FAR_POSE[:3, 3]]) == [64, 0, 0, 64, 64, 32]
    f = C.six_frames()
    before = om.buffer.copy()
    pts = om.project(f[1][0], C.K, C.FAR_POSE)
    _, rounds = om.raycast_relaxed(pts, C.FAR_POSE[:3, 3])
    assert rounds == 1 and om.stats["rays"] > 100 and om.box_skips == 0 and (om.buffer == before).all()
