"""CPU tests of the depth renderer (include/frp_nmpc_occmap_render.h): the boundary as far as it exists without a device, the
specification (tests/occmap_render_oracle.py) against closed forms, and the round trip render -> FusionOracle.project on the scenes
the GPU tests use, so that those cannot pass for the wrong reason."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from forces_resilient_planner_amd import solver, workloads
from tests import occmap_fusion_oracle as FO
from tests import occmap_render_cases as C
from tests import occmap_render_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRP_ERR_NO_DEVICE, FRP_ERR_ARG = -1001, -1003
NAN, INF = float("nan"), float("inf")
NAMES = ["frp_nmpc_occmap_render_depth", "frp_nmpc_occmap_camera_poses"]


# ---- header and exports ----
def _layout_lines():
    lines = [f'_Static_assert(sizeof(frp_nmpc_occmap_render) == {ctypes.sizeof(solver.OccMapRender)}, "size");']
    for fld, _ in solver.OccMapRender._fields_:
        lines.append(f'_Static_assert(offsetof(frp_nmpc_occmap_render, {fld}) == {getattr(solver.OccMapRender, fld).offset}, "{fld}");')
    lines.append('_Static_assert(FRP_NMPC_ABI_VERSION == 7 && FRP_OCCMAP_FUSE_MAX_FRAMES == 64 && FRP_OCCMAP_FUSE_REFUSED == -256, "unchanged");')
    # no existing struct changed
    for name, mirror in (("frp_nmpc_occmap", solver.OccMap), ("frp_nmpc_occmap_fuse", solver.OccMapFuse), ("frp_nmpc_occmap_fuse_batch", solver.OccMapFuseBatch)):
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(mirror)}, "{name}");')
    return lines


@pytest.mark.parametrize("header", ["frp_nmpc.h", "frp_nmpc_occmap_render.h"])
@pytest.mark.parametrize("lang", ["c99", "c11", "c++"])
def test_the_header_compiles_alone_and_through_frp_nmpc_h(tmp_path, header, lang):
    """Strict C99 (the boundary is a C ABI), C11 with the struct's layout against the ctypes mirror, and C++."""
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    assert '#include "frp_nmpc_occmap_render.h"' in hdr and "#define FRP_NMPC_ABI_VERSION 7" in hdr
    own = open(os.path.join(ROOT, "include", "frp_nmpc_occmap_render.h")).read()
    for n in NAMES:
        assert n + "(" in own and n + "(" not in hdr
    use = ("int use(const frp_nmpc_occmap *m, const frp_nmpc_occmap_render *r, void *ws, double *T) {\n"
           "  const double T_bc[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};\n"
           "  return frp_nmpc_occmap_render_depth(m, r, ws, 0, 0) + frp_nmpc_occmap_camera_poses(0, 0, T_bc, T, 0); }\n")
    layout = "\n".join(_layout_lines())
    if lang == "c++":
        src = tmp_path / "layout.cpp"
        src.write_text(f'#include <cstddef>\n#include "{header}"\n{layout.replace("_Static_assert", "static_assert")}\n{use}int main() {{ return 0; }}\n')
        cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-invalid-offsetof"]
    else:
        src = tmp_path / "layout.c"
        src.write_text(f'#include <stddef.h>\n#include "{header}"\n{layout if lang == "c11" else ""}\n{use}int main(void) {{ return 0; }}\n')
        cmd = ["gcc", "-std=" + lang, "-pedantic", "-Wall", "-Werror"]
    subprocess.check_call(cmd + ["-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(src) + ".o"])


def test_the_two_symbols_are_exported_and_checked_at_load():
    lib = solver.lib()
    assert solver.RENDER_EXPORTS == NAMES
    for n in NAMES:
        assert hasattr(lib, n), n
    assert lib.frp_nmpc_abi_version() == 7
    assert callable(solver.OccupancyMap.render_depth) and callable(solver.OccupancyMap.camera_poses)


def _map_desc():
    m = solver.OccMap()
    m.origin[:] = (-20.0, -20.0, -1.0); m.map_size[:] = (40.0, 40.0, 5.0); m.resolution = 0.1; m.grid[:] = (400, 400, 50)
    m.clamp_min_log, m.clamp_max_log, m.min_occupancy_log = -1.0, 2.0, 1.70
    m.local_radius[:] = (6.0, 6.0, 3.0)
    m.log_odds = 0x1000; m.occ = 0x2000   # never dereferenced on the host; nothing is launched in these tests
    return m


def _desc(**kw):
    """Fake device pointers: nothing behind them is ever read on the host."""
    r = solver.OccMapRender()
    r.frames, r.rows, r.cols = 4, 480, 640
    r.T_wc, r.active, r.depth, r.voxel, r.status = 0x7000, None, 0x3000000, None, 0x4000
    r.K[:] = (380.0, 0.0, 320.0, 0.0, 380.0, 240.0, 0.0, 0.0, 1.0)
    r.depth_scale, r.max_range = 1000.0, 6.0
    for k, v in kw.items():
        if isinstance(v, dict):
            for i, x in v.items():
                getattr(r, k)[i] = x
        else:
            setattr(r, k, v)
    return r


def _render(lib, m, r, ws_bytes, ws=0x5000):
    return lib.frp_nmpc_occmap_render_depth(ctypes.byref(m) if m is not None else None, ctypes.byref(r) if r is not None else None,
                                            ctypes.c_void_p(ws), ws_bytes, None)


REFUSED = {
    "null T_wc": dict(T_wc=None), "null depth": dict(depth=None), "null status": dict(status=None),
    "no frames": dict(frames=0), "negative frames": dict(frames=-1), "frames above the cap": dict(frames=solver.OCCMAP_FUSE_MAX_FRAMES + 1),
    "no rows": dict(rows=0), "no cols": dict(cols=0), "negative rows": dict(rows=-480), "more than 2^24 pixels": dict(rows=4097, cols=4096),
    "NaN K": dict(K={2: NAN}), "infinite K": dict(K={5: INF}), "fx 0": dict(K={0: 0.0}), "fy 0": dict(K={4: 0.0}),
    "depth_scale 0": dict(depth_scale=0.0), "negative depth_scale": dict(depth_scale=-1000.0), "NaN depth_scale": dict(depth_scale=NAN),
    "max_range 0": dict(max_range=0.0), "negative max_range": dict(max_range=-6.0), "NaN max_range": dict(max_range=NAN),
    "infinite max_range": dict(max_range=INF),
    "step bound above 4096": dict(max_range=136.5),                    # 3 * (ceil(136.5 / 0.1) + 2) = 4101
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_argument_errors_come_before_any_launch(what):
    lib = solver.lib()
    m = _map_desc()
    ws = lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    assert _render(lib, m, _desc(**REFUSED[what]), ws) == FRP_ERR_ARG


def test_a_bad_map_a_null_description_and_a_short_workspace_are_refused():
    lib = solver.lib()
    m, good = _map_desc(), _desc()
    ws = lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    bad_map = _map_desc(); bad_map.grid[2] = 51
    assert _render(lib, bad_map, good, ws) == FRP_ERR_ARG and _render(lib, None, good, ws) == FRP_ERR_ARG
    assert _render(lib, m, None, ws) == FRP_ERR_ARG
    assert _render(lib, m, good, ws - 1) == FRP_ERR_ARG and _render(lib, m, good, ws, ws=0) == FRP_ERR_ARG
    # camera_poses
    T_bc = (ctypes.c_double * 16)(*np.eye(4).ravel())
    P = ctypes.c_void_p
    assert lib.frp_nmpc_occmap_camera_poses(-1, P(0x9000), T_bc, P(0xa000), None) == FRP_ERR_ARG
    assert lib.frp_nmpc_occmap_camera_poses(4, None, T_bc, P(0xa000), None) == FRP_ERR_ARG
    assert lib.frp_nmpc_occmap_camera_poses(4, P(0x9000), T_bc, None, None) == FRP_ERR_ARG
    assert lib.frp_nmpc_occmap_camera_poses(4, P(0x9000), None, P(0xa000), None) == FRP_ERR_ARG


def _has_gpu():
    try:
        return solver.lib().frp_nmpc_device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the behaviour of a machine WITHOUT a device")
def test_valid_arguments_report_no_device():
    lib = solver.lib()
    m = _map_desc()
    ws = lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    # the limits themselves are accepted: the frame cap, 2^24 pixels, the largest step bound (3 * (1363 + 2) = 4095)
    for r in (_desc(), _desc(active=0x9000, voxel=0x6000000), _desc(frames=solver.OCCMAP_FUSE_MAX_FRAMES), _desc(rows=4096, cols=4096),
              _desc(max_range=136.3), _desc(frames=1, rows=1, cols=1)):
        assert _render(lib, m, r, ws) == FRP_ERR_NO_DEVICE
    # the poses are on the device: a host array of NaN behind the pointer is not looked at
    poses = (ctypes.c_double * 64)(*([NAN] * 64))
    assert _render(lib, m, _desc(T_wc=ctypes.addressof(poses)), ws) == FRP_ERR_NO_DEVICE
    T_bc = (ctypes.c_double * 16)(*np.eye(4).ravel())
    assert lib.frp_nmpc_occmap_camera_poses(4, ctypes.c_void_p(0x9000), T_bc, ctypes.c_void_p(0xa000), None) == FRP_ERR_NO_DEVICE
    assert lib.frp_nmpc_occmap_camera_poses(0, None, T_bc, None, None) == FRP_ERR_NO_DEVICE


# ---- the specification against closed forms ----
GEO = C.GEO["low"]
D_WALL = 1.2
CAM = (-1.0, 1.0, 1.05)                       # on a voxel face in x, mid-voxel in y and z: voxel (10, 18, 10)


def _wall_map(distance):
    """A one-voxel-thick wall perpendicular to x whose near face is `distance` in front of CAM."""
    occ = np.zeros(C.GRID["low"], dtype=np.uint8)
    ix = int(round((CAM[0] + distance - GEO["origin"][0]) / 0.1))
    occ[ix, :, :] = 1
    return RO.RenderOracle(occ, GEO["origin"], GEO["resolution"]), ix


def test_an_empty_world_gives_all_zeros():
    o = RO.RenderOracle(np.zeros(C.GRID["low"], dtype=np.uint8), GEO["origin"], GEO["resolution"])
    for T in (C.pose_of("middle"), C.pose_of("near_face"), C.pose_of(C.OUTSIDE), C.axis_pose(CAM)):
        d, vox, seg, st, steps = o.render(T, C.K_INT["small"], 24, 32, C.MAX_RANGE)
        assert not d.any() and (vox == -1).all() and not seg.any() and st == [1, 0] and steps > 0


def test_a_wall_at_a_known_distance():
    o, ix = _wall_map(D_WALL)
    assert ix == 22
    rows, cols = C.IMAGES["small"]
    Km = C.K_INT["small"]
    d, vox, seg, st, _ = o.render(C.axis_pose(CAM), Km, rows, cols, C.MAX_RANGE)
    v0, u0 = int(Km[1, 2]), int(Km[0, 2])                              # the central pixel: d_cam = (0, 0, 1), two zero components of d_w
    assert d[v0, u0] == round((D_WALL + 0.05) * 1000) == 1250
    assert vox[v0, u0] == (22 * 40 + 18) * 20 + 10
    assert abs(seg[v0, u0] - 0.1) < 1e-12
    # the wall is perpendicular to the optical axis and s is the camera-z depth: every ray enters it at 1.2 and leaves the voxel it
    # entered at 1.3 at the latest (an oblique ray leaves it sideways, into the wall's next voxel, before that)
    assert st == [1, rows * cols] and (d >= 1200).all() and (d <= 1250).all() and (seg <= 0.1 + 1e-12).all()
    assert (vox // (40 * 20) == 22).all()
    # ... and each pixel's voxel is the one its ray enters the wall in: y = CAM.y - s * (u - cx) / fx, z = CAM.z - s * (v - cy) / fy at s = 1.2
    for v, u in ((0, 0), (23, 31), (5, 20), (v0, u0 + 1), (v0 - 1, u0)):
        y, z = CAM[1] - 1.2001 * (u - Km[0, 2]) / Km[0, 0], CAM[2] - 1.2001 * (v - Km[1, 2]) / Km[1, 1]
        want = (22 * 40 + int(math.floor((y - GEO["origin"][1]) / 0.1))) * 20 + int(math.floor(z / 0.1))
        assert vox[v, u] == want, (v, u)
    # the rays along the camera's axes stay in the central voxel's row or column: they read the closed form too
    assert d[v0, u0 + 1] == 1250 and d[v0 - 1, u0] == 1250


def test_a_wall_beyond_max_range_gives_zero():
    o, _ = _wall_map(D_WALL)
    Km = C.K_INT["small"]
    d, vox, _, st, _ = o.render(C.axis_pose(CAM), Km, 24, 32, 1.15)     # the wall's entry face at 1.2 m is past 1.15 m on every ray
    assert not d.any() and (vox == -1).all() and st == [1, 0]
    # just inside: the central ray (|d_w| = 1) enters at 1.2 <= 1.25; the corner rays are longer by |d_w| = 1.33 and do not
    d, vox, _, st, _ = o.render(C.axis_pose(CAM), Km, 24, 32, 1.25)
    assert d[12, 16] == 1250 and d[0, 0] == 0 and 0 < st[1] < 24 * 32


def test_a_camera_inside_an_occupied_voxel_sees_nothing():
    o, ix = _wall_map(D_WALL)
    inside = (GEO["origin"][0] + (ix + 0.5) * 0.1, CAM[1], CAM[2])
    for T in (C.axis_pose(inside), FO.pose(inside)):
        d, vox, _, st, steps = o.render(T, C.K_INT["small"], 24, 32, C.MAX_RANGE)
        assert not d.any() and (vox == -1).all() and st == [1, 0] and steps == 0
    # one voxel further it looks away from the wall and into nothing
    d, _, _, st, _ = o.render(C.axis_pose((inside[0] + 0.1, CAM[1], CAM[2])), C.K_INT["small"], 24, 32, C.MAX_RANGE)
    assert not d.any() and st == [1, 0]


def test_a_non_finite_pose_is_refused_and_a_value_above_65535_is_no_return():
    o, _ = _wall_map(D_WALL)
    T = C.axis_pose(CAM); T[2, 0] = INF
    d, vox, _, st, _ = o.render(T, C.K_INT["small"], 24, 32, C.MAX_RANGE)
    assert st == [RO.REFUSED, 0] and RO.REFUSED == solver.OCCMAP_FUSE_REFUSED and not d.any() and (vox == -1).all()
    d, vox, _, st, _ = o.render(C.axis_pose(CAM), C.K_INT["small"], 24, 32, C.MAX_RANGE, depth_scale=60000.0)   # 1.25 * 60000 = 75000
    assert not d.any() and (vox == -1).all() and st == [1, 0]
    d, _, _, st, _ = o.render(C.axis_pose(CAM), C.K_INT["small"], 24, 32, C.MAX_RANGE, depth_scale=50000.0)
    assert d[12, 16] == 62500 and (d >= 60000).all() and st == [1, 24 * 32]


# ---- the round trip on the CPU ----
@pytest.mark.parametrize("placement", ["middle", "near_face"])
@pytest.mark.parametrize("scene", ["pillars", "wall"])
def test_a_rendered_image_projects_back_into_the_voxels_it_came_from(scene, placement):
    image = "large"
    d, vox, seg, st, _ = C.rendered(scene, "low", image, placement)
    returns = int((d != 0).sum())
    assert st == [1, returns] and returns > 200, (scene, placement, returns)
    assert ((vox >= 0) == (d != 0)).all()
    occ = C.world_occ(scene, "low").reshape(-1)
    assert occ[vox[d != 0]].all()                                      # every return is an occupied voxel of the world
    ex = C.excluded(d, seg)
    print(f"{scene} {placement}: {returns} returns, {int(ex.sum())} below 2 mm ({ex.sum() / returns:.4f})")
    assert ex.sum() <= 0.02 * returns
    back = C.projected_voxels(d, C.K[image], C.pose_of(placement), "low")
    keep = (d != 0) & ~ex
    assert np.array_equal(back[keep], vox[keep])


# ---- camera_poses ----
def test_the_camera_pose_statement_against_the_model_rotation():
    rng = np.random.default_rng(5)
    st = workloads._random_states(rng, 64)
    st[:, 6:8] = rng.uniform(-1.2, 1.2, (64, 2))                        # up to the model's attitude bound of 0.4 pi
    T_bc = FO.pose((0.05, -0.02, 0.1), yaw=0.1, pitch=-0.2)             # the camera convention of the fusion tests on the body
    got = RO.camera_poses(st, T_bc)
    T_wb = np.tile(np.eye(4), (64, 1, 1))
    T_wb[:, :3, :3] = workloads._rot(st[:, 6:9]); T_wb[:, :3, 3] = st[:, 0:3]
    want = T_wb @ T_bc
    # the same products summed in another order (numpy's matmul): a few ulp -- of 1 for the rotation, of 8 for positions up to 5.3 m
    assert np.abs(got - want)[:, :3, :3].max() < 4 * 2.0 ** -52 and np.abs(got - want)[:, :3, 3].max() < 4 * 2.0 ** -50
    assert np.array_equal(got[:, 3], np.tile(T_bc[3], (64, 1)))
    # the rotation is orthonormal and the level, unturned body gives T_bc shifted by its position
    R = got[:, :3, :3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14
    level = np.zeros((1, 9)); level[0, :3] = (1.0, 2.0, 3.0)
    want0 = T_bc.copy(); want0[:3, 3] += (1.0, 2.0, 3.0)
    assert np.array_equal(RO.camera_poses(level, T_bc)[0], want0)
