"""CPU tests of the point-scan renderer (include/frp_nmpc_occmap_render_scan.h): the boundary as far as it exists without a device,
the specification (tests/occmap_scan_oracle.py) against closed forms and against the depth renderer's specification, the beam table
of solver.lidar_beams, and the round trip scan -> FusionOracle on the scenes the GPU tests use, so that those cannot pass for the
wrong reason."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from forces_resilient_planner_amd import solver
from tests import occmap_render_cases as RC
from tests import occmap_render_oracle as RO
from tests import occmap_scan_cases as C
from tests import occmap_scan_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRP_ERR_NO_DEVICE, FRP_ERR_ARG = -1001, -1003
NAN, INF = float("nan"), float("inf")
NAMES = ["frp_nmpc_occmap_render_scan_batch"]


# ---- header and exports ----
def _layout_lines():
    lines = [f'_Static_assert(sizeof(frp_nmpc_occmap_render_scan) == {ctypes.sizeof(solver.OccMapRenderScan)}, "size");']
    for fld, _ in solver.OccMapRenderScan._fields_:
        lines.append(f'_Static_assert(offsetof(frp_nmpc_occmap_render_scan, {fld}) == {getattr(solver.OccMapRenderScan, fld).offset}, "{fld}");')
    lines.append('_Static_assert(FRP_NMPC_ABI_VERSION == 7 && FRP_OCCMAP_FUSE_POINTS_MAX_SCANS == 64 && FRP_OCCMAP_FUSE_REFUSED == -256, "unchanged");')
    # no existing struct changed
    for name, mirror in (("frp_nmpc_occmap", solver.OccMap), ("frp_nmpc_occmap_render", solver.OccMapRender), ("frp_nmpc_occmap_fuse_points", solver.OccMapFusePoints)):
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(mirror)}, "{name}");')
    return lines


@pytest.mark.parametrize("header", ["frp_nmpc.h", "frp_nmpc_occmap_render_scan.h"])
@pytest.mark.parametrize("lang", ["c99", "c11", "c++"])
def test_the_header_compiles_alone_and_through_frp_nmpc_h(tmp_path, header, lang):
    """Strict C99 (the boundary is a C ABI), C11 with the struct's layout against the ctypes mirror, and C++."""
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    assert '#include "frp_nmpc_occmap_render_scan.h"' in hdr and "#define FRP_NMPC_ABI_VERSION 7" in hdr
    own = open(os.path.join(ROOT, "include", "frp_nmpc_occmap_render_scan.h")).read()
    for n in NAMES:
        assert n + "(" in own and n + "(" not in hdr
    assert "render_scan" not in re.sub(r"/\*.*?\*/", "", hdr, flags=re.S).replace('#include "frp_nmpc_occmap_render_scan.h"', "")
    use = ("int use(const frp_nmpc_occmap *m, const frp_nmpc_occmap_render_scan *r, void *ws) {\n"
           "  return frp_nmpc_occmap_render_scan_batch(m, r, ws, 0, 0); }\n")
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


def test_the_symbol_is_exported_and_checked_at_load():
    lib = solver.lib()
    assert solver.RENDER_SCAN_EXPORTS == NAMES
    for n in NAMES:
        assert hasattr(lib, n), n
    syms = subprocess.run(["nm", "-D", "--defined-only", solver.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\sT\s+frp_nmpc_occmap_render_scan_batch$", syms, flags=re.M)
    assert lib.frp_nmpc_abi_version() == 7
    assert callable(solver.OccupancyMap.render_scan) and callable(solver.lidar_beams)


def _map_desc():
    m = solver.OccMap()
    m.origin[:] = (-20.0, -20.0, -1.0); m.map_size[:] = (40.0, 40.0, 5.0); m.resolution = 0.1; m.grid[:] = (400, 400, 50)
    m.clamp_min_log, m.clamp_max_log, m.min_occupancy_log = -1.0, 2.0, 1.70
    m.local_radius[:] = (6.0, 6.0, 3.0)
    m.log_odds = 0x1000; m.occ = 0x2000   # never dereferenced on the host; nothing is launched in these tests
    return m


def _desc(**kw):
    """Poisoned device pointers: nothing behind them is ever read on the host."""
    r = solver.OccMapRenderScan()
    r.scans, r.P = 4, 65536
    r.beams, r.T_ws, r.active = 0x7000, 0x8000, None
    r.min_range, r.max_range, r.far_range = 0.1, 6.0, 0.0
    r.points, r.points_f32, r.origin, r.count, r.range, r.voxel, r.status = 0x3000000, None, 0x9000, None, None, None, 0x4000
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _render(lib, m, r, ws_bytes, ws=0x5000):
    return lib.frp_nmpc_occmap_render_scan_batch(ctypes.byref(m) if m is not None else None, ctypes.byref(r) if r is not None else None,
                                                 ctypes.c_void_p(ws), ws_bytes, None)


REFUSED = {
    "null beams": dict(beams=None), "null T_ws": dict(T_ws=None), "null origin": dict(origin=None), "null status": dict(status=None),
    "both point outputs null": dict(points=None),
    "no scans": dict(scans=0), "negative scans": dict(scans=-1), "scans above the cap": dict(scans=solver.OCCMAP_FUSE_POINTS_MAX_SCANS + 1),
    "no beams": dict(P=0), "negative P": dict(P=-1), "P above 2^24": dict(P=(1 << 24) + 1),
    "NaN min_range": dict(min_range=NAN), "infinite min_range": dict(min_range=INF), "negative min_range": dict(min_range=-0.1),
    "NaN max_range": dict(max_range=NAN), "infinite max_range": dict(max_range=INF), "max_range 0": dict(max_range=0.0, min_range=0.0),
    "negative max_range": dict(max_range=-6.0, min_range=0.0),
    "min_range above max_range": dict(min_range=6.5),
    "far_range below max_range": dict(far_range=5.9), "negative far_range": dict(far_range=-8.0), "NaN far_range": dict(far_range=NAN),
    "infinite far_range": dict(far_range=INF),
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
    # the limits themselves are accepted: the scan cap, one beam and 2^24 beams, min_range = 0 and = max_range, far_range = max_range,
    # the largest step bound (3 * (1363 + 2) = 4095), either point output and both, every optional array
    for r in (_desc(), _desc(scans=solver.OCCMAP_FUSE_POINTS_MAX_SCANS), _desc(scans=1, P=1), _desc(P=1 << 24), _desc(min_range=0.0),
              _desc(min_range=6.0), _desc(far_range=6.0), _desc(far_range=8.0), _desc(max_range=136.3),
              _desc(points=None, points_f32=0x6000000), _desc(points_f32=0x6000000),
              _desc(active=0xa000, count=0xb000, range=0xc000000, voxel=0xd000000)):
        assert _render(lib, m, r, ws) == FRP_ERR_NO_DEVICE
    # poses and beams are on the device: host arrays of NaN behind the pointers are not looked at
    poses = (ctypes.c_double * 64)(*([NAN] * 64))
    table = (ctypes.c_double * 12)(*([NAN] * 12))
    assert _render(lib, m, _desc(T_ws=ctypes.addressof(poses), beams=ctypes.addressof(table), P=4), ws) == FRP_ERR_NO_DEVICE


# ---- the specification against closed forms ----
GEO = C.GEO["low"]
D_WALL = 1.2
SENSOR = (-1.0, 1.0, 1.05)                    # on a voxel face in x, mid-voxel in y and z: voxel (10, 18, 10)
AXES = C.SPECIAL[C.N_UNFIRED:]                # +x, -x, +y, -y, +z


def _wall_map(distance):
    """A one-voxel-thick wall perpendicular to x whose near face is `distance` in front of SENSOR."""
    occ = np.zeros(C.GRID["low"], dtype=np.uint8)
    ix = int(round((SENSOR[0] + distance - GEO["origin"][0]) / 0.1))
    occ[ix, :, :] = 1
    return SO.ScanOracle(occ, GEO["origin"], GEO["resolution"]), ix


def _empty():
    return SO.ScanOracle(np.zeros(C.GRID["low"], dtype=np.uint8), GEO["origin"], GEO["resolution"])


def test_a_wall_at_a_known_distance():
    o, ix = _wall_map(D_WALL)
    assert ix == 22
    s = o.scan(C.axis_pose(SENSOR), C.beams(), C.MAX_RANGE)
    P = len(C.beams())
    px = P - 5                                                          # the +x beam: two zero components of d_w
    assert abs(s["range"][px] - (D_WALL + 0.05)) < 1e-12               # the midpoint of the 0.1 m the beam spends inside the voxel
    assert s["voxel"][px] == (22 * 40 + 18) * 20 + 10
    assert np.abs(s["points"][px] - np.array([SENSOR[0] + 1.25, SENSOR[1], SENSOR[2]])).max() < 1e-12
    assert s["points"][px][1] == SENSOR[1] and s["points"][px][2] == SENSOR[2]      # t + s_mid * 0 exactly
    # an unnormalised beam along +x gives the same range, point and voxel: metres along the beam, not the ray parameter
    twice = o.scan(C.axis_pose(SENSOR), np.array([[2.0, 0.0, 0.0]]), C.MAX_RANGE)
    assert abs(twice["range"][0] - 1.25) < 1e-12 and abs(twice["s_mid"][0] - 0.625) < 1e-12 and twice["voxel"][0] == s["voxel"][px]
    # -x, +-y and +z leave the map without a hit; the three beams that are not fired give NaN
    assert (s["voxel"][[P - 4, P - 3, P - 2, P - 1]] == -1).all() and np.isnan(s["points"][P - 8:P - 5]).all()
    ret = s["voxel"] >= 0
    assert s["status"] == [1, int(ret.sum())] and s["count"] == P and 300 < ret.sum() < P
    assert np.array_equal(np.isnan(s["points"]).any(axis=1), ~ret) and np.array_equal(s["range"] > 0, ret)
    # every return lies in the wall, at a range of at least 1.2 m, and its range is the distance from the sensor
    assert (s["voxel"][ret] // (40 * 20) == 22).all() and (s["range"][ret] >= D_WALL).all()
    assert np.abs(np.linalg.norm(s["points"][ret] - np.array(SENSOR), axis=1) - s["range"][ret]).max() < 1e-12
    assert np.array_equal(s["origin"], np.array(SENSOR))


def test_an_empty_world_gives_all_nan_or_points_at_far_range():
    o = _empty()
    for T in (C.pose_of("middle"), C.pose_of("near_face"), C.pose_of(C.OUTSIDE), C.axis_pose(SENSOR)):
        s = o.scan(T, C.beams(), C.MAX_RANGE)
        assert np.isnan(s["points"]).all() and (s["voxel"] == -1).all() and not s["range"].any() and s["status"] == [1, 0] and s["steps"] > 0
        assert s["count"] == len(C.beams())
        f = o.scan(T, C.beams(), C.MAX_RANGE, far_range=8.0)
        fired = np.isfinite(C.beams()).all(axis=1) & (np.linalg.norm(C.beams(), axis=1) > 0)
        assert fired.sum() == len(C.beams()) - C.N_UNFIRED
        assert np.isnan(f["points"][~fired]).all() and np.isfinite(f["points"][fired]).all()
        dist = np.linalg.norm(f["points"][fired] - T[:3, 3], axis=1)
        assert np.abs(dist - 8.0).max() <= 4 * np.spacing(8.0)            # exactly 8 m out, within 4 ulp
        assert f["status"] == [1, 0] and (f["voxel"] == -1).all() and not f["range"].any()      # far points are no returns


def test_a_wall_beyond_max_range_and_a_hit_nearer_than_min_range_give_no_return():
    o, _ = _wall_map(D_WALL)
    T = C.axis_pose(SENSOR)
    px = len(C.beams()) - 5
    s = o.scan(T, C.beams(), 1.15)                                      # the wall's entry face at 1.2 m is past 1.15 m on every beam
    assert np.isnan(s["points"]).all() and (s["voxel"] == -1).all() and s["status"] == [1, 0]
    s = o.scan(T, C.beams(), 1.25)                                      # just inside: the +x beam enters at 1.2 <= 1.25, oblique ones do not
    assert s["voxel"][px] >= 0 and 0 < s["status"][1] < 200
    # min_range: the +x beam's return is at 1.25 m
    assert o.scan(T, AXES, C.MAX_RANGE, min_range=1.25)["voxel"][0] >= 0
    s = o.scan(T, AXES, C.MAX_RANGE, min_range=1.2500001)
    assert s["voxel"][0] == -1 and np.isnan(s["points"][0]).all() and s["range"][0] == 0.0 and s["status"] == [1, 0]
    # ... and the walk does not go on behind the hit: a second wall 0.5 m further is not seen either
    occ = np.zeros(C.GRID["low"], dtype=np.uint8); occ[22, :, :] = 1; occ[27, :, :] = 1
    two = SO.ScanOracle(occ, GEO["origin"], GEO["resolution"])
    assert two.scan(T, AXES, C.MAX_RANGE, min_range=1.5)["status"] == [1, 0]
    # with far_range the beam that lost its return gives the far point
    s = two.scan(T, AXES, C.MAX_RANGE, min_range=1.5, far_range=8.0)
    assert s["voxel"][0] == -1 and abs(s["points"][0][0] - (SENSOR[0] + 8.0)) < 1e-12


def test_a_sensor_inside_an_occupied_voxel_sees_nothing_and_a_non_finite_pose_is_refused():
    o, ix = _wall_map(D_WALL)
    inside = (GEO["origin"][0] + (ix + 0.5) * 0.1, SENSOR[1], SENSOR[2])
    for T in (C.axis_pose(inside), C.sensor_pose(inside)):
        s = o.scan(T, C.beams(), C.MAX_RANGE)
        assert np.isnan(s["points"]).all() and (s["voxel"] == -1).all() and s["status"] == [1, 0] and s["steps"] == 0
    T = C.axis_pose(SENSOR); T[2, 0] = INF
    s = o.scan(T, C.beams(), C.MAX_RANGE, far_range=8.0)
    assert s["status"] == [SO.REFUSED, 0] and SO.REFUSED == solver.OCCMAP_FUSE_REFUSED and s["count"] == 0
    assert np.isnan(s["points"]).all() and (s["voxel"] == -1).all() and not s["range"].any()
    assert np.array_equal(s["origin"], np.array(SENSOR))                # as it stands
    T = C.axis_pose(SENSOR); T[1, 3] = NAN
    s = o.scan(T, C.beams(), C.MAX_RANGE)
    assert s["status"] == [SO.REFUSED, 0] and np.isnan(s["origin"][1]) and s["origin"][0] == SENSOR[0]


# ---- the specification pinned to the depth renderer's ----
@pytest.mark.parametrize("placement", ["middle", "near_face"])
@pytest.mark.parametrize("scene", ["pillars", "wall"])
def test_the_pinhole_table_gives_the_depth_renderers_image(scene, placement):
    rows, cols = RC.IMAGES["large"]
    Km = RC.K["large"]
    d, vox, _, st, steps = RC.rendered(scene, "low", "large", placement)
    s = C.oracle(scene, "low").scan(RC.pose_of(placement), C.pinhole_beams(Km, rows, cols), C.MAX_RANGE)
    assert st[1] > 200
    # depth_scale 1000 keeps every return of these scenes within 1 ... 65535, so the two have the same returns
    assert np.array_equal(s["voxel"].reshape(rows, cols), vox)
    ret = s["voxel"] >= 0
    pix = np.zeros(rows * cols)
    pix[ret] = np.floor(s["s_mid"][ret] * 1000.0 + 0.5)
    assert np.array_equal(pix.reshape(rows, cols), d.astype(np.float64))
    assert s["status"] == st and s["steps"] == steps


# ---- lidar_beams ----
def test_lidar_beams_shape_firing_order_and_unit_length():
    b = solver.lidar_beams(16, 72, -0.4, 0.4)
    assert b.shape == (1152, 3) and b.dtype == np.float64
    assert np.abs(np.linalg.norm(b, axis=1) - 1.0).max() <= 2 * 2.0 ** -52
    for j, i in ((0, 0), (0, 15), (1, 0), (35, 7), (71, 15)):                # column-major: all rings of one azimuth, then the next
        az, el = 2 * math.pi * j / 72, -0.4 + 0.8 * i / 15
        want = (math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el))
        assert np.abs(b[16 * j + i] - want).max() <= 2 * 2.0 ** -52, (j, i)
    assert (np.diff(b[:16, 2]) > 0).all() and np.ptp(np.arctan2(b[:16, 1], b[:16, 0])) < 1e-15     # a column: rising elevation, one azimuth
    # a one-ring table: the four cardinal beams, elevation_min as the elevation
    c = solver.lidar_beams(1, 4, 0.0, 0.3)
    assert c.shape == (4, 3) and np.abs(c - np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], dtype=np.float64)).max() < 2e-16
    assert np.array_equal(c[0], [1.0, 0.0, 0.0])
    h = solver.lidar_beams(2, 8, -0.1, 0.2, azimuth_span=math.pi)                                  # half a turn
    assert abs(math.atan2(h[14, 1], h[14, 0]) - math.pi * 7 / 8) < 1e-15 and abs(h[15, 2] - math.sin(0.2)) < 1e-16
    with pytest.raises(ValueError):
        solver.lidar_beams(0, 8, 0.0, 0.1)


# ---- the round trip on the CPU ----
@pytest.mark.parametrize("as_float", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("placement", ["middle", "near_face"])
@pytest.mark.parametrize("scene", ["pillars", "wall"])
def test_a_rendered_scan_fuses_back_into_the_voxels_it_came_from(scene, placement, as_float):
    height = "low"
    s = C.scanned(scene, height, placement)
    pts = s["points"].astype(np.float32).astype(np.float64) if as_float else s["points"]
    ret = s["voxel"] >= 0
    returns = int(ret.sum())
    assert s["status"] == [1, returns] and returns > 200, (scene, placement, returns)
    occ = C.world_occ(scene, height).reshape(-1) != 0
    assert occ[s["voxel"][ret]].all()                                   # every return is an occupied voxel of the world
    ex = C.excluded(pts, ret, height, C.MARGIN[np.float32 if as_float else np.float64])
    print(f"{scene} {placement} {'float' if as_float else 'double'}: {returns} returns, {int(ex.sum())} excluded ({ex.sum() / returns:.4f})")
    assert ex.sum() <= 0.01 * returns
    keep = ret & ~ex
    fo = C.fusion_oracle(height)
    for p in np.flatnonzero(keep):                                      # every kept return indexes into the voxel reported
        id_ = fo._index([float(v) for v in pts[p]])
        assert id_ is not None and C.linear(id_, height) == s["voxel"][p], p
    # one fusion raises every kept hit voxel ...
    om = C.fuse_chain(height, [(pts, s["origin"])])
    flat = om.buffer.reshape(-1)
    assert (flat[s["voxel"][keep]] > om.clamp_min_log).all()
    # ... and after three (-1 -> 0.2 -> 1.4 -> 2.0 crosses min_occupancy_log = 1.7) the belief holds obstacles, all of them the world's
    om = C.fuse_chain(height, [(pts, s["origin"])], times=3)
    got = om.buffer.reshape(-1) > om.min_occupancy_log
    allowed = occ.copy()
    for p in np.flatnonzero(ex):
        id_ = fo._index([float(v) for v in pts[p]])
        if id_ is not None:
            allowed[C.linear(id_, height)] = True
    assert got.sum() > 50 and not (got & ~allowed).any(), (int(got.sum()), int((got & ~allowed).sum()))
