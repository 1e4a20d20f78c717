"""CPU tests of the occupancy map: hand-computed known answers for the restatement (tests/occmap_oracle.py) that the GPU tests
compare the device map against, and the boundary of section (8) of include/frp_nmpc.h as far as it exists without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from forces_resilient_planner_amd import solver
from tests import occmap_oracle as OO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_map():
    """4 x 3 x 2 voxels of 0.5 m: x in [-1, 1), y in [-0.5, 1), z in [0, 1).  Every number below is exact in binary."""
    m = OO.OccMapOracle(origin=(-1.0, -0.5, 0.0), map_size=(2.0, 1.5, 1.0), resolution=0.5, local_radius=(1.5, 0.3, 0.3))
    assert tuple(m.grid_size) == (4, 3, 2)
    return m


def occupied(m):
    return sorted(map(tuple, np.argwhere(m.buffer > m.min_occupancy_log).tolist()))


def test_insert_known_answers():
    m = small_map()
    assert occupied(m) == [] and np.all(m.buffer == 0.12)
    # exactly on the face between voxels x = 1 and x = 2 (x = 0.0: (0 + 1) * 2 = 2.0): belongs to the upper voxel
    m.insert_cloud([[0.0, 0.25, 0.25]])
    assert occupied(m) == [(2, 1, 0)] and m.buffer[2, 1, 0] == 0.97
    # exactly on the far edge of the map (x = 1.0 -> index 4 = grid_size): dropped; one float below it: the last voxel
    m.insert_cloud([[1.0, 0.25, 0.25]])
    assert occupied(m) == [(2, 1, 0)]
    m.insert_cloud([[np.nextafter(np.float32(1.0), np.float32(0.0)), 0.25, 0.25]])
    assert occupied(m) == [(2, 1, 0), (3, 1, 0)]
    # just below the origin: floor gives -1 (dropped); truncation towards zero would have hit voxel 0
    m.insert_cloud([[-1.0001, 0.25, 0.25], [0.25, -0.5001, 0.25], [0.25, 0.25, -0.0001]])
    assert occupied(m) == [(2, 1, 0), (3, 1, 0)]
    # NaN in any coordinate, infinities, beyond int: dropped
    m.insert_cloud([[np.nan, 0.25, 0.25], [0.25, np.nan, 0.25], [0.25, 0.25, np.nan], [np.inf, 0.25, 0.25], [-np.inf, 0.25, 0.25], [3e38, 0.25, 0.25]])
    assert occupied(m) == [(2, 1, 0), (3, 1, 0)]
    # exactly on the origin corner: voxel 0
    m.insert_cloud([[-1.0, -0.5, 0.0]])
    assert occupied(m) == [(0, 0, 0), (2, 1, 0), (3, 1, 0)]
    assert np.array_equal(m.occ(), (m.buffer == 0.97).astype(np.uint8)) and m.occ().dtype == np.uint8


def test_local_range_sticking_out_and_the_exclusive_inclusive_difference():
    m = small_map()
    # centre (0, 0.25, 0.5), radius (1.5, 0.3, 0.3):
    #   x: floor((-1.5 + 1) * 2) = -1 -> max(0, -1) = 0;   floor((1.5 + 1) * 2) = 5 -> min(4, 5) = 4     (sticks out on both sides)
    #   y: floor((-0.05 + 0.5) * 2) = 0;                   floor((0.55 + 0.5) * 2) = 2 -> min(3, 2) = 2
    #   z: floor(0.2 * 2) = 0;                             floor(0.8 * 2) = 1 -> min(2, 1) = 1
    c = (0.0, 0.25, 0.5)
    box = m.local_box(c)
    assert box == [0, 0, 0, 4, 2, 1]
    m.buffer[1, 0, 0] = 0.97   # inside both
    m.buffer[2, 2, 1] = 0.97   # y and z ON max_id: local for isInLocalMap (inclusive, :56), not visited by the cloud loops (exclusive, :192-194)
    m.buffer[3, 1, 1] = 0.97   # z on max_id
    m.buffer[0, 1, 0] = 0.97   # inside both
    cloud = m.local_cloud_loops(c)
    # x, y, z loop order; centres origin + (id + 0.5) * 0.5
    assert np.array_equal(cloud, np.array([[-0.75, 0.25, 0.25], [-0.25, -0.25, 0.25]]))
    assert np.array_equal(m.local_cloud(c), cloud)
    for idx, in_cloud in (((1, 0, 0), True), ((2, 2, 1), False), ((3, 1, 1), False), ((0, 1, 0), True)):
        pos = m.index_to_pos(idx)
        assert m.get_voxel_state(pos, box) == 1                      # all four are occupied AND local for the query
        assert any(np.array_equal(pos, p) for p in cloud) == in_cloud
    # the whole map: all four, in x, y, z order
    assert m.local_box(None) == [0, 0, 0, 4, 3, 2]
    assert np.array_equal(m.local_cloud_loops(None), np.array([[-0.75, 0.25, 0.25], [-0.25, -0.25, 0.25], [0.25, 0.75, 0.75], [0.75, 0.25, 0.75]]))
    assert np.array_equal(m.local_cloud(None), m.local_cloud_loops(None))
    # a range entirely outside the map, a NaN centre: empty, and nothing is local
    for c2 in ((50.0, 0.25, 0.5), (-50.0, 0.25, 0.5), (np.nan, 0.25, 0.5)):
        b2 = m.local_box(c2)
        assert len(m.local_cloud_loops(c2)) == 0 and len(m.local_cloud(c2)) == 0
        assert m.get_voxel_state(m.index_to_pos((1, 0, 0)), b2) == 0
    assert m.local_box((50.0, 0.25, 0.5))[:4] == [99, 0, 0, 4]       # floor((50 - 1.5 + 1) * 2) = 99: min_id is NOT clamped to the grid from above (:50-52)


def test_point_query_known_answers():
    m = small_map()
    m.buffer[1, 0, 0] = 0.97
    m.buffer[3, 2, 1] = 0.80   # exactly the threshold: NOT occupied (strict >, :105)
    # radius (1.5, 0.3, 0.3): x floor((-2.25 + 1) * 2) = -3 -> 0, floor((0.75 + 1) * 2) = 3; y floor((-0.65 + 0.5) * 2) = -1 -> 0, floor((-0.05 + 0.5) * 2) = 0;
    # z floor(-0.05 * 2) = -1 -> 0, floor(0.55 * 2) = 1
    box = m.local_box((-0.75, -0.35, 0.25))
    assert box == [0, 0, 0, 3, 0, 1]
    assert m.get_voxel_state((-0.25, -0.25, 0.25)) == 1 and m.get_voxel_state((-0.25, -0.25, 0.25), box) == 1
    assert m.get_voxel_state((-0.25, 0.25, 0.25)) == 0                      # free
    assert m.get_voxel_state((0.75, 0.75, 0.75)) == 0                       # at the threshold
    assert m.get_voxel_state((1.0, 0.0, 0.5)) == -1 and m.get_voxel_state((np.nan, 0.0, 0.5)) == -1 and m.get_voxel_state((-1.0001, 0.0, 0.5)) == -1
    m.buffer[1, 1, 0] = 0.97
    assert m.get_voxel_state((-0.25, 0.25, 0.25)) == 1 and m.get_voxel_state((-0.25, 0.25, 0.25), box) == 0   # occupied, but outside the local map
    assert m.get_voxel_state((1.0, 0.0, 0.5), box) == -1                    # the map test comes first (:99-102)


def test_reset_buffer_known_answers():
    m = small_map()
    m.buffer[...] = 0.97
    # min (-0.6, -9, 0.5) -> clamped y -0.5 -> ids (0, 0, 1); max (0.5, 0.25, 9) -> clamped z 1.0, minus 0.25 -> (0.25, 0.0, 0.75) -> ids (2, 1, 1); inclusive
    m.reset_buffer((-0.6, -9.0, 0.5), (0.5, 0.25, 9.0))
    want = np.full((4, 3, 2), 0.97)
    want[0:3, 0:2, 1:2] = 0.12
    assert np.array_equal(m.buffer, want)
    m.reset_buffer((5.0, 5.0, 5.0), (9.0, 9.0, 9.0))   # beyond the map: nothing
    assert np.array_equal(m.buffer, want)
    m.reset()
    assert np.all(m.buffer == 0.12)


def test_centres_pass_through_float32():
    m = OO.OccMapOracle(origin=(-10.0, -10.0, -1.0), map_size=(20.0, 20.0, 4.0), resolution=0.1)
    assert tuple(m.grid_size) == (200, 200, 40)
    m.buffer[0, 3, 7] = 0.97
    pos = m.index_to_pos((0, 3, 7))
    assert pos[0] == -10.0 + 0.5 * 0.1 and pos[0] == -9.95
    got = m.local_cloud_loops(None)
    assert got.shape == (1, 3) and got.dtype == np.float64
    assert got[0, 0] == float(np.float32(-9.95)) and got[0, 0] != pos[0]          # the pcl::PointXYZ passage is visible
    assert np.array_equal(got, pos.astype(np.float32).astype(np.float64)[None, :]) and not np.array_equal(got[0], pos)
    assert np.array_equal(m.local_cloud(None), got)
    # and the cloud's own points land in the voxels they came from (the corridor's cloud re-inserted reproduces the map)
    m2 = OO.OccMapOracle(origin=(-10.0, -10.0, -1.0), map_size=(20.0, 20.0, 4.0), resolution=0.1)
    m2.insert_cloud(got)
    assert np.array_equal(m2.buffer, m.buffer)


def test_vectorised_cloud_equals_the_loops_on_a_random_map():
    rng = np.random.default_rng(5)
    m = OO.OccMapOracle(origin=(-0.7, 0.3, -0.2), map_size=(1.3, 0.9, 0.7), resolution=0.1, local_radius=(0.45, 0.3, 0.25))
    m.buffer[rng.random(m.buffer.shape) < 0.3] = 0.97
    for c in [None] + list(rng.uniform(-1.2, 1.5, (40, 3))):
        assert np.array_equal(m.local_cloud(c), m.local_cloud_loops(c))


# ---- the boundary ----
def _prototypes():
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(frp_nmpc_occmap_\w+)\s*\(", hdr)))


def test_every_new_prototype_is_exported_and_the_abi_version_stays():
    names = _prototypes()
    assert set(names) == {"frp_nmpc_occmap_workspace_bytes", "frp_nmpc_occmap_reset", "frp_nmpc_occmap_clear_box", "frp_nmpc_occmap_insert_cloud",
                          "frp_nmpc_occmap_refresh", "frp_nmpc_occmap_local_view", "frp_nmpc_occmap_query"}
    lib = solver.lib()
    for n in names:
        assert hasattr(lib, n), n
        assert n in solver.EXPORTS
    assert lib.frp_nmpc_abi_version() == 7 and solver.ABI_VERSION == 7
    assert "#define FRP_NMPC_ABI_VERSION 7" in open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    assert lib.frp_nmpc_abi_check(7, ctypes.sizeof(solver.Options), ctypes.sizeof(solver.Batch), solver.INFO_STRIDE) == 0


def test_ctypes_mirrors_have_the_headers_layout(tmp_path):
    fields = {"frp_nmpc_occmap": solver.OccMap, "frp_nmpc_occmap_view": solver.OccMapView}
    lines = []
    for cname, cls in fields.items():
        lines.append(f'_Static_assert(sizeof({cname}) == {ctypes.sizeof(cls)}, "{cname}");')
        for f, _ in cls._fields_:
            lines.append(f'_Static_assert(offsetof({cname}, {f}) == {getattr(cls, f).offset}, "{cname}.{f}");')
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "frp_nmpc.h"\n' + "\n".join(lines) + "\nint main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "layout.o")])


def _has_gpu():
    try:
        return solver.lib().frp_nmpc_device_count() > 0
    except Exception:
        return False


def _desc(**kw):
    m = solver.OccMap()
    m.origin[:] = (-20.0, -20.0, 0.0); m.map_size[:] = (40.0, 40.0, 5.0); m.resolution = 0.1; m.grid[:] = (400, 400, 50)
    m.clamp_min_log, m.clamp_max_log, m.min_occupancy_log = 0.12, 0.97, 0.80
    m.local_radius[:] = (6.0, 6.0, 3.0)
    m.log_odds = 0x1000; m.occ = 0x2000   # never dereferenced on the host; nothing is launched in these tests
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(m, k)[:] = v
        else:
            setattr(m, k, v)
    return m


def _calls(lib, m, ws_bytes, P=16, view_kw=None):
    """Every call of section (8) on the description m (None: a null map), with otherwise valid arguments."""
    pm = ctypes.byref(m) if m is not None else None
    ws = ctypes.c_void_p(0x3000)
    v = solver.OccMapView(4, 0x4000, P, 0x5000, 0x6000, 0x7000)
    for k, val in (view_kw or {}).items():
        setattr(v, k, val)
    lo, hi = (ctypes.c_double * 3)(0.0, 0.0, 0.0), (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    return {"reset": lib.frp_nmpc_occmap_reset(pm, ws, ws_bytes, None),
            "refresh": lib.frp_nmpc_occmap_refresh(pm, ws, ws_bytes, None),
            "clear_box": lib.frp_nmpc_occmap_clear_box(pm, lo, hi, ws, ws_bytes, None),
            "insert_cloud": lib.frp_nmpc_occmap_insert_cloud(pm, ctypes.c_void_p(0x8000), 16, ws, ws_bytes, None),
            "local_view": lib.frp_nmpc_occmap_local_view(pm, ctypes.byref(v), ws, ws_bytes, None),
            "query": lib.frp_nmpc_occmap_query(pm, 8, ctypes.c_void_p(0x9000), None, None, ctypes.c_void_p(0xa000), ws, ws_bytes, None)}


FRP_ERR_NO_DEVICE, FRP_ERR_ARG = -1001, -1003


def test_workspace_query_and_argument_errors():
    lib = solver.lib()
    good = _desc()
    need = lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(good))
    assert need == 400 * 400 * 2 * 4   # two 32-bit words per column of 50 voxels
    assert lib.frp_nmpc_occmap_workspace_bytes(None) == 0
    bad = {"null map": None, "zero resolution": _desc(resolution=0.0), "negative resolution": _desc(resolution=-0.1),
           "NaN resolution": _desc(resolution=float("nan")), "grid inconsistent with map_size / resolution": _desc(grid=(400, 400, 51)),
           "grid inconsistent (x)": _desc(grid=(399, 400, 50)), "null log_odds": _desc(log_odds=None), "null occ": _desc(occ=None)}
    for what, m in bad.items():
        if m is not None:
            assert lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(m)) == 0, what
        for call, rc in _calls(lib, m, need).items():
            assert rc == FRP_ERR_ARG, (what, call, rc)
    # arguments of single calls, on a good map
    assert all(rc == FRP_ERR_ARG for rc in _calls(lib, good, need - 1).values())            # workspace too small
    assert _calls(lib, good, need, P=65536 + 1)["local_view"] == FRP_ERR_ARG                # P above FRP_CORRIDOR_MAX_POINTS
    assert _calls(lib, good, need, P=-1)["local_view"] == FRP_ERR_ARG
    assert _calls(lib, good, need, view_kw=dict(B=0))["local_view"] == FRP_ERR_ARG
    assert _calls(lib, good, need, view_kw=dict(centre=None))["local_view"] == FRP_ERR_ARG   # the whole-map mode is B = 1
    assert _calls(lib, good, need, view_kw=dict(cloud=None))["local_view"] == FRP_ERR_ARG    # counts without a cloud
    assert _calls(lib, good, need, view_kw=dict(cloud_count=None))["local_view"] == FRP_ERR_ARG
    assert _calls(lib, good, need, view_kw=dict(cloud=None, cloud_count=None, local_box=None))["local_view"] == FRP_ERR_ARG
    pm, ws = ctypes.byref(good), ctypes.c_void_p(0x3000)
    assert lib.frp_nmpc_occmap_local_view(pm, None, ws, need, None) == FRP_ERR_ARG
    assert lib.frp_nmpc_occmap_insert_cloud(pm, None, 16, ws, need, None) == FRP_ERR_ARG
    assert lib.frp_nmpc_occmap_insert_cloud(pm, ctypes.c_void_p(0x8000), -1, ws, need, None) == FRP_ERR_ARG
    assert lib.frp_nmpc_occmap_query(pm, 8, None, None, None, ctypes.c_void_p(0xa000), ws, need, None) == FRP_ERR_ARG
    assert lib.frp_nmpc_occmap_query(pm, 8, ctypes.c_void_p(0x9000), ctypes.c_void_p(0xb000), None, ctypes.c_void_p(0xa000), ws, need, None) == FRP_ERR_ARG
    nan3 = (ctypes.c_double * 3)(float("nan"), 0.0, 0.0)
    assert lib.frp_nmpc_occmap_clear_box(pm, nan3, (ctypes.c_double * 3)(1.0, 1.0, 1.0), ws, need, None) == FRP_ERR_ARG
    assert lib.frp_nmpc_occmap_clear_box(pm, None, None, ws, need, None) == FRP_ERR_ARG


@pytest.mark.skipif(_has_gpu(), reason="checks the behaviour of a machine WITHOUT a device")
def test_every_call_reports_no_device():
    lib = solver.lib()
    good = _desc()
    need = lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(good))
    for call, rc in _calls(lib, good, need).items():
        assert rc == FRP_ERR_NO_DEVICE, (call, rc)
    assert _calls(lib, good, need, view_kw=dict(B=1, centre=None))["local_view"] == FRP_ERR_NO_DEVICE   # whole-map mode
    assert _calls(lib, good, need, view_kw=dict(cloud=None, cloud_count=None))["local_view"] == FRP_ERR_NO_DEVICE  # boxes only
    with pytest.raises(RuntimeError):
        solver.OccupancyMap(origin=(0, 0, 0), map_size=(1, 1, 1), resolution=0.1, device="cpu")
