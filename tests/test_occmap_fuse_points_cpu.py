"""CPU tests of point-scan fusion (include/frp_nmpc_occmap_fuse_points.h): the boundary as far as it exists without a device, and the
conditions on the inputs of tests/test_gpu_occmap_fuse_points.py, checked with the oracle so that the GPU tests cannot pass for
the wrong reason."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from forces_resilient_planner_amd import solver
from tests import occmap_fuse_points_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRP_ERR_NO_DEVICE, FRP_ERR_ARG = -1001, -1003
NAN, INF = float("nan"), float("inf")
S, P = 4, 20000


def _map_desc():
    m = solver.OccMap()
    m.origin[:] = (-20.0, -20.0, -1.0); m.map_size[:] = (40.0, 40.0, 5.0); m.resolution = 0.1; m.grid[:] = (400, 400, 50)
    m.clamp_min_log, m.clamp_max_log, m.min_occupancy_log = -1.0, 2.0, 1.70
    m.local_radius[:] = (6.0, 6.0, 3.0)
    m.log_odds = 0x1000; m.occ = 0x2000   # never dereferenced on the host; nothing is launched in these tests
    return m


def _desc(**kw):
    """S scans behind fake device pointers: nothing behind them is ever read on the host."""
    f = solver.OccMapFusePoints()
    f.scans, f.P = S, P
    f.points, f.points_f32, f.count, f.origin, f.active, f.status = 0x3000000, None, None, 0x7000, None, 0x4000
    for k in solver.OCCMAP_FUSE_POINTS_PARAMS:
        setattr(f, k, solver.OCCMAP_FUSE_DEFAULTS[k])
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def _fuse(lib, m, f, ws_bytes, fws_bytes, ws=0x5000, fws=0x10000000):
    return lib.frp_nmpc_occmap_fuse_points_batch(ctypes.byref(m) if m is not None else None, ctypes.byref(f) if f is not None else None,
                                                 ctypes.c_void_p(ws), ws_bytes, ctypes.c_void_p(fws), fws_bytes, None)


def _need(lib, m, f):
    return lib.frp_nmpc_occmap_fuse_points_workspace_bytes(ctypes.byref(m) if m is not None else None, ctypes.byref(f) if f is not None else None)


@pytest.mark.parametrize("header", ["frp_nmpc.h", "frp_nmpc_occmap_fuse_points.h"])
def test_symbols_struct_layout_and_abi_version(tmp_path, header):
    lib = solver.lib()
    assert solver.FUSE_POINTS_EXPORTS == ["frp_nmpc_occmap_fuse_points_workspace_bytes", "frp_nmpc_occmap_fuse_points_batch"]
    for n in solver.FUSE_POINTS_EXPORTS:
        assert hasattr(lib, n)
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    assert '#include "frp_nmpc_occmap_fuse_points.h"' in hdr and "#define FRP_NMPC_ABI_VERSION 7" in hdr and lib.frp_nmpc_abi_version() == 7
    lines = [f'_Static_assert(sizeof(frp_nmpc_occmap_fuse_points) == {ctypes.sizeof(solver.OccMapFusePoints)}, "size");']
    for fld, _ in solver.OccMapFusePoints._fields_:
        lines.append(f'_Static_assert(offsetof(frp_nmpc_occmap_fuse_points, {fld}) == {getattr(solver.OccMapFusePoints, fld).offset}, "{fld}");')
    lines.append(f'_Static_assert(FRP_OCCMAP_FUSE_POINTS_MAX_SCANS == {solver.OCCMAP_FUSE_POINTS_MAX_SCANS} && FRP_OCCMAP_FUSE_POINTS_MAX_SCANS == FRP_OCCMAP_FUSE_MAX_FRAMES, "scans cap");')
    lines.append('_Static_assert(FRP_OCCMAP_FUSE_REFUSED == -256 && FRP_NMPC_ABI_VERSION == 7 && FRP_OCCMAP_FUSE_DEFAULT_ROUNDS == 128, "refused, version, default rounds");')
    # the existing fusion structs did not change, through either header
    lines.append(f'_Static_assert(sizeof(frp_nmpc_occmap_fuse) == {ctypes.sizeof(solver.OccMapFuse)}, "single-frame size");')
    lines.append(f'_Static_assert(sizeof(frp_nmpc_occmap_fuse_batch) == {ctypes.sizeof(solver.OccMapFuseBatch)}, "batch size");')
    use = ("size_t use(const frp_nmpc_occmap *m, const frp_nmpc_occmap_fuse_points *f) { return frp_nmpc_occmap_fuse_points_workspace_bytes(m, f)"
           " + (size_t)frp_nmpc_occmap_fuse_points_batch(m, f, 0, 0, 0, 0, 0); }")
    body = f'#include <stddef.h>\n#include "{header}"\n' + "\n".join(lines) + f"\n{use}\nint main(void) {{ return 0; }}\n"
    c11 = tmp_path / "layout.c"
    c11.write_text(body)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(c11), "-o", str(tmp_path / "layout.o")])
    # the header alone (and inside frp_nmpc.h) as strict C99, and as C++ with its own extern "C"
    c99 = tmp_path / "alone.c"
    c99.write_text(f'#include <stddef.h>\n#include "{header}"\n{use}\nint main(void) {{ return 0; }}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(c99), "-o", str(tmp_path / "alone.o")])
    cpp = tmp_path / "alone.cpp"
    cpp.write_text(f'#include <cstddef>\n#include "{header}"\n{use}\nint main() {{ return 0; }}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(cpp), "-o", str(tmp_path / "alonepp.o")])
    syms = subprocess.run(["nm", "-D", "--defined-only", solver.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in solver.FUSE_POINTS_EXPORTS:
        assert re.search(r"\sT\s+%s$" % n, syms, flags=re.M), n          # unmangled: the extern "C" holds in the library as well


def test_frp_nmpc_h_itself_declares_no_new_occmap_name():
    """tests/test_occmap_cpu.py pins the names frp_nmpc.h itself declares; the new prototypes live in the header of their own."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frp_nmpc.h")).read(), flags=re.S)
    own = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frp_nmpc_occmap_fuse_points.h")).read(), flags=re.S)
    assert "fuse_points" not in hdr.replace('#include "frp_nmpc_occmap_fuse_points.h"', "")
    assert sorted(set(re.findall(r"\b(frp_nmpc_occmap_\w+)\s*\(", own))) == sorted(solver.FUSE_POINTS_EXPORTS)
    doc = open(os.path.join(ROOT, "include", "frp_nmpc_occmap_fuse_points.h")).read()
    assert "NON-FINITE POINTS" in doc and "dropped" in doc and "keeps its index" in doc   # the departure from the reference is stated


REFUSED = {
    "max_ray_length below min_ray_length": dict(min_ray_length=2.0, max_ray_length=1.0),
    "step bound above 4096": dict(max_ray_length=136.5),          # 3 * (ceil(136.5 / 0.1) + 2) = 4101
    "max_rounds negative": dict(max_rounds=-1), "max_rounds above 255": dict(max_rounds=256),
    "NaN hit": dict(prob_hit_log=NAN), "infinite miss": dict(prob_miss_log=-INF), "NaN min_ray_length": dict(min_ray_length=NAN),
    "infinite max_ray_length": dict(max_ray_length=INF),
    "no scans": dict(scans=0), "negative scans": dict(scans=-1), "scans above the cap": dict(scans=solver.OCCMAP_FUSE_POINTS_MAX_SCANS + 1),
    "negative P": dict(P=-1), "P above 2^24": dict(P=(1 << 24) + 1),
}
# refused by the call for a pointer; the size function does not look at pointers
REFUSED_POINTERS = {"null origin": dict(origin=None), "null status": dict(status=None), "neither point pointer": dict(points=None),
                    "both point pointers": dict(points_f32=0x6000000)}


def test_argument_errors_come_before_any_launch():
    lib = solver.lib()
    m, good = _map_desc(), _desc()
    ws = lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    need = _need(lib, m, good)
    assert need > 0
    for what, kw in REFUSED.items():
        f = _desc(**kw)
        assert _need(lib, m, f) == 0, what
        assert _fuse(lib, m, f, ws, 1 << 40) == FRP_ERR_ARG, what
    for what, kw in REFUSED_POINTERS.items():
        f = _desc(**kw)
        assert _need(lib, m, f) == need, what
        assert _fuse(lib, m, f, ws, need) == FRP_ERR_ARG, what
    assert _need(lib, None, good) == 0 and _need(lib, m, None) == 0
    bad_map = _map_desc(); bad_map.grid[2] = 51
    assert _need(lib, bad_map, good) == 0
    assert _fuse(lib, bad_map, good, ws, need) == FRP_ERR_ARG and _fuse(lib, None, good, ws, need) == FRP_ERR_ARG and _fuse(lib, m, None, ws, need) == FRP_ERR_ARG
    assert _fuse(lib, m, good, ws - 1, need) == FRP_ERR_ARG and _fuse(lib, m, good, ws, need - 1) == FRP_ERR_ARG      # short workspaces
    assert _fuse(lib, m, good, ws, need, ws=0) == FRP_ERR_ARG and _fuse(lib, m, good, ws, need, fws=0) == FRP_ERR_ARG
    assert _fuse(lib, m, good, ws, need + 8, fws=0x10000004) == FRP_ERR_ARG                                            # misaligned
    # the caps themselves, the float form, and every optional array are accepted as descriptions
    assert _need(lib, m, _desc(scans=solver.OCCMAP_FUSE_POINTS_MAX_SCANS)) > need
    assert _need(lib, m, _desc(P=1 << 24, scans=1)) > need
    assert _need(lib, m, _desc(points=None, points_f32=0x6000000, count=0x8000, active=0x9000, max_rounds=255)) == need


def test_what_is_behind_the_pointers_is_not_a_host_matter():
    """Origins and counts live on the device: the host must not (and cannot) look at them.  Real host arrays of NaN origins and wild
    counts stand behind the pointers here -- a host that read them would refuse or size the workspace by them."""
    lib = solver.lib()
    m = _map_desc()
    need = _need(lib, m, _desc())
    origin = (ctypes.c_double * (3 * S))(*([NAN] * (3 * S)))
    count = (ctypes.c_int * S)(-5, 1 << 30, 0, 7)
    assert _need(lib, m, _desc(origin=ctypes.addressof(origin), count=ctypes.addressof(count))) == need


def test_workspace_grows_with_scans_and_points_and_p_zero_is_valid():
    lib = solver.lib()
    m = _map_desc()
    one = _need(lib, m, _desc(scans=1))
    prev = 0
    for scans in (1, 2, 3, 16, solver.OCCMAP_FUSE_POINTS_MAX_SCANS):
        need = _need(lib, m, _desc(scans=scans))
        assert need > prev and need <= scans * one + 256, scans              # S slices and a descriptor per scan (inside `one` already)
        prev = need
    per_point = (_need(lib, m, _desc(scans=1, P=2 * P)) - one) / P
    assert abs(per_point - 36) < 4 * 256 / P                                   # the clipped point (3 doubles), its end voxel, its count, its list entry: four arrays, each rounded up to 256 bytes
    # the depth call for as many points has the same slice: the layout is shared
    fb = solver.OccMapFuseBatch()
    fb.frames, fb.rows, fb.cols = 1, 100, 200
    fb.K[:] = (380.0, 0.0, 320.0, 0.0, 380.0, 240.0, 0.0, 0.0, 1.0)
    for k, v in solver.OCCMAP_FUSE_DEFAULTS.items():
        setattr(fb, k, v)
    fb.depth_filter_margin, fb.skip_pixel = 0, 1
    assert lib.frp_nmpc_occmap_fuse_batch_workspace_bytes(ctypes.byref(m), ctypes.byref(fb)) == one and 100 * 200 == P
    # no points at all: a valid description, with or without point pointers (the call itself: test_fuse_points_reports_no_device and the GPU tests)
    assert 0 < _need(lib, m, _desc(scans=1, P=0, points=None)) == _need(lib, m, _desc(scans=1, P=0)) < one


def _has_gpu():
    try:
        return solver.lib().frp_nmpc_device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the behaviour of a machine WITHOUT a device")
def test_fuse_points_reports_no_device():
    lib = solver.lib()
    m = _map_desc()
    ws = lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    for f in (_desc(), _desc(points=None, points_f32=0x6000000), _desc(max_rounds=1, active=0x9000, count=0x8000, scans=1), _desc(P=0, points=None)):
        need = _need(lib, m, f)
        assert need > 0 and _fuse(lib, m, f, ws, need) == FRP_ERR_NO_DEVICE


def test_the_python_binding_exists():
    assert callable(solver.OccupancyMap.fuse_points)
    assert ctypes.sizeof(solver.OccMapFusePoints) > 0 and solver.OccMapFusePoints._fields_[0][0] == "scans"
    assert set(solver.OCCMAP_FUSE_POINTS_PARAMS) < set(solver.OCCMAP_FUSE_DEFAULTS)


# ---- the conditions the GPU tests rely on ----
def _all_point_sets():
    sets = {f"realistic {s} {p}": C.realistic(s, p) for s, p in C.REALISTIC}
    sets.update({f"realistic {s} {p} as float": (C.widened(C.realistic(s, p)[0]), C.realistic(s, p)[1]) for s, p in C.REALISTIC})
    sets.update({"float-sensitive": C.float_sensitive(), "float-sensitive as float": (C.widened(C.float_sensitive()[0]), C.MIDDLE)})
    sets.update({f"camera frame {k}": sc for k, sc in enumerate(C.six_scans())})
    sets.update({f"edge: {n}": C.edge_sets()[n] for n in C.EDGE_NAMES})
    sets.update({f"single ray {k}": C.single_ray(k) for k in (0, 1)})
    sets.update({f"one of 64, {k}": sc for k, sc in enumerate(C.many_scans(64))})
    return sets


def test_the_rounds_solve_every_point_set_of_the_gpu_tests():
    """FusionOracle.raycast == raycast_relaxed (stops and map) on every scan the GPU tests fuse, with no cell skipped for the ray box."""
    rounds = {}
    for name, (pts, origin) in _all_point_sets().items():
        r, rays, same = C.relaxed(pts, origin)
        assert same and 1 <= r <= solver.OCCMAP_FUSE_DEFAULT_ROUNDS, name
        rounds[name] = (r, rays)
    print(rounds)
    assert all(rounds[f"realistic {s} {p}"][0] >= 2 and rounds[f"realistic {s} {p}"][1] > 100 for s, p in C.REALISTIC)
    assert all(rounds[f"single ray {k}"] == (1, 1) for k in (0, 1))


def test_the_edge_sets_are_what_their_names_say():
    e = C.edge_sets()
    st = {n: C.edge_chain(n)[1][0] for n in C.EDGE_NAMES}
    start = C.oracle().buffer.tobytes()
    print(st)
    assert st["count 0"] == [1, 0] and C.edge_chain("count 0")[0].buffer.tobytes() == start
    assert st["all closer than min_ray_length"] == [1, 0] and C.edge_chain("all closer than min_ray_length")[0].buffer.tobytes() == start
    # clipped: every end is a miss, so no voxel gains anything
    om = C.edge_chain("beyond max_ray_length")[0]
    assert st["beyond max_ray_length"][1] > 30 and (om.buffer <= C.oracle().buffer).all() and om.buffer.tobytes() != start
    assert all(hit == 0 for _, hit in om.last_counts.values())
    # INVALID_IDX ends are not deduplicated: every point casts, the repeated ones as well
    assert st["ends outside the map"][1] == len(e["ends outside the map"][0]) == 50
    # 24 points share a voxel and one of them casts; the order decides which, and with it the map
    a, b = C.edge_chain("many points in one voxel"), C.edge_chain("many points in one voxel, reversed")
    assert a[1][0][1] == b[1][0][1] == 3 and a[0].buffer.tobytes() != b[0].buffer.tobytes()
    assert a[0].last_counts[(42, 37, 12)][1] == 24 == b[0].last_counts[(42, 37, 12)][1]
    # need_ray false: the first of the three points is the one ray, no cell is walked, the sensor's voxel takes the three hits
    om = C.edge_chain("sensor and point in one voxel")[0]
    assert st["sensor and point in one voxel"] == [1, 1] and om.last_counts == {(32, 32, 16): (3, 3)}
    assert st["sensor outside the map"][0] >= 2 and st["sensor outside the map"][1] > 30
    assert st["points on voxel faces"][1] >= 6
    holes = e["NaN and inf rows"][0]
    dropped = int((~np.isfinite(holes).all(axis=1)).sum())
    assert dropped >= 10 and len(C.finite_rows(holes)) == len(holes) - dropped
    assert C.edge_chain("NaN and inf rows")[0].buffer.tobytes() != C.realistic_chain("random", "middle", False)[0].buffer.tobytes()
    # the batch of all of them is a chain of its own, not the last scan's map
    assert C.edge_batch_chain()[1] == [st[n] for n in C.EDGE_NAMES]
    assert C.edge_batch_chain()[0].buffer.tobytes() not in {C.edge_chain(n)[0].buffer.tobytes() for n in C.EDGE_NAMES}


def test_a_float_scan_differs_from_its_double_scan():
    """The float32 cases are cases of their own only if rounding the points to float changes the map.  The projected scans are too
    far from voxel faces for that (printed); the scan built for it is not."""
    print([C.realistic_chain(s, p, True)[0].buffer.tobytes() != C.realistic_chain(s, p, False)[0].buffer.tobytes() for s, p in C.REALISTIC])
    (as_float, st_f), (as_double, st_d) = C.float_sensitive_chain(True), C.float_sensitive_chain(False)
    assert as_float.buffer.tobytes() != as_double.buffer.tobytes() and st_f[0][1] > 30 and st_d[0][1] > 30
    pts = C.float_sensitive()[0]
    assert (C.widened(pts) != pts).mean() > 0.9


def test_the_order_of_the_two_scans_matters():
    fwd, st = C.order_chain(False)
    rev, st_rev = C.order_chain(True)
    assert st_rev == st[::-1] and all(s[0] >= 2 and s[1] > 100 for s in st)
    assert fwd.buffer.tobytes() != rev.buffer.tobytes()
    # ... because of a clamp: among the voxels where the two maps differ, many are at a clamp in one of them
    d = fwd.buffer != rev.buffer
    at_clamp = np.isin(fwd.buffer[d], (-1.0, 2.0)) | np.isin(rev.buffer[d], (-1.0, 2.0))
    assert at_clamp.sum() > 10


def test_the_capped_scan_does_not_converge_at_its_cap_and_its_neighbours_do():
    scans = C.cap_scans()
    free = [C.relaxed(p, o)[:2] for p, o in scans]
    assert free[0] == (1, 1) and free[2] == (1, 1) and free[3] == (1, 0) and free[1][0] >= 2 and free[1][1] > 100, free
    om = C.oracle()
    pts = [tuple(float(v) for v in p) for p in scans[1][0]]
    before = om.buffer.copy()
    assert om.raycast_relaxed(pts, scans[1][1], max_rounds=1) == (None, -1) and (om.buffer == before).all()
    capped, st = C.cap_chain()
    assert st == [[1, 1], [-1, free[1][1]], [1, 1], [1, 0]]
    assert capped.buffer.tobytes() == C.chain(scans, skip={1})[0].buffer.tobytes() != C.chain(scans)[0].buffer.tobytes()


def test_many_scans_touch_the_map():
    om, st = C.many_chain(64)
    assert len(st) == 64 and all(s[0] >= 1 and 1 <= s[1] <= 4 for s in st) and om.buffer.tobytes() != C.oracle().buffer.tobytes()
