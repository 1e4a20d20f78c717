"""CPU tests of the occupancy map's distance field and clearance queries (include/frp_nmpc_occmap_distance.h): the brute-force
statement tests/occmap_distance_oracle.py against SciPy's Euclidean distance transform and against properties that need no second
implementation; a separable model of the device's three passes (from the bit plane's words, windows of +-R, the cut at the end) that
equals the statement as written and, broken deliberately in five ways, fails on a named case each; and the boundary of the calls as
far as it exists without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from forces_resilient_planner_amd import solver
from tests import occmap_distance_oracle as DO
from tests import occmap_oracle as OO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(7, 5, 33), (13, 9, 70), (4, 3, 2), (6, 6, 40), (5, 5, 5), (3, 3, 3)]
NONE = np.int64(1) << 40


def random_occ(grid, p, seed):
    occ = np.random.default_rng(seed).random(grid) < p
    occ[tuple(np.random.default_rng(seed + 1).integers(0, g) for g in grid)] = True   # never empty
    return occ


# ---- the statement against SciPy and against itself ----
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_the_statement_equals_scipys_distance_transform_without_a_border(grid):
    from scipy import ndimage
    for seed, p in ((1, 0.02), (2, 0.3)):
        occ = random_occ(grid, p, seed)
        edt2 = np.rint(ndimage.distance_transform_edt(~occ) ** 2).astype(np.int64)
        assert np.array_equal(DO.squared_distance(occ, False), edt2)
        for R in (1, 2, 5, 9):
            assert np.array_equal(DO.field(occ, R, False), np.where(edt2 <= R * R, edt2, DO.FAR).astype(np.uint16)), (seed, R)


@pytest.mark.parametrize("grid", GRIDS[:4], ids=lambda g: "x".join(map(str, g)))
def test_the_border_terms_are_a_shell_of_occupied_voxels(grid):
    """`border` as the definition words it -- every voxel outside the map is occupied -- on a map padded by one shell of them (the
    nearest outside voxel of a voxel of the map lies in that shell, straight along an axis)."""
    occ = random_occ(grid, 0.01, 5)
    padded = np.ones(tuple(g + 2 for g in grid), dtype=bool)
    padded[1:-1, 1:-1, 1:-1] = occ
    assert np.array_equal(DO.squared_distance(padded, False)[1:-1, 1:-1, 1:-1], DO.squared_distance(occ, True))
    assert np.array_equal(DO.squared_distance(np.zeros(grid, dtype=bool), True)[0, 0, 0], 1)


def test_properties_that_need_no_second_implementation():
    grid, R = (13, 9, 70), 3   # (with the border, R = 3 leaves the columns y = 3 ... 5 out of the walls' reach)
    occ = random_occ(grid, 0.004, 7)
    plain, bordered = DO.field(occ, R, False), DO.field(occ, R, True)
    assert (plain[occ] == 0).all() and (bordered[occ] == 0).all() and (plain[~occ] > 0).all()
    assert (plain == DO.FAR).any() and (plain != DO.FAR).any()
    for axis in range(3):
        for border in (False, True):
            assert np.array_equal(DO.field(np.flip(occ, axis), R, border), np.flip(DO.field(occ, R, border), axis)), (axis, border)
    assert (bordered <= plain).all() and (bordered < plain).any()
    for border in (False, True):
        small, large = DO.field(occ, R, border), DO.field(occ, R + 3, border)
        keep = small != DO.FAR
        assert np.array_equal(small[keep], large[keep]) and (large[~keep] > R * R).all() and (large[~keep] != DO.FAR).any()
    # the empty map: all FAR, or border distances only; the full map: all 0
    empty = np.zeros((4, 3, 2), dtype=bool)
    assert (DO.field(empty, 9, False) == DO.FAR).all()
    assert (DO.field(empty, 9, True) == 1).all()   # two voxels along z: each touches the outside
    e = DO.field(np.zeros((7, 5, 33), dtype=bool), 2, True)
    assert e[3, 2, 16] == DO.FAR and e[0, 2, 16] == 1 and e[1, 2, 16] == 4 and e[3, 2, 32] == 1 and e[3, 2, 31] == 4 and e[1, 1, 1] == 4 and e[2, 2, 16] == DO.FAR
    assert (DO.field(np.ones((5, 5, 5), dtype=bool), 3, False) == 0).all()


def test_the_bit_plane_round_trip_and_its_padding():
    occ = random_occ((7, 5, 33), 0.2, 9)
    plane = DO.pack_plane(occ)
    assert plane.shape == (7, 5, 2) and plane.dtype == np.uint32 and (plane[:, :, 1] <= 1).all()   # the second word has one voxel
    assert np.array_equal(DO.unpack_plane(plane, 33), occ)
    assert plane[2, 3, 0] == sum(1 << z for z in range(32) if occ[2, 3, z])
    stale = plane.copy()
    stale[:, :, 1] |= np.uint32(0xfffffffe)
    assert np.array_equal(DO.unpack_plane(stale, 33), occ)


# ---- a separable model of the device's passes, and its deliberate breaks ----
def separable(plane, gz, R, border, window=None, cut_lt=False, count_padding=False, border_shift=0):
    """Three passes f'(i) = min over |k| <= W of f(i + k) + k * k, z first, from f = 0 on set bits and none elsewhere; with `border` an
    index outside the axis contributes k * k; the cut at R * R once, at the end.  The knobs are the breaks: `window` W = R - 1,
    `cut_lt` a cut at < R * R, `count_padding` the bits at z >= gz of the last word taken for voxels, `border_shift` the border moved by
    that many voxels."""
    plane = np.asarray(plane, dtype=np.uint32)
    gx, gy, wz = plane.shape
    W = R if window is None else window
    bits = ((plane[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).reshape(gx, gy, wz * 32).astype(bool)
    if not count_padding:
        bits[:, :, gz:] = False
    f = np.where(bits, np.int64(0), NONE)
    for axis, g in ((2, gz), (1, gy), (0, gx)):
        n = f.shape[axis]
        out = np.full(f.shape, NONE, dtype=np.int64)
        idx = np.arange(n)
        for k in range(-W, W + 1):
            src = idx + k
            ok = (src >= 0) & (src < n)
            cand = np.full(f.shape, NONE, dtype=np.int64)
            sl_out = [slice(None)] * 3; sl_in = [slice(None)] * 3
            sl_out[axis] = idx[ok]; sl_in[axis] = src[ok]
            cand[tuple(sl_out)] = f[tuple(sl_in)] + k * k
            out = np.minimum(out, cand)
        if border:
            shape = [1, 1, 1]; shape[axis] = n
            for edge in (idx + 1 + border_shift, g - idx + border_shift):
                term = np.where((edge <= W) & (idx < g), edge * edge, NONE).reshape(shape)
                out = np.minimum(out, term)
        f = out
    f = f[:, :, :gz]
    keep = f < R * R if cut_lt else f <= R * R
    return np.where(keep, f, DO.FAR).astype(np.uint16)


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_the_separable_model_equals_the_statement(grid):
    for seed, p in ((3, 0.0), (4, 0.01), (5, 0.2), (6, 1.0)):
        occ = np.random.default_rng(seed).random(grid) < p if 0.0 < p < 1.0 else np.full(grid, p == 1.0)
        plane = DO.pack_plane(occ)
        for R in range(1, 10):
            for border in (0, 1):
                assert np.array_equal(separable(plane, grid[2], R, border), DO.field(occ, R, border)), (seed, R, border)


def one_voxel(grid, at):
    occ = np.zeros(grid, dtype=bool)
    occ[at] = True
    return occ


def test_every_deliberate_break_fails_on_its_named_case():
    grid, R = (7, 5, 33), 3
    # an occupied voxel exactly R away along x: the value R * R = 9 is in the field
    occ = one_voxel(grid, (0, 2, 10))
    plane = DO.pack_plane(occ)
    want = DO.field(occ, R, 0)
    assert want[3, 2, 10] == 9 and want[4, 2, 10] == DO.FAR and np.array_equal(separable(plane, 33, R, 0), want)
    assert separable(plane, 33, R, 0, window=R - 1)[3, 2, 10] == DO.FAR                        # a window of R - 1
    assert separable(plane, 33, R, 0, cut_lt=True)[3, 2, 10] == DO.FAR                         # a cut at < instead of <=
    assert separable(plane, 33, R, 0, cut_lt=True)[2, 2, 10] == 4
    # a stale padding bit (z = 34 of a 33-voxel column): not a voxel without a border
    empty = DO.pack_plane(np.zeros(grid, dtype=bool))
    stale = empty.copy()
    stale[3, 2, 1] |= np.uint32(1 << 2)
    assert (DO.field_of_plane(stale, 33, R, 0) == DO.FAR).all() and np.array_equal(separable(stale, 33, R, 0), DO.field_of_plane(stale, 33, R, 0))
    assert separable(stale, 33, R, 0, count_padding=True)[3, 2, 32] == 4                       # padding bits counted
    # the border one voxel off: the map's own edge voxels would be outside
    want = DO.field_of_plane(empty, 33, R, 1)
    assert want[0, 0, 0] == 1 and want[3, 2, 16] == 9 and np.array_equal(separable(empty, 33, R, 1), want)
    broken = separable(empty, 33, R, 1, border_shift=-1)
    assert broken[0, 0, 0] == 0 and broken[3, 2, 16] == 4
    # floor(pos) taken before the offset is subtracted: another voxel wherever the origin is no multiple of the resolution
    m = OO.OccMapOracle(origin=(-1.25, -1.0, 0.0), map_size=(0.7, 0.5, 3.3), resolution=0.1)
    assert tuple(m.grid_size) == grid
    pos = np.array([-1.2, -0.75, 1.05])
    assert DO.voxel_of(m, pos) == (0, 2, 10)
    early = tuple(int(v) for v in np.floor(pos * m.resolution_inv) - np.floor(m.origin * m.resolution_inv))
    assert early == (1, 2, 10)
    fld = DO.field(occ, R, 0)
    assert DO.clearance(m, fld, pos) == (0.0, 0) and fld[early] == 1


def test_clearance_rule_and_trace_accumulation_known_answers():
    m = OO.OccMapOracle(origin=(-1.25, -1.0, 0.0), map_size=(0.7, 0.5, 3.3), resolution=0.1)
    fld = DO.field(one_voxel((7, 5, 33), (0, 2, 10)), 3, 0)
    inside, near, far = np.array([-1.2, -0.75, 1.05]), np.array([-1.0, -0.65, 1.05]), np.array([-0.7, -0.75, 1.05])
    assert DO.clearance(m, fld, inside) == (0.0, 0)
    assert DO.voxel_of(m, near) == (2, 3, 10) and DO.clearance(m, fld, near) == (0.1 * np.sqrt(5.0), 5)
    assert DO.clearance(m, fld, far) == (float("inf"), DO.FAR)
    for bad in ([np.nan, -0.75, 1.05], [np.inf, -0.75, 1.05], [-1.2, -np.inf, 1.05], [-1.26, -0.75, 1.05], [-1.2, -0.75, 3.31]):
        assert DO.clearance(m, fld, np.array(bad)) == (0.0, -1), bad
    trace = np.zeros((3, 4, 9))
    trace[0, :, 0:3] = [far, near, far, near]
    trace[1, :, 0:3] = [near, [np.nan, 0.0, 0.0], far, inside]
    trace[2, :, 0:3] = [inside] * 4
    mn, hits, samples = DO.trace_accumulate(m, fld, trace, [np.inf, np.inf, 7.0], [0, 0, 5], [0, 2, 9], active=[1, 1, 0])
    assert list(mn) == [0.1 * np.sqrt(5.0), 0.0, 7.0] and list(hits) == [0, 2, 5] and list(samples) == [4, 6, 9]
    # one call of S samples is S calls of one
    state = (np.full(3, np.inf), np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32))
    for s in range(4):
        state = DO.trace_accumulate(m, fld, trace[:, s:s + 1], *state)
    whole = DO.trace_accumulate(m, fld, trace, np.full(3, np.inf), np.zeros(3), np.zeros(3))
    assert all(np.array_equal(a, b) for a, b in zip(state, whole))


# ---- the boundary ----
FRP_ERR_NO_DEVICE, FRP_ERR_ARG = -1001, -1003
NAMES = ["frp_nmpc_occmap_distance_scratch_bytes", "frp_nmpc_occmap_distance_update", "frp_nmpc_occmap_clearance",
         "frp_nmpc_occmap_clearance_trace", "frp_nmpc_occmap_clearance_reset"]


def test_the_calls_are_declared_and_exported_and_the_abi_version_stays(tmp_path):
    lib = solver.lib()
    assert solver.DISTANCE_EXPORTS == NAMES
    for n in NAMES:
        assert hasattr(lib, n), n
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    assert hdr.count('#include "frp_nmpc_occmap_distance.h"') == 1 and "#define FRP_NMPC_ABI_VERSION 7" in hdr and solver.ABI_VERSION == 7
    own = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "frp_nmpc_occmap_distance.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(frp_nmpc_occmap_\w+)\s*\(", own))) == sorted(NAMES)
    assert (solver.OCCMAP_DIST_FAR, solver.OCCMAP_DIST_MAX_R) == (DO.FAR, DO.MAX_R)
    lines = [f'_Static_assert(FRP_OCCMAP_DIST_FAR == {solver.OCCMAP_DIST_FAR}, "far");', f'_Static_assert(FRP_OCCMAP_DIST_MAX_R == {solver.OCCMAP_DIST_MAX_R}, "r");',
             '_Static_assert(FRP_OCCMAP_DIST_MAX_R * FRP_OCCMAP_DIST_MAX_R < FRP_OCCMAP_DIST_FAR, "room");',
             "static int (*const p_update)(const frp_nmpc_occmap *, int, int, uint16_t *, void *, size_t, void *, size_t, void *) = frp_nmpc_occmap_distance_update;"]
    for inc in ("frp_nmpc.h", "frp_nmpc_occmap_distance.h"):   # through frp_nmpc.h, and on its own
        src = tmp_path / ("distance_" + inc.replace(".", "_") + ".c")
        src.write_text('#include "' + inc + '"\n' + "\n".join(lines) + "\nint main(void) { (void)p_update; return 0; }\n")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(src) + ".o"])
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-x", "c++", "-D_Static_assert=static_assert", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(src) + ".cpp.o"])


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
        if k == "grid":
            m.grid[:] = v
        else:
            setattr(m, k, v)
    return m


UPDATE = dict(map=True, R=20, border=1, field=0x9000, scratch=0xa000, short=0, ws=0x3000, ws_short=0)
POINTS = dict(map=True, field=0x9000, R=20, Q=8, pos=0xa000, clear=0xb000, d2=None)
TRACE = dict(map=True, field=0x9000, R=20, B=4, S=5, stride=9, pos=0xa000, active=None, min_clear=0xb000, hits=0xc000, samples=0xd000)
RESET = dict(B=4, mask=None, min_clear=0xb000, hits=0xc000, samples=0xd000)


def _call(which, **kw):
    lib = solver.lib()
    m = _desc(**kw.pop("desc", {}))
    a = dict({"update": UPDATE, "points": POINTS, "trace": TRACE, "reset": RESET}[which]); a.update(kw)
    pm = ctypes.byref(m) if a.get("map") else None
    if which == "update":
        need = lib.frp_nmpc_occmap_distance_scratch_bytes(ctypes.byref(_desc()), 20)
        ws = lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(_desc()))
        return lib.frp_nmpc_occmap_distance_update(pm, a["R"], a["border"], a["field"], a["scratch"], need - a["short"], a["ws"], ws - a["ws_short"], None)
    if which == "points":
        return lib.frp_nmpc_occmap_clearance(pm, a["field"], a["R"], a["Q"], a["pos"], a["clear"], a["d2"], None)
    if which == "trace":
        return lib.frp_nmpc_occmap_clearance_trace(pm, a["field"], a["R"], a["B"], a["S"], a["stride"], a["pos"], a["active"], a["min_clear"], a["hits"],
                                                   a["samples"], None)
    return lib.frp_nmpc_occmap_clearance_reset(a["B"], a["mask"], a["min_clear"], a["hits"], a["samples"], None)


BAD = [("update", dict(map=False)), ("update", dict(R=0)), ("update", dict(R=65)), ("update", dict(R=-3)), ("update", dict(field=None)),
       ("update", dict(scratch=None)), ("update", dict(short=1)), ("update", dict(ws=None)), ("update", dict(ws_short=1)),
       ("update", dict(desc=dict(grid=(400, 400, 51)))), ("update", dict(desc=dict(resolution=0.0))), ("update", dict(desc=dict(log_odds=None))),
       ("points", dict(map=False)), ("points", dict(field=None)), ("points", dict(R=0)), ("points", dict(R=65)), ("points", dict(Q=-1)),
       ("points", dict(pos=None)), ("points", dict(clear=None)), ("points", dict(desc=dict(grid=(399, 400, 50)))),
       ("trace", dict(map=False)), ("trace", dict(field=None)), ("trace", dict(R=0)), ("trace", dict(B=-1)), ("trace", dict(S=0)), ("trace", dict(S=-5)),
       ("trace", dict(stride=2)), ("trace", dict(stride=0)), ("trace", dict(pos=None)), ("trace", dict(min_clear=None)), ("trace", dict(hits=None)),
       ("trace", dict(samples=None)), ("trace", dict(B=1 << 30, S=4)),
       ("reset", dict(B=-1)), ("reset", dict(min_clear=None)), ("reset", dict(hits=None)), ("reset", dict(samples=None))]


@pytest.mark.parametrize("which,kw", BAD, ids=[f"{w}-{'-'.join(k)}-{i}" for i, (w, k) in enumerate(BAD)])
def test_argument_errors_come_before_any_launch(which, kw):
    assert _call(which, **kw) == FRP_ERR_ARG


def test_scratch_size_query():
    lib = solver.lib()
    n = 400 * 400 * 50
    assert n % 256 == 0
    for R in (1, 20, 64):
        assert lib.frp_nmpc_occmap_distance_scratch_bytes(ctypes.byref(_desc()), R) == 3 * n   # an 8-bit and a 16-bit volume
    odd = _desc(map_size=(ctypes.c_double * 3)(0.7, 0.5, 3.3), grid=(7, 5, 33))
    assert lib.frp_nmpc_occmap_distance_scratch_bytes(ctypes.byref(odd), 5) == 1280 + 2 * 1155              # the first volume padded to 256 bytes
    for bad_R in (0, -1, 65):
        assert lib.frp_nmpc_occmap_distance_scratch_bytes(ctypes.byref(_desc()), bad_R) == 0
    assert lib.frp_nmpc_occmap_distance_scratch_bytes(None, 20) == 0
    assert lib.frp_nmpc_occmap_distance_scratch_bytes(ctypes.byref(_desc(grid=(400, 400, 51))), 20) == 0
    assert lib.frp_nmpc_occmap_distance_scratch_bytes(ctypes.byref(_desc(resolution=float("nan"))), 20) == 0


@pytest.mark.skipif(_has_gpu(), reason="checks the behaviour of a machine WITHOUT a device")
def test_every_call_reports_no_device():
    for which in ("update", "points", "trace", "reset"):
        assert _call(which) == FRP_ERR_NO_DEVICE, which
    assert _call("update", R=1, border=0) == FRP_ERR_NO_DEVICE and _call("update", R=64) == FRP_ERR_NO_DEVICE
    assert _call("points", Q=0, pos=None, clear=None) == FRP_ERR_NO_DEVICE and _call("points", d2=0xe000) == FRP_ERR_NO_DEVICE
    assert _call("trace", B=0, pos=None, min_clear=None, hits=None, samples=None) == FRP_ERR_NO_DEVICE
    assert _call("trace", active=0xe000, stride=3) == FRP_ERR_NO_DEVICE
    assert _call("reset", mask=0xe000) == FRP_ERR_NO_DEVICE and _call("reset", B=0, min_clear=None, hits=None, samples=None) == FRP_ERR_NO_DEVICE


def test_python_objects_refuse_what_the_header_refuses():
    """(what needs no device: the radius check comes before any allocation)"""
    import types
    fake = types.SimpleNamespace(torch=None)
    for R in (0, 65, -1):
        with pytest.raises(ValueError):
            solver.DistanceField(fake, R)
