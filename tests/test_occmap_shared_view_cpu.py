"""CPU tests of the device-built shared view (include/frp_nmpc_occmap_view.h: frp_nmpc_occmap_shared_view,
frp_nmpc_occmap_shared_view_dims / _update, frp_nmpc_corridor_batch_view): the header and its ctypes mirror, the exports, and the
argument checks that run before a device is touched."""
import ctypes
import os
import subprocess

import pytest

from forces_resilient_planner_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
FRP_OK, FRP_ERR_NO_DEVICE, FRP_ERR_ARG = 0, -1001, -1003
NAN, INF = float("nan"), float("inf")
NAMES = ["frp_nmpc_occmap_shared_view_dims", "frp_nmpc_occmap_shared_view_update", "frp_nmpc_corridor_batch_view"]
FIELDS = [f for f, _ in solver.OccMapSharedView._fields_]


@pytest.mark.parametrize("header", ["frp_nmpc.h", "frp_nmpc_occmap_view.h"])
def test_header_compiles_as_c99_and_the_mirror_has_its_layout(tmp_path, header):
    hdr = open(os.path.join(INC, "frp_nmpc.h")).read()
    own = open(os.path.join(INC, "frp_nmpc_occmap_view.h")).read()
    assert '#include "frp_nmpc_occmap_view.h"' in hdr
    for n in NAMES:
        assert n + "(" in own and n + "(" not in hdr
    offs = ", ".join(f"offsetof(frp_nmpc_occmap_shared_view, {f})" for f in FIELDS)
    use = ('int use(const frp_nmpc_occmap *m, const frp_nmpc_occmap_shared_view *v, const frp_nmpc_corridor *p, void *ws, int *d) {\n'
           '  return frp_nmpc_occmap_shared_view_dims(m, 0.5, d) + frp_nmpc_occmap_shared_view_update(m, v, ws, 0, 0)\n'
           '       + frp_nmpc_corridor_batch_view(p, 0, 0); }\n')
    main = ('int main(void) { size_t o[] = {sizeof(frp_nmpc_occmap_shared_view), %s}; size_t i;\n' % offs +
            '  for (i = 0; i < sizeof o / sizeof o[0]; i++) printf("%zu ", o[i]);\n'
            '  printf("%d %d %d %d\\n", FRP_OCCMAP_VIEW_MAX_GROUPS, FRP_OCCMAP_VIEW_LAUNCHES, FRP_CORRIDOR_MAX_CELLS, FRP_CORRIDOR_MAX_POINTS);\n'
            '  return FRP_NMPC_ABI_VERSION == 7 ? 0 : 1; }\n')
    head = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n' % header
    src = tmp_path / "view.c"
    src.write_text(head + use + main)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INC, "-fsyntax-only", str(src)])
    src.write_text(head + main)                                                  # (the program itself calls nothing: no library to link)
    exe = tmp_path / "view"
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    V = solver.OccMapSharedView
    assert out[:1 + len(FIELDS)] == [ctypes.sizeof(V)] + [getattr(V, f).offset for f in FIELDS]
    assert out[1 + len(FIELDS):] == [solver.OCCMAP_VIEW_MAX_GROUPS, solver.OCCMAP_VIEW_LAUNCHES, solver.CORRIDOR_MAX_CELLS, solver.CORRIDOR_MAX_POINTS]


def test_the_symbols_are_exported_and_checked_at_load():
    lib = solver.lib()
    assert solver.VIEW_EXPORTS == NAMES
    for n in NAMES:
        assert hasattr(lib, n), n
    assert lib.frp_nmpc_abi_version() == 7 and solver.ABI_VERSION == 7
    assert callable(solver.OccupancyMap.shared_view_device) and callable(solver.SharedView.update) and callable(solver.SharedView.overflowed)


def _map_desc():
    m = solver.OccMap()
    m.origin[:] = (-20.0, -20.0, -1.0); m.map_size[:] = (40.0, 40.0, 5.0); m.resolution = 0.1; m.grid[:] = (400, 400, 50)
    m.clamp_min_log, m.clamp_max_log, m.min_occupancy_log = -1.0, 2.0, 1.70
    m.local_radius[:] = (6.0, 6.0, 3.0)
    m.log_odds = 0x1000; m.occ = 0x2000   # never dereferenced on the host; nothing is launched in these tests
    return m


def _view(**kw):
    """Fake device pointers: nothing behind them is ever read on the host."""
    v = solver.OccMapSharedView()
    v.cap, v.cell = solver.CORRIDOR_MAX_POINTS, 0.5
    v.dims[:] = (80, 80, 10)
    for i, f in enumerate(FIELDS[3:]):
        setattr(v, f, 0x100000 * (i + 1))
    for k, x in kw.items():
        if k == "dims":
            v.dims[:] = x
        else:
            setattr(v, k, x)
    return v


def _update(lib, m, v, ws_bytes, ws=0x5000):
    return lib.frp_nmpc_occmap_shared_view_update(ctypes.byref(m) if m is not None else None, ctypes.byref(v) if v is not None else None,
                                                  ctypes.c_void_p(ws), ws_bytes, None)


REFUSED = {"cap 0": dict(cap=0), "negative cap": dict(cap=-1), "cap above the limit": dict(cap=solver.CORRIDOR_MAX_POINTS + 1),
           "cell 0": dict(cell=0.0), "negative cell": dict(cell=-0.5), "NaN cell": dict(cell=NAN), "infinite cell": dict(cell=INF),
           "too many cells": dict(cell=0.1, dims=(400, 400, 50)),             # 8 000 000 > FRP_CORRIDOR_MAX_CELLS
           "dims of another cell size": dict(dims=(40, 40, 5)), "dims one short": dict(dims=(80, 80, 9))}
REFUSED.update({"null " + f: {f: None} for f in FIELDS[3:]})


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_update_refuses_bad_arguments_before_touching_a_device(what):
    lib = solver.lib()
    m = _map_desc()
    ws = lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    assert _update(lib, m, _view(**REFUSED[what]), ws) == FRP_ERR_ARG


def test_update_refuses_a_bad_map_a_null_view_and_a_short_workspace_and_dims_states_the_grid():
    lib = solver.lib()
    m, good = _map_desc(), _view()
    ws = lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    bad_map = _map_desc(); bad_map.grid[2] = 51
    assert _update(lib, bad_map, good, ws) == FRP_ERR_ARG and _update(lib, None, good, ws) == FRP_ERR_ARG
    assert _update(lib, m, None, ws) == FRP_ERR_ARG
    assert _update(lib, m, good, ws - 1) == FRP_ERR_ARG and _update(lib, m, good, ws, ws=0) == FRP_ERR_ARG
    d = (ctypes.c_int * 3)(-1, -1, -1)
    pm = ctypes.byref(m)
    assert lib.frp_nmpc_occmap_shared_view_dims(pm, 0.5, ctypes.byref(d)) == FRP_OK and tuple(d) == (80, 80, 10)
    assert lib.frp_nmpc_occmap_shared_view_dims(pm, 0.3, ctypes.byref(d)) == FRP_OK and tuple(d) == (134, 134, 17)   # ceil, as shared_view()
    assert lib.frp_nmpc_occmap_shared_view_dims(pm, 100.0, ctypes.byref(d)) == FRP_OK and tuple(d) == (1, 1, 1)
    for cell in (0.0, -0.5, NAN, INF, 0.1, 1e-300):
        assert lib.frp_nmpc_occmap_shared_view_dims(pm, cell, ctypes.byref(d)) == FRP_ERR_ARG, cell
    assert tuple(d) == (1, 1, 1)                                                 # a refused call leaves dims alone
    assert lib.frp_nmpc_occmap_shared_view_dims(pm, 0.5, None) == FRP_ERR_ARG
    assert lib.frp_nmpc_occmap_shared_view_dims(None, 0.5, ctypes.byref(d)) == FRP_ERR_ARG
    assert lib.frp_nmpc_occmap_shared_view_dims(ctypes.byref(bad_map), 0.5, ctypes.byref(d)) == FRP_ERR_ARG


def _has_gpu():
    try:
        return solver.lib().frp_nmpc_device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="checks the behaviour of a machine WITHOUT a device")
def test_valid_update_arguments_report_no_device():
    lib = solver.lib()
    m = _map_desc()
    ws = lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    for v in (_view(), _view(cap=1), _view(cell=100.0, dims=(1, 1, 1)), _view(cell=0.125, dims=(320, 320, 40))):   # 4 096 000 cells: under the limit
        assert _update(lib, m, v, ws) == FRP_ERR_NO_DEVICE


def _corridor_args():
    cr = solver.Corridor()
    cr.B, cr.N, cr.F, cr.P = 4, 20, 64, 1000
    for f in ("cloud", "cloud_count", "ref_pos", "ref_yaw", "ellipsoid", "poly_A", "poly_b", "poly_nfaces", "poly_index"):
        setattr(cr, f, 8)   # any non-NULL address: the checks must fail before it would be dereferenced on the device
    cr.bbox = (ctypes.c_double * 3)(2, 2, 1); cr.seed_len = 0.1; cr.inflation = 1.1
    cr.grid_origin = (ctypes.c_double * 3)(-10, -10, -1); cr.grid_cell = 0.5; cr.grid_dims = (ctypes.c_int * 3)(40, 40, 8)
    cr.grid_points = 8; cr.grid_index = 8; cr.grid_start = 8
    return cr


def _cut(box=8, origin=(-10.0, -10.0, -1.0), resolution=0.1):
    return solver.CorridorCut(box, (ctypes.c_double * 3)(*origin), resolution)


def test_corridor_view_entry_refuses_bad_arguments_before_touching_a_device():
    l = solver.lib()
    call = lambda cr, cut: l.frp_nmpc_corridor_batch_view(ctypes.byref(cr), ctypes.byref(cut) if cut is not None else None, None)
    cr = _corridor_args()
    for cut in (_cut(), None):
        cr.cloud_count = None
        assert call(cr, cut) == FRP_ERR_ARG                                      # the device-side count is what the entry is for
        cr.cloud_count = 8
        cr.cloud_per_planner = 1
        assert call(cr, cut) == FRP_ERR_ARG                                      # the view is a shared cloud
        cr.cloud_per_planner = 0
        # every bad-field case of frp_nmpc_corridor_batch, through the new entry
        for field, bad in (("F", 5), ("F", 65), ("N", 0), ("N", 65), ("P", 65537), ("P", -1), ("seed_len", 0.0), ("poly_index", None), ("cloud", None),
                           ("B", 0), ("inflation", -1.0), ("ref_pos", None), ("ellipsoid", None), ("grid_points", None), ("grid_index", None),
                           ("grid_cell", 0.0)):
            keep = getattr(cr, field)
            setattr(cr, field, bad)
            assert call(cr, cut) == FRP_ERR_ARG, field
            setattr(cr, field, keep)
    # the cut's own checks
    assert call(cr, _cut(box=None)) == FRP_ERR_ARG
    for res in (0.0, -0.1, NAN, INF):
        assert call(cr, _cut(resolution=res)) == FRP_ERR_ARG, res
    assert call(cr, _cut(origin=(NAN, -10.0, -1.0))) == FRP_ERR_ARG
    assert l.frp_nmpc_corridor_batch_view(None, ctypes.byref(_cut()), None) == FRP_ERR_ARG
    # the existing entry points are as they were: a missing count is no error there
    cr.cloud_count = None
    cr.grid_start = None
    cr.P = 65537
    assert l.frp_nmpc_corridor_batch_cut(ctypes.byref(cr), ctypes.byref(_cut()), None) == FRP_ERR_ARG
