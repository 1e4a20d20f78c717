"""CPU tests of the shared-cloud route beyond FRP_CORRIDOR_MAX_POINTS (include/frp_nmpc_corridor_large.h: frp_nmpc_corridor_large,
frp_nmpc_corridor_large_workspace_bytes, frp_nmpc_corridor_batch_large, frp_nmpc_occmap_shared_view_update_large): the header as C and
as C++, its ctypes mirror and constants, the exports, and every refusal that is made before a device is touched -- and that the existing
entries keep their limit."""
import ctypes
import os
import subprocess

import pytest

from forces_resilient_planner_amd import solver
from tests.test_occmap_shared_view_cpu import _corridor_args, _cut, _has_gpu, _map_desc, _view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
FRP_OK, FRP_ERR_NO_DEVICE, FRP_ERR_ARG = 0, -1001, -1003
NAN, INF = float("nan"), float("inf")
NAMES = ["frp_nmpc_corridor_large_workspace_bytes", "frp_nmpc_corridor_batch_large", "frp_nmpc_occmap_shared_view_update_large"]
FIELDS = [f for f, _ in solver.CorridorLarge._fields_]
LIST_BYTES = 4 * solver.CORRIDOR_LARGE_LIST


@pytest.mark.parametrize("lang", ["c", "c++"])
@pytest.mark.parametrize("header", ["frp_nmpc.h", "frp_nmpc_corridor_large.h", "frp_nmpc_occmap_view.h"])
def test_header_compiles_as_c_and_as_cpp_and_the_mirror_has_its_layout(tmp_path, header, lang):
    hdr = open(os.path.join(INC, "frp_nmpc.h")).read()
    own = open(os.path.join(INC, "frp_nmpc_corridor_large.h")).read()
    assert '#include "frp_nmpc_corridor_large.h"' in hdr and "#define FRP_NMPC_ABI_VERSION 7" in hdr   # no existing struct changed
    for n in NAMES:
        assert n + "(" in own and n + "(" not in hdr
    offs = ", ".join(f"offsetof(frp_nmpc_corridor_large, {f})" for f in FIELDS)
    use = ('int use(const frp_nmpc_occmap *m, const frp_nmpc_occmap_shared_view *v, const frp_nmpc_corridor *p, const frp_nmpc_corridor_cut *c,\n'
           '        const frp_nmpc_corridor_large *w, void *ws) {\n'
           '  return (int)frp_nmpc_corridor_large_workspace_bytes(4) + frp_nmpc_corridor_batch_large(p, c, w, 0)\n'
           '       + frp_nmpc_occmap_shared_view_update_large(m, v, ws, 0, 0); }\n')
    main = ('int main(void) { size_t o[] = {sizeof(frp_nmpc_corridor_large), %s}; size_t i;\n' % offs +
            '  for (i = 0; i < sizeof o / sizeof o[0]; i++) printf("%lu ", (unsigned long)o[i]);\n'
            '  printf("%d %d %d %d\\n", FRP_CORRIDOR_LARGE_MAX_POINTS, FRP_CORRIDOR_LARGE_LIST, FRP_CORRIDOR_LARGE_GROUPS, FRP_CORRIDOR_MAX_POINTS);\n'
            '  return 0; }\n')
    head = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n' % header
    cc = ["gcc", "-std=c99", "-pedantic"] if lang == "c" else ["g++", "-std=c++11", "-x", "c++"]
    src = tmp_path / "large.c"
    src.write_text(head + use + main)
    subprocess.check_call(cc + ["-Wall", "-Werror", "-I", INC, "-fsyntax-only", str(src)])
    src.write_text(head + main)                                                  # (the program itself calls nothing: no library to link)
    exe = tmp_path / "large"
    subprocess.check_call(cc + ["-I", INC, str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    W = solver.CorridorLarge
    assert out[:1 + len(FIELDS)] == [ctypes.sizeof(W)] + [getattr(W, f).offset for f in FIELDS]
    assert out[1 + len(FIELDS):] == [solver.CORRIDOR_LARGE_MAX_POINTS, solver.CORRIDOR_LARGE_LIST, solver.CORRIDOR_LARGE_GROUPS, solver.CORRIDOR_MAX_POINTS]
    assert out[1 + len(FIELDS):] == [1 << 22, 65536, 512, 65536]


def test_the_symbols_are_exported_and_checked_at_load_and_the_wrappers_exist():
    lib = solver.lib()
    assert solver.LARGE_EXPORTS == NAMES
    for n in NAMES:
        assert hasattr(lib, n), n
    assert lib.frp_nmpc_abi_version() == 7 and solver.ABI_VERSION == 7
    assert callable(solver.SharedView._large_args)


def test_workspace_bytes_is_monotone_and_constant_from_512_planners_on():
    wb = solver.lib().frp_nmpc_corridor_large_workspace_bytes
    assert wb(0) == 0 and wb(-3) == 0
    sizes = [wb(B) for B in range(1, 700)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[:512] == [LIST_BYTES * B for B in range(1, 513)]                # one list per workgroup, min(B, 512) workgroups
    assert set(sizes[511:]) == {128 << 20} and wb(4096) == wb(1 << 30) == 128 << 20


def _large(B=4, **kw):
    w = solver.CorridorLarge(0x7000, solver.lib().frp_nmpc_corridor_large_workspace_bytes(B), 0x9000)
    for k, x in kw.items():
        setattr(w, k, x)
    return w


def _call(cr, cut, w):
    return solver.lib().frp_nmpc_corridor_batch_large(ctypes.byref(cr) if cr is not None else None, ctypes.byref(cut) if cut is not None else None,
                                                      ctypes.byref(w) if w is not None else None, None)


@pytest.mark.parametrize("with_cut", [True, False])
@pytest.mark.parametrize("count", [8, None])
def test_corridor_large_refuses_bad_arguments_before_anything_is_launched(with_cut, count):
    cr = _corridor_args()
    cr.cloud_count = count
    cut = _cut() if with_cut else None
    # everything frp_nmpc_corridor_batch_cut refuses other than P <= FRP_CORRIDOR_MAX_POINTS
    for field, bad in (("F", 5), ("F", 65), ("N", 0), ("N", 65), ("P", -1), ("P", solver.CORRIDOR_LARGE_MAX_POINTS + 1), ("seed_len", 0.0), ("seed_len", NAN),
                       ("poly_index", None), ("poly_nfaces", None), ("poly_A", None), ("poly_b", None), ("cloud", None), ("B", 0), ("B", -1),
                       ("inflation", -1.0), ("inflation", NAN), ("ref_pos", None), ("ref_yaw", None), ("ellipsoid", None), ("grid_points", None),
                       ("grid_index", None), ("grid_cell", 0.0), ("grid_cell", NAN),
                       ("cloud_per_planner", 1),                                  # the large route is a shared cloud
                       ("grid_start", None)):                                     # ... with its grid
        keep = getattr(cr, field)
        setattr(cr, field, bad)
        assert _call(cr, cut, _large()) == FRP_ERR_ARG, field
        setattr(cr, field, keep)
    for k in range(3):
        keep = cr.grid_dims[k]
        cr.grid_dims[k] = 0
        assert _call(cr, cut, _large()) == FRP_ERR_ARG, ("grid_dims", k)
        cr.grid_dims[k] = keep
    cr.bbox = (ctypes.c_double * 3)(0, 0, 0)                                     # ... and a local box
    assert _call(cr, cut, _large()) == FRP_ERR_ARG
    cr.bbox = (ctypes.c_double * 3)(2, 2, 1)
    # the workspace
    assert _call(cr, cut, None) == FRP_ERR_ARG
    assert _call(cr, cut, _large(workspace=None)) == FRP_ERR_ARG
    assert _call(cr, cut, _large(workspace_bytes=4 * LIST_BYTES - 1)) == FRP_ERR_ARG
    assert _call(cr, cut, _large(workspace_bytes=0)) == FRP_ERR_ARG
    cr.B = 600
    assert _call(cr, cut, _large(workspace_bytes=512 * LIST_BYTES - 1)) == FRP_ERR_ARG
    cr.B = 4
    assert _call(None, cut, _large()) == FRP_ERR_ARG
    if with_cut:
        assert _call(cr, _cut(box=None), _large()) == FRP_ERR_ARG
        for res in (0.0, -0.1, NAN, INF):
            assert _call(cr, _cut(resolution=res), _large()) == FRP_ERR_ARG, res
        for k in range(3):
            o = [-10.0, -10.0, -1.0]; o[k] = NAN
            assert _call(cr, _cut(origin=tuple(o)), _large()) == FRP_ERR_ARG


def _update_large(m, v, ws_bytes, ws=0x5000):
    return solver.lib().frp_nmpc_occmap_shared_view_update_large(ctypes.byref(m) if m is not None else None, ctypes.byref(v) if v is not None else None,
                                                                 ctypes.c_void_p(ws), ws_bytes, None)


VIEW_FIELDS = [f for f, _ in solver.OccMapSharedView._fields_]
REFUSED = {"cap 0": dict(cap=0), "negative cap": dict(cap=-1), "cap above the large limit": dict(cap=solver.CORRIDOR_LARGE_MAX_POINTS + 1),
           "cell 0": dict(cell=0.0), "negative cell": dict(cell=-0.5), "NaN cell": dict(cell=NAN), "infinite cell": dict(cell=INF),
           "too many cells": dict(cell=0.1, dims=(400, 400, 50)), "dims of another cell size": dict(dims=(40, 40, 5)), "dims one short": dict(dims=(80, 80, 9))}
REFUSED.update({"null " + f: {f: None} for f in VIEW_FIELDS[3:]})


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_update_large_refuses_what_the_update_refuses(what):
    m = _map_desc()
    ws = solver.lib().frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    assert _update_large(m, _view(**REFUSED[what]), ws) == FRP_ERR_ARG


def test_update_large_refuses_a_bad_map_a_null_view_and_a_short_workspace():
    m, good = _map_desc(), _view(cap=100000)
    ws = solver.lib().frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    bad_map = _map_desc(); bad_map.grid[2] = 51
    assert _update_large(bad_map, good, ws) == FRP_ERR_ARG and _update_large(None, good, ws) == FRP_ERR_ARG
    assert _update_large(m, None, ws) == FRP_ERR_ARG
    assert _update_large(m, good, ws - 1) == FRP_ERR_ARG and _update_large(m, good, ws, ws=0) == FRP_ERR_ARG


@pytest.mark.skipif(_has_gpu(), reason="checks the behaviour of a machine WITHOUT a device")
def test_65537_points_are_no_argument_error_for_the_large_entries():
    """P = cap = 65537 passes every check of the new entries: what comes back is the missing device, as from the existing calls with
    valid arguments (tests/test_occmap_shared_view_cpu.py::test_valid_update_arguments_report_no_device)."""
    m = _map_desc()
    ws = solver.lib().frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    for cap in (1, 65536, 65537, solver.CORRIDOR_LARGE_MAX_POINTS):
        assert _update_large(m, _view(cap=cap), ws) == FRP_ERR_NO_DEVICE, cap
    cr = _corridor_args()
    for P in (0, 1000, 65536, 65537, solver.CORRIDOR_LARGE_MAX_POINTS):
        cr.P = P
        for cut in (_cut(), None):
            for count in (8, None):
                cr.cloud_count = count
                assert _call(cr, cut, _large()) == FRP_ERR_NO_DEVICE, (P, cut is not None, count)
    assert _call(cr, _cut(), _large(overflow=None)) == FRP_ERR_NO_DEVICE        # overflow may be NULL


def test_the_existing_entries_still_refuse_65537_points():
    l = solver.lib()
    m = _map_desc()
    ws = l.frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    v = _view(cap=65537)
    assert l.frp_nmpc_occmap_shared_view_update(ctypes.byref(m), ctypes.byref(v), ctypes.c_void_p(0x5000), ws, None) == FRP_ERR_ARG
    cr = _corridor_args()
    cr.P = 65537
    assert l.frp_nmpc_corridor_batch_view(ctypes.byref(cr), ctypes.byref(_cut()), None) == FRP_ERR_ARG
    assert l.frp_nmpc_corridor_batch_view(ctypes.byref(cr), None, None) == FRP_ERR_ARG
    assert l.frp_nmpc_corridor_batch_cut(ctypes.byref(cr), ctypes.byref(_cut()), None) == FRP_ERR_ARG
    cr.cloud_count = None
    assert l.frp_nmpc_corridor_batch_cut(ctypes.byref(cr), ctypes.byref(_cut()), None) == FRP_ERR_ARG
    assert l.frp_nmpc_corridor_batch(ctypes.byref(cr), None) == FRP_ERR_ARG
    cr.grid_start = None
    assert l.frp_nmpc_corridor_batch(ctypes.byref(cr), None) == FRP_ERR_ARG
    ov = solver.OccMapView()
    names = [f for f, _ in solver.OccMapView._fields_]
    assert "P" in names
    for f, t in solver.OccMapView._fields_:
        if t is ctypes.c_void_p:
            setattr(ov, f, 0x3000)
    ov.B, ov.P = 1, 65537
    assert l.frp_nmpc_occmap_local_view(ctypes.byref(m), ctypes.byref(ov), ctypes.c_void_p(0x5000), ws, None) == FRP_ERR_ARG
    with pytest.raises(ValueError):
        solver.SharedView.__init__(solver.SharedView.__new__(solver.SharedView), _FakeMap(), solver.CORRIDOR_LARGE_MAX_POINTS + 1)
    assert "CORRIDOR_MAX_POINTS" in solver.OccupancyMap.shared_view.__doc__      # the host-side shared_view() keeps its limit


class _FakeMap:
    """Enough of an OccupancyMap for SharedView's capacity check, which comes before anything touches a device."""
    torch = None
