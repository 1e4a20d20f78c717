"""CPU tests of the corridor's per-planner visibility cut (include/frp_nmpc.h (5): frp_nmpc_corridor_cut,
frp_nmpc_corridor_batch_cut): the argument checks that run before a device is touched, the header and its ctypes mirror, and --
on the oracles alone -- the definition itself: the whole-map cloud cut in POSITION form by a planner's local_box is that planner's
local cloud, order included, and on the tunnel world the cut changes the polytopes."""
import ctypes
import os
import subprocess
import sys

import numpy as np

from forces_resilient_planner_amd import solver
from tests import occmap_oracle as OO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
GEO = dict(origin=(-10.0, -10.0, -1.0), map_size=(20.0, 20.0, 4.0), resolution=0.1)
ERR = -1003


def _corridor_args():
    cr = solver.Corridor()
    cr.B, cr.N, cr.F, cr.P = 4, 20, 64, 100
    for f in ("cloud", "ref_pos", "ref_yaw", "ellipsoid", "poly_A", "poly_b", "poly_nfaces", "poly_index"):
        setattr(cr, f, 8)   # any non-NULL address: the checks must fail before it would be dereferenced on the device
    cr.bbox = (ctypes.c_double * 3)(2, 2, 1); cr.seed_len = 0.1; cr.inflation = 1.1
    return cr


def _cut(box=8, origin=(-10.0, -10.0, -1.0), resolution=0.1):
    return solver.CorridorCut(box, (ctypes.c_double * 3)(*origin), resolution)


def test_cut_entry_point_rejects_bad_arguments_before_touching_a_device():
    l = solver.lib()
    call = lambda cr, cut: l.frp_nmpc_corridor_batch_cut(ctypes.byref(cr), ctypes.byref(cut) if cut is not None else None, None)
    cr = _corridor_args()
    assert call(cr, _cut(box=None)) == ERR
    for res in (0.0, -0.1, float("nan"), float("inf")):
        assert call(cr, _cut(resolution=res)) == ERR, res
    for k in range(3):
        for bad in (float("inf"), -float("inf"), float("nan")):
            o = [-10.0, -10.0, -1.0]; o[k] = bad
            assert call(cr, _cut(origin=o)) == ERR, (k, bad)
    cr.cloud_per_planner = 1
    assert call(cr, _cut()) == ERR                                             # the cut belongs to a shared cloud
    cr.cloud_per_planner = 0
    # every bad-field case of frp_nmpc_corridor_batch, through the new entry with a valid cut -- and with no cut at all
    for cut in (_cut(), None):
        for field, bad in (("F", 5), ("F", 65), ("N", 0), ("N", 65), ("P", 65537), ("seed_len", 0.0), ("poly_index", None), ("cloud", None),
                           ("B", 0), ("inflation", -1.0), ("ref_pos", None), ("ellipsoid", None)):
            keep = getattr(cr, field)
            setattr(cr, field, bad)
            assert call(cr, cut) == ERR, field
            setattr(cr, field, keep)
        cr.grid_start = 8                                                       # a grid without its other arrays / cell size
        assert call(cr, cut) == ERR
        cr.grid_start = None
    assert l.frp_nmpc_corridor_batch_cut(None, ctypes.byref(_cut()), None) == ERR


def test_header_compiles_as_c99_and_the_mirror_has_its_layout(tmp_path):
    src = tmp_path / "cut.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "frp_nmpc.h"\n'
                   'int main(void) { frp_nmpc_corridor_cut c; c.box = 0; c.origin[2] = 0.0; c.resolution = 0.1; (void)c;\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(frp_nmpc_corridor_cut), offsetof(frp_nmpc_corridor_cut, box),\n'
                   '         offsetof(frp_nmpc_corridor_cut, origin), offsetof(frp_nmpc_corridor_cut, resolution));\n'
                   '  return FRP_NMPC_ABI_VERSION == 7 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INC, "-fsyntax-only", str(src)])
    exe = tmp_path / "cut"
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", str(exe)])
    size, o_box, o_origin, o_res = (int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    C = solver.CorridorCut
    assert (ctypes.sizeof(C), C.box.offset, C.origin.offset, C.resolution.offset) == (size, o_box, o_origin, o_res)
    assert solver.lib().frp_nmpc_abi_version() == 7 and solver.ABI_VERSION == 7
    assert "frp_nmpc_corridor_batch_cut" in solver.EXPORTS


def tunnel_inputs(seed, B, N=20, P=6000):
    """The host half of tests/test_gpu_occmap.py::_tunnel_world, draw for draw: the float32 cloud, stage references, yaws and the
    plan rows the tube is made from."""
    rng = np.random.default_rng(seed)
    cloud = np.c_[rng.uniform(-3, 9, P), rng.uniform(-4, 4, P), rng.uniform(-0.5, 3, P)]
    s = np.linspace(0, 5, N)
    centre = np.c_[s, 0.4 * np.sin(0.8 * s), 1.0 + 0.1 * np.cos(s)]
    cx = np.interp(cloud[:, 0], centre[:, 0], centre[:, 1]); cz = np.interp(cloud[:, 0], centre[:, 0], centre[:, 2])
    cloud = cloud[np.hypot(cloud[:, 1] - cx, cloud[:, 2] - cz) > 0.75].astype(np.float32)
    ref = centre[None] + rng.normal(0, 0.03, (B, N, 3))
    yaw = np.arctan2(np.gradient(centre[:, 1]), np.gradient(centre[:, 0]))[None] + rng.normal(0, 0.05, (B, N))
    z = np.zeros((B, N, 17)); z[..., 3] = 7.3; z[..., 8:11] = ref; z[..., 16] = yaw
    z[..., 11:14] = rng.normal(0, 0.5, (B, N, 3)); z[..., 14:16] = rng.normal(0, 0.1, (B, N, 2))
    return cloud, ref, yaw, z


def cut_by_position(om, cloud, box):
    """frp_nmpc_corridor_cut's rule, as the header states it: lo <= q < hi per axis, lo / hi = origin + id * resolution (one multiply,
    one add); a NaN compares false."""
    box = np.asarray(box)
    lo = om.origin + box[:3].astype(np.float64) * om.resolution
    hi = om.origin + box[3:].astype(np.float64) * om.resolution
    with np.errstate(invalid="ignore"):
        keep = np.all((lo <= cloud) & (cloud < hi), axis=1)
    return cloud[keep]


def test_whole_map_cloud_cut_by_position_is_the_local_cloud_and_changes_the_corridor():
    B = 4
    cloud, ref, yaw, z = tunnel_inputs(61, B)
    radius = (4.0, 3.0, 3.0)
    om = OO.OccMapOracle(local_radius=radius, **GEO)
    om.insert_cloud(cloud)
    whole = om.local_cloud(None)
    assert len(whole) == 5568
    # the condition under which a voxel centre's float32 rounding cannot carry it across a bound (include/frp_nmpc.h)
    assert (np.abs(om.origin).max() + om.map_size.max()) * 2.0 ** -23 < om.resolution / 2
    centres = {"p0": ref[0, 0], "p1": ref[1, 0], "p2": ref[2, 0], "p3": ref[3, 0], "end": ref[0, -1],
               "top face": np.array([2.0, 0.0, 2.95]), "bottom face": np.array([2.0, 0.5, -0.95]), "x face": np.array([-9.95, 0.0, 1.0]),
               "corner": np.array([9.97, 9.97, 2.95]), "on the origin": np.array([0.0, -10.0, -1.0]),
               "above the map": np.array([2.0, 0.0, 4.5]),          # outside the map, its range still reaches in
               "far away": np.array([100.0, 0.0, 1.0]),             # outside, range empty: min_id > max_id
               "below the map": np.array([0.0, 0.0, -6.0])}         # an empty z range
    sizes = {}
    for name, c in centres.items():
        box = om.local_box(c)
        want = om.local_cloud(c)
        got = cut_by_position(om, whole, box)
        assert np.array_equal(got, want), (name, len(got), len(want))
        sizes[name] = len(want)
    assert sizes["p0"] == 2252 and sizes["far away"] == 0 and sizes["below the map"] == 0
    assert all(0 < sizes[k] < len(whole) for k in ("p1", "end", "top face", "bottom face", "above the map")), sizes
    far = om.local_box(centres["far away"])
    assert any(far[k] > far[3 + k] for k in range(3))
    assert np.array_equal(cut_by_position(om, whole, om.local_box(None)), whole)      # the whole-map row hides nothing
    # ... and the cut matters: without it the corridor of some planner is another one
    sys.path.insert(0, ROOT)
    from oracle import corridor_oracle as C, tube_oracle as T
    E = T.tube_batch(z)
    differs = []
    for p in range(B):
        idx_c, polys_c = C.corridor_one(ref[p], yaw[p], E[p], om.local_cloud(ref[p, 0]))
        idx_w, polys_w = C.corridor_one(ref[p], yaw[p], E[p], whole)
        same = np.array_equal(idx_c, idx_w) and len(polys_c) == len(polys_w) and all(
            a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(polys_c, polys_w))
        differs.append(not same)
    assert any(differs), differs
