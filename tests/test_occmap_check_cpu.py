"""CPU tests of the safety timer's checks on the occupancy map (include/frp_nmpc_occmap_check.h): known answers for the restatement
(tests/occmap_check_oracle.py) that the GPU tests compare the device against, the goal-search table of
solver.goal_search_table(), and the boundary of the three calls as far as it exists without a device."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from forces_resilient_planner_amd import solver
from tests import occmap_check_oracle as CO
from tests import occmap_oracle as OO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN_GEO = dict(origin=(-1.6, -1.6, 0.0), map_size=(3.2, 3.2, 0.8), resolution=0.1)
KNOWN_VOXEL = (16, 16, 4)


def known_map():
    """32 x 32 x 8 voxels of 0.1 m with the single occupied voxel KNOWN_VOXEL."""
    m = OO.OccMapOracle(**KNOWN_GEO)
    assert tuple(m.grid_size) == (32, 32, 8)
    m.buffer[KNOWN_VOXEL] = m.clamp_max_log
    return m


def corner_cases(m, ratio):
    """[(position, free?)] around KNOWN_VOXEL for the launch file's body: the centre of the voxel from which the probe corner
    (+hx, +hy, +hz) -- then (-hx, -hy, -hz) -- is exactly the occupied voxel collides; one voxel further away along x, along z
    and along both it is free.  Centres keep every probe half a voxel away from a face, and every probe stays inside the map."""
    h = CO.half_extents(m, ratio)
    assert h == {1.2: (4, 4, 1), 1.5: (5, 5, 1)}[ratio]   # ceil(3.24), ceil(0.51); ceil(4.05), ceil(0.6375)
    cases = []
    for s in (-1, 1):   # the point sits on the low side (its + corner touches) or on the high side (its - corner touches)
        at = tuple(KNOWN_VOXEL[a] + s * h[a] for a in range(3))
        cases.append((m.index_to_pos(at), False))
        for d in ((s, 0, 0), (0, 0, s), (s, 0, s)):
            cases.append((m.index_to_pos(tuple(at[a] + d[a] for a in range(3))), True))
    return cases


def brute_force_free(m, pos, ratio, box=None, body=(0.27, 0.0425)):
    """Every probe's state first, the verdict afterwards: no early exit, no shared loop body with the restatement."""
    hx, hy, hz = (int(math.ceil(e * ratio / float(m.resolution))) for e in (body[0], body[0], body[1]))
    states = [m.get_voxel_state(np.array([pos[0] + i * float(m.resolution), pos[1] + j * float(m.resolution), pos[2] + k * float(m.resolution)]), box)
              for i in range(-hx, hx + 1) for j in range(-hy, hy + 1) for k in range(-hz, hz + 1)]
    assert len(states) == (2 * hx + 1) * (2 * hy + 1) * (2 * hz + 1)
    return all(s == 0 for s in states)


def test_check_pos_surround_equals_a_brute_force_loop():
    rng = np.random.default_rng(3)
    m = OO.OccMapOracle(origin=(-1.2, -1.0, 0.0), map_size=(2.4, 2.0, 1.2), resolution=0.1, local_radius=(0.5, 0.4, 0.3))
    m.buffer[rng.random(m.buffer.shape) < 0.0015] = m.clamp_max_log
    pts = np.c_[rng.uniform(-0.9, 0.9, 200), rng.uniform(-0.7, 0.7, 200), rng.uniform(0.0, 1.2, 200)]   # mostly inside; some probes leave the map
    pts[:20] = np.round(pts[:20] * 10) / 10   # on voxel faces
    box = m.local_box((0.1, -0.1, 0.6))
    got = [[CO.check_pos_surround(m, p, r, b) for p in pts] for r, b in ((1.2, None), (1.5, None), (1.2, box))]
    want = [[brute_force_free(m, p, r, b) for p in pts] for r, b in ((1.2, None), (1.5, None), (1.2, box))]
    assert got == want
    for g in got:
        assert 30 < sum(g) < 170   # neither verdict is rare
    assert got[0] != got[2]        # the local box hides obstacles from some points


@pytest.mark.parametrize("ratio", [1.2, 1.5])
def test_single_voxel_known_answers(ratio):
    m = known_map()
    cases = corner_cases(m, ratio)
    assert len(cases) == 8 and [f for _, f in cases] == [False, True, True, True] * 2
    for pos, free in cases:
        assert CO.check_pos_surround(m, pos, ratio) is free, (pos, ratio)
    # an empty map: all of them are free; a point whose probes leave the map collides with nothing occupied anywhere
    m.reset()
    assert all(CO.check_pos_surround(m, pos, ratio) for pos, _ in cases)
    assert not CO.check_pos_surround(m, m.index_to_pos((2, 16, 4)), ratio)
    assert not CO.check_pos_surround(m, (float("nan"), 0.0, 0.4), ratio)


def test_goal_search_table_is_the_three_loops():
    tab, n_groups, group_size = solver.goal_search_table()
    rows = []
    sizes = []
    r = 0.2
    while r <= 5 * 0.2 + 1e-3:
        theta = -90.0
        while theta <= 270:
            nz, n = 1.0, 0
            while nz <= 1.6:
                rows.append((r * math.cos(theta), r * math.sin(theta), nz))
                nz += 0.2; n += 1
            sizes.append(n)
            theta += 30
        r += 0.2
    assert (n_groups, group_size) == (65, 4) and sizes == [4] * 65          # 5 radii x 13 angles; 1.0 + 0.2 + 0.2 + 0.2 <= 1.6 in double
    assert tab.dtype == np.float64 and tab.shape == (260, 3) and np.array_equal(tab, np.array(rows))
    orows, osizes = CO.goal_search_table()
    assert np.array_equal(tab, np.array(orows)) and osizes == sizes
    assert np.array_equal(tab[:4, 2], [1.0, 1.2, 1.4, 1.0 + 0.2 + 0.2 + 0.2]) and tab[3, 2] < 1.6
    # theta counts degrees and is used as radians: the first group is r * cos(-90 rad), not r * cos(-pi / 2) = 0
    assert tab[0, 0] == 0.2 * math.cos(-90.0) and abs(tab[0, 0]) > 0.08
    assert tab[-1, 0] == (0.2 + 0.2 + 0.2 + 0.2 + 0.2) * math.cos(270.0)


def walk_table(m, end_pt, tab, n_groups, group_size, box=None):
    """The goal walk as frp_nmpc_occmap_check_goals states it, over a table."""
    e = np.array(end_pt, dtype=np.float64)
    if CO.check_pos_surround(m, e, 1.2, box):
        return e, 0, 0
    hits = 0
    for g in range(n_groups):
        for k in range(group_size):
            t = tab[g * group_size + k]
            cand = np.array([e[0] + t[0], e[1] + t[1], t[2]])
            if CO.check_pos_surround(m, cand, 1.5, box):
                e = cand; hits += 1
                break
    return e, 1, hits


def two_pocket_map():
    """A solid map with two pockets, each exactly the probe box (ratio 1.5) of one candidate: A = candidate 13 (group 3: r = 0.2,
    theta = 0, nz = 1.2) seen from the goal, B = candidate 120 (group 30: r = 0.6, theta = 30, nz = 1.0) seen from A.  Returns
    (map, goal, table, A, B)."""
    m = OO.OccMapOracle(origin=(-1.6, -1.6, 0.0), map_size=(3.2, 3.2, 2.0), resolution=0.1)
    m.buffer[...] = m.clamp_max_log
    tab, _, _ = solver.goal_search_table()
    goal = np.array([0.05, 0.05, 0.55])
    A = np.array([goal[0] + tab[13, 0], goal[1] + tab[13, 1], tab[13, 2]])
    B = np.array([A[0] + tab[120, 0], A[1] + tab[120, 1], tab[120, 2]])
    hx, hy, hz = CO.half_extents(m, 1.5)
    for p in (A, B):
        for i in range(-hx, hx + 1):
            for j in range(-hy, hy + 1):
                for k in range(-hz, hz + 1):
                    idx = m.pos_to_index(p + np.array([i, j, k], dtype=np.float64) * m.resolution)
                    assert m.is_in_map(idx)
                    m.buffer[tuple(idx)] = m.clamp_min_log
    return m, goal, tab, A, B


def test_goal_walk_continues_from_the_moved_goal():
    m, goal, tab, A, B = two_pocket_map()
    assert tab[13, 0] == 0.2 and tab[13, 1] == 0.0 and tab[13, 2] == 1.2          # r = 0.2, cos(0), sin(0)
    end, blocked, hits = CO.check_goal(m, goal)
    assert blocked == 1 and hits == 2
    # the second move is relative to the FIRST move, not to the original goal, and z is the table's absolute value
    assert np.array_equal(end, B) and end[0] == (0.05 + 0.2) + tab[120, 0] and end[2] == 1.0
    assert not np.array_equal(end[:2], goal[:2] + tab[120, :2])
    e2, b2, h2 = walk_table(m, goal, *solver.goal_search_table())
    assert np.array_equal(e2, end) and (b2, h2) == (1, 2)
    # no target: untouched; a free goal: untouched; nothing free anywhere: blocked, unchanged
    assert CO.check_goal(m, goal, have_target=False)[1:] == (0, 0)
    e3, b3, h3 = CO.check_goal(m, A)                                              # inside its pocket the smaller body of ratio 1.2 is free
    assert np.array_equal(e3, A) and (b3, h3) == (0, 0)
    m.buffer[...] = m.clamp_max_log
    e4, b4, h4 = CO.check_goal(m, goal)
    assert np.array_equal(e4, goal) and (b4, h4) == (1, 0)
    m.reset()
    e5, b5, h5 = CO.check_goal(m, goal)
    assert np.array_equal(e5, goal) and (b5, h5) == (0, 0)


def test_path_loop_known_answers():
    m = known_map()
    hit = corner_cases(m, 1.2)[0][0]
    free = corner_cases(m, 1.2)[1][0]
    path = np.tile(free, (16, 1))
    assert CO.check_path(m, path, 16) == -1
    path[4] = hit
    assert CO.check_path(m, path, 16) == -1                   # sample 4 is not looked at with stride 5
    path[10] = hit
    assert CO.check_path(m, path, 16) == 10 and CO.check_path(m, path, 10) == -1 and CO.check_path(m, path, 11) == 10
    path[5] = hit
    assert CO.check_path(m, path, 16) == 5 and CO.check_path(m, path, 16, have_traj=False) == -1 and CO.check_path(m, path, 0) == -1
    assert CO.check_path(m, path, 99) == 5                     # a size beyond the storage is cut to it


# ---- the boundary ----
FRP_ERR_NO_DEVICE, FRP_ERR_ARG = -1001, -1003
NAMES = ["frp_nmpc_occmap_check_surround", "frp_nmpc_occmap_check_paths", "frp_nmpc_occmap_check_goals"]


def test_the_three_calls_are_declared_and_exported_and_the_abi_version_stays(tmp_path):
    lib = solver.lib()
    assert solver.CHECK_EXPORTS == NAMES
    for n in NAMES:
        assert hasattr(lib, n), n
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    assert '#include "frp_nmpc_occmap_check.h"' in hdr and "#define FRP_NMPC_ABI_VERSION 7" in hdr
    own = open(os.path.join(ROOT, "include", "frp_nmpc_occmap_check.h")).read()
    for n in NAMES:
        assert n + "(" in own
    lines = [f'_Static_assert(sizeof(frp_nmpc_occmap_body) == {ctypes.sizeof(solver.OccMapBody)}, "size");']
    for fld, _ in solver.OccMapBody._fields_:
        lines.append(f'_Static_assert(offsetof(frp_nmpc_occmap_body, {fld}) == {getattr(solver.OccMapBody, fld).offset}, "{fld}");')
    for inc in ("frp_nmpc.h", "frp_nmpc_occmap_check.h"):   # through frp_nmpc.h, and on its own
        src = tmp_path / ("layout_" + inc.replace(".", "_") + ".c")
        src.write_text('#include <stddef.h>\n#include "' + inc + '"\n' + "\n".join(lines) + "\nint main(void) { return 0; }\n")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(src) + ".o"])


def _has_gpu():
    try:
        return solver.lib().frp_nmpc_device_count() > 0
    except Exception:
        return False


def _desc():
    m = solver.OccMap()
    m.origin[:] = (-20.0, -20.0, 0.0); m.map_size[:] = (40.0, 40.0, 5.0); m.resolution = 0.1; m.grid[:] = (400, 400, 50)
    m.clamp_min_log, m.clamp_max_log, m.min_occupancy_log = 0.12, 0.97, 0.80
    m.local_radius[:] = (6.0, 6.0, 3.0)
    m.log_odds = 0x1000; m.occ = 0x2000   # never dereferenced on the host; nothing is launched in these tests
    return m


P = ctypes.c_void_p
SURROUND = dict(map=True, body=(0.27, 0.0425), ratio=1.2, Q=8, pos=0x9000, planner=None, local_box=None, free_out=0xa000, ws=0x3000, short=0)
PATHS = dict(map=True, body=(0.27, 0.0425), ratio=1.2, B=4, K=16, stride=5, kino_path=0x9000, kino_size=0xa000, have_traj=None, local_box=None,
             first_hit=0xb000, ws=0x3000, short=0)
GOALS = dict(map=True, body=(0.27, 0.0425), check=1.2, search=1.5, B=4, end_pt=0x9000, have_target=None, local_box=None, n_groups=65, group_size=4,
             table=0xa000, goal_blocked=0xb000, goal_hits=0xc000, ws=0x3000, short=0)


def _call(which, **kw):
    lib = solver.lib()
    m = _desc()
    need = lib.frp_nmpc_occmap_workspace_bytes(ctypes.byref(m))
    a = dict({"surround": SURROUND, "paths": PATHS, "goals": GOALS}[which]); a.update(kw)
    pm = ctypes.byref(m) if a["map"] else None
    bd = solver.OccMapBody(*a["body"]) if a["body"] is not None else None
    pb = ctypes.byref(bd) if bd is not None else None
    tail = (P(a["ws"]) if a["ws"] else None, need - a["short"], None)
    if which == "surround":
        return lib.frp_nmpc_occmap_check_surround(pm, pb, a["ratio"], a["Q"], a["pos"], a["planner"], a["local_box"], a["free_out"], *tail)
    if which == "paths":
        return lib.frp_nmpc_occmap_check_paths(pm, pb, a["ratio"], a["B"], a["K"], a["stride"], a["kino_path"], a["kino_size"], a["have_traj"],
                                               a["local_box"], a["first_hit"], *tail)
    return lib.frp_nmpc_occmap_check_goals(pm, pb, a["check"], a["search"], a["B"], a["end_pt"], a["have_target"], a["local_box"], a["n_groups"],
                                           a["group_size"], a["table"], a["goal_blocked"], a["goal_hits"], *tail)


BAD = [("surround", dict(map=False)), ("surround", dict(body=None)), ("surround", dict(ws=0)), ("surround", dict(short=1)),
       ("surround", dict(ratio=12.0)),                                            # ceil(0.27 * 12 / 0.1) = 33
       ("surround", dict(body=(3.2, 0.0425), ratio=1.0)),                        # ceil(32.0) = 32
       ("surround", dict(body=(0.27, 3.11), ratio=1.0)),                         # the z extent alone: ceil(31.1) = 32
       ("surround", dict(ratio=float("nan"))), ("surround", dict(ratio=-1.2)), ("surround", dict(body=(float("inf"), 0.0425))),
       ("surround", dict(Q=-1)), ("surround", dict(pos=None)), ("surround", dict(free_out=None)),
       ("surround", dict(planner=0xd000)),                                        # planner rows without a local_box
       ("paths", dict(map=False)), ("paths", dict(body=None)), ("paths", dict(short=1)), ("paths", dict(ratio=12.0)),
       ("paths", dict(B=-1)), ("paths", dict(K=0)), ("paths", dict(K=-3)), ("paths", dict(stride=0)), ("paths", dict(stride=-5)),
       ("paths", dict(kino_path=None)), ("paths", dict(kino_size=None)), ("paths", dict(first_hit=None)),
       ("goals", dict(map=False)), ("goals", dict(body=None)), ("goals", dict(short=1)), ("goals", dict(check=12.0)), ("goals", dict(search=12.0)),
       ("goals", dict(B=-1)), ("goals", dict(group_size=0)), ("goals", dict(group_size=-4)), ("goals", dict(n_groups=-1)), ("goals", dict(table=None)),
       ("goals", dict(end_pt=None)), ("goals", dict(goal_blocked=None)), ("goals", dict(goal_hits=None))]


@pytest.mark.parametrize("which,kw", BAD, ids=[f"{w}-{'-'.join(k)}-{i}" for i, (w, k) in enumerate(BAD)])
def test_argument_errors_come_before_any_launch(which, kw):
    assert _call(which, **kw) == FRP_ERR_ARG


def test_half_extent_31_is_accepted_and_32_refused():
    assert math.ceil(3.1 * 1.0 / 0.1) == 31 and math.ceil(3.2 * 1.0 / 0.1) == 32
    ok = FRP_ERR_NO_DEVICE if not _has_gpu() else None
    if ok is not None:   # (with a device the accepted call would be launched on made-up pointers)
        assert _call("surround", body=(3.1, 3.1), ratio=1.0) == ok
    assert _call("surround", body=(3.2, 3.1), ratio=1.0) == FRP_ERR_ARG
    assert _call("surround", body=(3.1, 3.2), ratio=1.0) == FRP_ERR_ARG


@pytest.mark.skipif(_has_gpu(), reason="checks the behaviour of a machine WITHOUT a device")
def test_every_call_reports_no_device():
    for which in ("surround", "paths", "goals"):
        assert _call(which) == FRP_ERR_NO_DEVICE, which
    assert _call("surround", Q=0, pos=None, free_out=None) == FRP_ERR_NO_DEVICE
    assert _call("surround", planner=0xd000, local_box=0xe000) == FRP_ERR_NO_DEVICE
    assert _call("paths", have_traj=0xd000, local_box=0xe000) == FRP_ERR_NO_DEVICE
    assert _call("goals", n_groups=0, table=None) == FRP_ERR_NO_DEVICE
    assert _call("goals", have_target=0xd000, local_box=0xe000) == FRP_ERR_NO_DEVICE
