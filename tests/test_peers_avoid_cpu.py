"""CPU tests of peer avoidance (include/frp_nmpc.h section 19): the box oracle (tests/peers_avoid_oracle.py) on hand-worked cases with the
expected arrays written out, every named branch counted, independence of the neighbour grid, the argument rules through the library
(FRP_ERR_ARG comes before the device is looked for), a scenario proved on the oracles alone -- a parked peer midway on a straight line in
the empty world -- and, from tests/astar_path_cases.py's conditions, that the overlay cases of the GPU tests take the window, the
fallback, the byte-map and the local-box routes."""
import collections
import ctypes

import numpy as np

from forces_resilient_planner_amd import build, capi, solver, workloads

from . import astar_lib as AL
from . import astar_path_cases as AC
from . import peers_avoid_cases as AV
from . import peers_avoid_oracle as AO
from . import peers_oracle as PO

# the hand-worked map: 8 x 8 x 4 voxels of 0.5 m at the origin (inv = 2.0 exactly); everybody is everybody's peer
ORIGIN, RES, GRID, R = (0.0, 0.0, 0.0), 0.5, (8, 8, 4), 10.0
N = 4
COUNT = collections.Counter()


def _run(pos, half=(0.5, 0.5, 0.5), stages=(), plans=None, have=None, Q=8, ent=None):
    pos = np.asarray(pos, dtype=np.float64)
    B = len(pos)
    pre = np.zeros((B, N, 17)) if plans is None else plans
    have = np.zeros(B, dtype=np.int32) if have is None else np.asarray(have, dtype=np.int32)
    ent = np.ones(B, dtype=bool) if ent is None else ent
    return AO.boxes(pos, ent, pre, have, stages, half, R, ORIGIN, RES, GRID, Q, COUNT)


def _rows(out, b):
    return out[0][b, :max(int(out[1][b]), 0)].tolist()


def test_a_a_centre_on_a_voxel_face_and_one_ulp_to_either_side():
    me = (0.25, 0.25, 0.25)
    for x, want in ((2.0, [3, 3, 1, 5, 5, 3]), (np.nextafter(2.0, 0.0), [2, 3, 1, 5, 5, 3]), (np.nextafter(2.0, 3.0), [3, 3, 1, 5, 5, 3])):
        # (one ulp below: c - half = 1.5 - 2^-52 is exact and falls in voxel 2; c + half = 2.5 - 2^-52 is a tie and rounds to 2.5, voxel 5)
        out = _run([me, (x, 2.0, 1.0)])
        assert _rows(out, 0) == [want] and out[1].tolist() == [1, 1] and out[3].tolist() == [0, 0]
        assert _rows(out, 1) == [[0, 0, 0, 1, 1, 1]]                 # the peer at 0.25: lo = floor(-0.5) = -1, clipped
    # the upper bound on a face: c + half = 2.5 - ulp stays in voxel 4, 2.5 is voxel 5
    assert AO.voxel_f(np.nextafter(2.5, 0.0), 0.0, 2.0) == 4.0 and AO.voxel_f(2.5, 0.0, 2.0) == 5.0


def test_b_half_zero_is_the_centres_voxel():
    out = _run([(0.25, 0.25, 0.25), (2.0, 2.0, 1.0)], half=(0.0, 0.0, 0.0))
    assert _rows(out, 0) == [[4, 4, 2, 4, 4, 2]] and _rows(out, 1) == [[0, 0, 0, 0, 0, 0]]


def test_c_a_box_clipped_at_each_face_wholly_outside_and_a_nan_centre():
    me = (2.1, 2.1, 1.1)                                              # voxel (4, 4, 2)
    out = _run([me, (0.1, 1.0, 1.0), (3.9, 1.0, 1.0), (1.0, 0.1, 1.0), (1.0, 3.9, 1.0), (1.0, 1.0, 0.1), (1.0, 1.0, 1.9)])
    # planner 0's peers ascending in (d2, id)
    rows = {tuple(r) for r in _rows(out, 0)}
    assert rows == {(0, 1, 1, 1, 3, 3), (6, 1, 1, 7, 3, 3), (1, 0, 1, 3, 1, 3), (1, 6, 1, 3, 7, 3), (1, 1, 0, 3, 3, 1), (1, 1, 2, 3, 3, 3)} and out[1][0] == 6
    out = _run([me, (-3.0, 2.0, 1.0), (2.0, 6.0, 1.0), (2.0, 2.0, 4.0)], half=(0.25, 0.25, 0.25))   # beyond x = 0, y = 4, z = 2: hi < 0 or lo > grid - 1
    assert out[1][0] == 0 and _rows(out, 0) == []
    plans = np.zeros((2, N, 17)); plans[1, :, 8:11] = (1.0, 1.0, 1.0); plans[1, 1, 9] = np.nan; plans[1, 2, 8] = np.inf
    out = _run([me, (1.0, 1.0, 1.0)], stages=(0, 1, 2, 7), plans=plans, have=[0, 1])
    assert _rows(out, 0) == [[1, 1, 1, 3, 3, 3], [1, 1, 1, 3, 3, 3]]   # the position and stage 0; NaN, inf and the stage outside the plan give none
    assert _rows(out, 1) == [[3, 3, 1, 5, 5, 3]] and out[3].tolist() == [0, 0]     # planner 0 has no plan: its position alone


def test_d_the_own_voxel_drop():
    out = _run([(1.9, 1.9, 0.9), (2.0, 2.0, 1.0)])                   # voxel (3, 3, 1) lies in [3 .. 5, 3 .. 5, 1 .. 3]
    assert out[1].tolist() == [0, 0] and out[3].tolist() == [1, 1]   # ... and (4, 4, 2) in the other's [2 .. 4, 2 .. 4, 0 .. 2]
    out = _run([(0.25, 0.25, 0.25), (2.0, 2.0, 1.0)])
    assert out[3].tolist() == [0, 0]
    # a later stage over the spot the planner stands on is dropped, the peer's position is kept
    plans = np.zeros((2, N, 17)); plans[1, :, 8:11] = (0.3, 0.3, 0.3)
    out = _run([(0.25, 0.25, 0.25), (2.0, 2.0, 1.0)], stages=(1,), plans=plans, have=[0, 1])
    assert _rows(out, 0) == [[3, 3, 1, 5, 5, 3]] and out[3][0] == 1


def test_e_k_0_and_8_exact_fill_one_too_many_and_65_peers():
    pos = [(0.25, 0.25, 0.25), (2.0, 2.0, 1.0)]
    plans = np.zeros((2, N, 17))
    for k in range(N):
        plans[1, k, 8:11] = (2.0 + 0.5 * k, 2.0, 1.0)
    out0 = _run(pos, stages=(), plans=plans, have=[0, 1])
    out8 = _run(pos, stages=(0, 1, 2, 3, 0, 1, 2, 3), plans=plans, have=[0, 1], Q=9)
    assert out0[1][0] == 1 and out8[1][0] == 9 and _rows(out8, 0)[1:5] == [[3, 3, 1, 5, 5, 3], [4, 3, 1, 6, 5, 3], [5, 3, 1, 7, 5, 3], [6, 3, 1, 7, 5, 3]]
    assert _rows(out8, 0)[0] == _rows(out0, 0)[0] and _rows(out8, 0)[5:] == _rows(out8, 0)[1:5]        # peer rank first, then centre
    short = _run(pos, stages=(0, 1, 2, 3, 0, 1, 2, 3), plans=plans, have=[0, 1], Q=8)
    assert short[1][0] == -9 and not short[0][0].any() and short[1][1] == 1
    # 66 vehicles in a row: planner 0 has 65 peers, the nearest 64 are kept
    pos = [(0.05 + 0.05 * i, 2.0, 1.0) for i in range(66)]
    out = _run(pos, half=(0.0, 0.0, 0.0), Q=64)
    assert out[2][0] == 1 and out[1][0] + out[3][0] == 64
    assert out[2][33] == 1 and out[2].sum() == 66


def test_f_every_named_branch_was_taken():
    out = _run([(0.25, 0.25, 0.25), (2.0, 2.0, 1.0), (np.nan, 0.0, 0.0)], ent=np.array([True, True, False]))
    assert out[1][2] == 0
    _run([(0.25, 0.25, 0.25)])
    _run([(0.25, 0.25, 0.25), (2.0, 2.0, 1.0)], Q=1)
    missing = [n for n in AO.BRANCHES if COUNT[n] == 0]
    assert not missing, missing


def test_g_the_neighbour_grid_is_invisible():
    rng = np.random.default_rng(3)
    B = 40
    pos = np.zeros((B, 9)); pos[:, :3] = rng.random((B, 3)) * (3.5, 3.5, 1.8) + 0.1
    plans = rng.random((B, N, 17)) * 3.0
    have = (rng.random(B) < 0.5).astype(np.int32)
    outs = []
    for g in (dict(origin=(-1.0, -1.0, -1.0), dims=(6, 6, 4), cell=1.0), dict(origin=(-3.0, -2.0, -5.0), dims=(4, 3, 3), cell=3.0), dict(origin=(0.0, 0.0, 0.0), dims=(8, 8, 4), cell=0.55)):
        ent = PO.entered(pos[:, None, :3], g["origin"], g["dims"], g["cell"])[:, 0]
        assert ent.all()
        outs.append(AO.boxes(pos, ent, plans, have, (0, 2), (0.2, 0.2, 0.3), 0.5, ORIGIN, RES, GRID, 64))
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], o))
    assert outs[0][1].sum() > 0


# ---- the argument rules through the library ----
def _good():
    k = (ctypes.c_double * 64)()
    a = ctypes.addressof(k)
    p = capi.PeersArgs(4, 1, (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_int * 3)(4, 4, 4), 1.0, 1.0, 0.5, 0.25, *([a] * 14))
    v = capi.PeersBoxArgs(4, 1, 2, (ctypes.c_double * 3)(0.2, 0.2, 0.2), (ctypes.c_double * 3)(0, 0, 0), 0.5, (ctypes.c_int * 3)(8, 8, 4), *([a] * 7))
    return p, v, k, a


def test_h_the_c_abi_refuses_every_bad_argument_before_it_looks_for_a_device():
    l = solver.lib()
    nan, inf = float("nan"), float("inf")
    n = 0
    for what, edit in (("N 0", dict(N=0)), ("K < 0", dict(K=-1)), ("K 9", dict(K=9)), ("Q < 0", dict(Q=-1)), ("half < 0", dict(half=(0.1, -0.1, 0.1))), ("half nan", dict(half=(nan, 0.1, 0.1))),
                       ("half inf", dict(half=(0.1, 0.1, inf))), ("resolution 0", dict(resolution=0.0)), ("resolution nan", dict(resolution=nan)), ("origin inf", dict(origin=(0.0, inf, 0.0))),
                       ("grid 0", dict(grid=(8, 0, 4))), ("pre_plan NULL", dict(pre_plan=None)), ("have_traj NULL", dict(have_traj=None)), ("stages NULL with K", dict(stages=None)),
                       ("boxes NULL with Q", dict(boxes=None)), ("count NULL", dict(count=None)), ("overflow NULL", dict(overflow=None)), ("dropped_own NULL", dict(dropped_own=None)),
                       ("rows beyond int", dict(Q=1 << 28))):
        p, v, k, a = _good()
        for f, val in edit.items():
            setattr(v, f, type(getattr(v, f))(*val) if isinstance(val, tuple) else val)
        assert l.frp_nmpc_peers_boxes(ctypes.byref(p), ctypes.byref(v), a, 9, None) == capi.FRP_ERR_ARG, what
        n += 1
        if what in ("Q < 0", "resolution 0", "resolution nan", "origin inf", "grid 0", "boxes NULL with Q", "count NULL", "rows beyond int"):
            assert l.frp_nmpc_peers_check_paths(ctypes.byref(v), 4, 16, 5, a, a, None, a, None) == capi.FRP_ERR_ARG, what
            n += 1
    p, v, k, a = _good()
    for what, call in (("v NULL", lambda: l.frp_nmpc_peers_boxes(ctypes.byref(p), None, a, 9, None)), ("p NULL", lambda: l.frp_nmpc_peers_boxes(None, ctypes.byref(v), a, 9, None)),
                       ("pos NULL", lambda: l.frp_nmpc_peers_boxes(ctypes.byref(p), ctypes.byref(v), None, 9, None)), ("stride 2", lambda: l.frp_nmpc_peers_boxes(ctypes.byref(p), ctypes.byref(v), a, 2, None)),
                       ("walk: v NULL", lambda: l.frp_nmpc_peers_check_paths(None, 4, 16, 5, a, a, None, a, None)), ("walk: B < 0", lambda: l.frp_nmpc_peers_check_paths(ctypes.byref(v), -1, 16, 5, a, a, None, a, None)),
                       ("walk: K 0", lambda: l.frp_nmpc_peers_check_paths(ctypes.byref(v), 4, 0, 5, a, a, None, a, None)), ("walk: stride 0", lambda: l.frp_nmpc_peers_check_paths(ctypes.byref(v), 4, 16, 0, a, a, None, a, None)),
                       ("walk: path NULL", lambda: l.frp_nmpc_peers_check_paths(ctypes.byref(v), 4, 16, 5, None, a, None, a, None)), ("walk: size NULL", lambda: l.frp_nmpc_peers_check_paths(ctypes.byref(v), 4, 16, 5, a, None, None, a, None)),
                       ("walk: first_hit NULL", lambda: l.frp_nmpc_peers_check_paths(ctypes.byref(v), 4, 16, 5, a, a, None, None, None)),
                       ("walk: samples beyond int", lambda: l.frp_nmpc_peers_check_paths(ctypes.byref(v), 1 << 20, 1 << 12, 5, a, a, None, a, None))):
        assert call() == capi.FRP_ERR_ARG, what
        n += 1
    p.S = 2
    assert l.frp_nmpc_peers_boxes(ctypes.byref(p), ctypes.byref(v), a, 9, None) == capi.FRP_ERR_ARG
    p.S, p.R = 1, 2.0
    assert l.frp_nmpc_peers_boxes(ctypes.byref(p), ctypes.byref(v), a, 9, None) == capi.FRP_ERR_ARG
    # the search: Q < 0, one pointer without the other, rows without Q, Q without rows, and whatever the plain entry refuses
    st = capi.Astar()
    for Q, bx, cnt in ((-1, a, a), (2, a, None), (2, None, a), (2, None, None), (0, a, a), (1 << 28, a, a)):
        assert l.frp_nmpc_astar_batch_peers(ctypes.byref(st), bx, cnt, Q, a, 1 << 20, None) == capi.FRP_ERR_ARG, Q
    assert l.frp_nmpc_astar_batch_peers(ctypes.byref(st), a, a, 2, a, 1 << 20, None) == capi.FRP_ERR_ARG        # an empty frp_nmpc_astar
    assert l.frp_nmpc_astar_batch_peers(None, a, a, 2, a, 1 << 20, None) == capi.FRP_ERR_ARG
    assert l.frp_nmpc_astar_batch_peers(ctypes.byref(st), None, None, 0, a, 1 << 20, None) == l.frp_nmpc_astar_batch(ctypes.byref(st), a, 1 << 20, None) == capi.FRP_ERR_ARG
    assert n > 35
    if l.frp_nmpc_device_count() == 0:
        p, v, k, a = _good()
        assert l.frp_nmpc_peers_boxes(ctypes.byref(p), ctypes.byref(v), a, 9, None) == capi.FRP_ERR_NO_DEVICE
        assert l.frp_nmpc_peers_check_paths(ctypes.byref(v), 4, 16, 5, a, a, None, a, None) == capi.FRP_ERR_NO_DEVICE
        v.K, v.stages, v.Q, v.boxes = 0, None, 0, None
        assert l.frp_nmpc_peers_boxes(ctypes.byref(p), ctypes.byref(v), a, 9, None) == capi.FRP_ERR_NO_DEVICE


def test_i_placement_build_and_documents():
    hdr = open(build.ROOT + "/include/frp_nmpc.h").read()
    assert "#define FRP_NMPC_ABI_VERSION 7" in hdr and hdr.index("---- (19) ") < hdr.index("---- (15) ")
    names = ["frp_nmpc_peers_boxes", "frp_nmpc_astar_batch_peers", "frp_nmpc_peers_check_paths"]
    i = solver.EXPORTS.index(names[0])
    assert solver.EXPORTS[i:i + 3] == names and solver.EXPORTS[i + 3] == "frp_nmpc_disturbance_eval" and all(hasattr(solver.lib(), n) for n in names)
    assert capi.C_TYPES[capi.PeersBoxArgs] == ("frp_nmpc_peers_box_view", "frp_nmpc.h")
    for unit in ("frp_peers_boxes.hip", "frp_astar_peers.hip"):
        assert unit in build.SOURCES and build.PER_SOURCE_FLAGS[unit] == ["-ffp-contract=off"]
    assert build.PER_SOURCE_FLAGS["frp_astar_peers.hip"] == build.PER_SOURCE_FLAGS["frp_astar.hip"]
    assert "IDENTICAL" in open(build.ROOT + "/profiles/peers_avoid_astar_identity.txt").read()
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "frp_nmpc_astar_batch_peers" in open(build.ROOT + "/" + doc).read(), doc


# ---- a scenario on the oracles alone: a parked peer midway on a straight line in the empty world ----
def test_j_a_parked_peer_on_the_line_is_routed_around_and_the_walk_tells_the_two_paths_apart():
    w = workloads.astar_world(0, "empty", allocate_num=12000)
    a = lambda *rows: np.asarray(rows, dtype=float)
    q = dict(start_pt=a((-6.0, 0.05, 1.05)), start_v=np.zeros((1, 3)), start_a=np.zeros((1, 3)), end_pt=a((4.0, 0.05, 1.05)), end_v=np.zeros((1, 3)), f_ext=np.zeros((1, 3)))
    peer = np.array([-3.0, 0.05, 1.05])
    state = np.zeros((2, 9)); state[0, :3] = q["start_pt"][0]; state[1, :3] = peer
    grid = w["occ"].shape
    bx, cnt, over, own = AO.boxes(state, np.ones(2, dtype=bool), np.zeros((2, 4, 17)), np.zeros(2, dtype=np.int32), (), (0.3, 0.3, 0.3), 5.0, w["origin"], w["resolution"], grid, 4)
    centre = AV.voxel(w, peer)
    assert cnt.tolist() == [1, 1] and own.tolist() == [0, 0] and bx[0, 0].tolist() == [centre[0] - 3, centre[1] - 3, centre[2] - 3, centre[0] + 3, centre[1] + 3, centre[2] + 3]
    plain = AL.plan_batch(w, q["start_pt"], q["start_v"], q["start_a"], q["end_pt"], q["end_v"], q["f_ext"])
    around = AO.plan_with_boxes(w, q, bx[:1], cnt[:1])
    n0, n1 = int(plain["kino_size"][0]), int(around["kino_size"][0])
    p0, p1 = plain["kino_path"][0, :n0], around["kino_path"][0, :n1]
    vox = lambda p: [tuple(AV.voxel(w, x)) for x in p]
    assert plain["status"][0] != AC.STATUS_NO_PATH and np.all(p0[:, 1] == 0.05) and np.all(p0[:, 2] == 1.05) and tuple(centre) in vox(p0)   # the straight line, through the peer
    assert around["status"][0] != AC.STATUS_NO_PATH and not (n0 == n1 and np.array_equal(p0, p1)) and tuple(centre) not in vox(p1)
    inside = lambda v: all(bx[0, 0, k] <= v[k] <= bx[0, 0, 3 + k] for k in range(3))
    assert not any(inside(v) for v in vox(p1))
    first = next(s for s in range(0, n0, 5) if inside(vox(p0[s:s + 1])[0]))
    walk = collections.Counter()
    K = max(n0, n1)
    paths = np.zeros((2, K, 3)); paths[0, :n0] = p0; paths[1, :n1] = p1
    hit = AO.check_paths(np.stack([bx[0], bx[0]]), np.array([1, 1]), paths, np.array([n0, n1]), np.array([1, 1]), 5, w["origin"], w["resolution"], grid, walk)
    assert hit.tolist() == [first, -1] and walk["sample_hit"] == 1 and walk["clean"] == 1
    # the walk's other branches: no plan held, no boxes, a sample outside the map
    paths[1, 0] = (99.0, 0.0, 1.0)
    hit = AO.check_paths(np.stack([bx[0], bx[0]]), np.array([1, 0]), paths, np.array([n0, n1]), np.array([0, 1]), 5, w["origin"], w["resolution"], grid, walk)
    assert hit.tolist() == [-1, -1]
    hit = AO.check_paths(np.stack([bx[0], bx[0]]), np.array([-3, 1]), paths, np.array([n0, n1]), None, 5, w["origin"], w["resolution"], grid, walk)
    assert hit.tolist() == [-1, -1] and not [n for n in AO.BRANCHES_WALK if walk[n] == 0]


def test_k_the_overlay_cases_take_the_routes_they_are_named_after():
    routes = {name: AV.route_of(AV.overlay_case(name)) for name in AV.OVERLAY}
    for name in ("empty", "pillars", "wall_gap"):
        assert routes[name] == {"window"}, (name, routes[name])
    assert routes["window_edge"] == routes["beyond_window"] == {"window", "fallback"}
    assert routes["local_box"] == {"window", "local_box"} and routes["byte_map"] == {"byte_map"}
    for name in AV.OVERLAY:
        c = AV.overlay_case(name)
        assert AC.fast_flag(c["world"]) and c["count"].tolist() == ([1, 0, 1, 1] if name in ("window_edge", "beyond_window") else [1, 0, 3, 2]), name
    # the boxes of the two window cases against the window of the start node: columns start - WIN_R_MAX ... start + WIN_R_MAX
    for name, straddles in (("window_edge", True), ("beyond_window", False)):
        c = AV.overlay_case(name)
        w = c["world"]
        reach = int(np.floor((w["max_vel"] * w["max_tau"] + 0.5 * w["max_acc"] * w["max_tau"] ** 2) / w["resolution"]))      # of a node at the velocity bound
        assert reach > AC.WIN_R_MAX
        for b in (0, 2, 3):
            x0 = AV.voxel(w, c["q"]["start_pt"][b])[0]
            lo, hi = c["boxes"][b, 0, 0] - x0, c["boxes"][b, 0, 3] - x0
            assert hi > AC.WIN_R_MAX and (lo <= AC.WIN_R_MAX) == straddles and lo <= reach, (name, b, lo, hi, reach)
    c = AV.overlay_case("local_box")                                  # half of every box lies beyond the planner's local box
    for b in (0, 2, 3):
        assert c["boxes"][b, 0, 1] <= c["local_box"][b, 4] < c["boxes"][b, 0, 4]
