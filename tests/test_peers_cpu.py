"""CPU tests of the fleet peers (include/frp_nmpc.h section 18): the NumPy statement tests/peers_oracle.py on hand-worked scenarios with the
expected arrays written out, every named branch counted over the cases, the grid-free result's independence of the box and of the order
of the vehicles, the argument rules through the library (FRP_ERR_ARG comes before the device is looked for), and the header's placement."""
import collections
import ctypes
import os

import numpy as np
import pytest

from forces_resilient_planner_amd import build, capi, solver

from . import peers_cases as PC
from . import peers_oracle as PO

GRID = PC.GRIDS["unit"]
UP = lambda v: float(np.nextafter(np.float64(v), np.inf))


def _run(frames, grid=GRID, R=PC.R, d_warn=PC.D_WARN, d_hit=PC.D_HIT, active=None, count=None):
    """frames: a list of [B,S,3] arrays; the record after the last one, the entered masks, the counter."""
    B = np.asarray(frames[0]).shape[0]
    rec, tick, ents = PO.new_record(B, R), 0, []
    for pos in frames:
        ent = PO.entered(np.asarray(pos, dtype=np.float64), grid["origin"], grid["dims"], grid["cell"], active, count)
        tick = PO.separation(rec, np.asarray(pos, dtype=np.float64), ent, R, d_warn, d_hit, tick, 1, count)
        ents.append(ent)
    return rec, ents, tick


def _pair(dx):
    return [np.array([[[0.0, 0.0, 1.0]], [[dx, 0.0, 1.0]]])]


def test_a_two_vehicles_at_each_radius_and_one_ulp_beyond():
    # R = 1, d_warn = 0.5, d_hit = 0.25: the squares 1, 0.25, 0.0625 are exact
    want = {  # dx: (sep2_min, nearest, near, hit, first_hit)
        0.25: (0.0625, 1, 1, 1, 0), UP(0.25): (UP(0.25) * UP(0.25), 1, 1, 0, -1),
        0.5: (0.25, 1, 1, 0, -1), UP(0.5): (UP(0.5) * UP(0.5), 1, 0, 0, -1),
        1.0: (1.0, -1, 0, 0, -1),          # within R (a peer), but not strictly below the initial R * R: nobody is `nearest`
        UP(1.0): (1.0, -1, 0, 0, -1)}      # no peer at all
    for dx, (m, who, near, hit, first) in want.items():
        assert dx * dx > {UP(0.25): 0.0625, UP(0.5): 0.25, UP(1.0): 1.0}.get(dx, -1.0)
        count = collections.Counter()
        rec, _, tick = _run(_pair(dx), count=count)
        assert tick == 1 and count["peer" if dx <= 1.0 else "no_peer"] == 2
        other = 0 if who == 1 else -1
        assert rec["sep2_min"].tolist() == [m, m] and rec["nearest"].tolist() == [who, other]
        assert rec["near_samples"].tolist() == [near] * 2 and rec["hit_samples"].tolist() == [hit] * 2 and rec["samples"].tolist() == [1, 1]
        assert rec["first_hit"].tolist() == [first] * 2


def test_b_coincident_vehicles_a_tie_and_a_strict_replacement():
    p = [1.0, 1.0, 1.0]
    rec, _, _ = _run([np.array([[p], [p], [p]])])
    assert rec["sep2_min"].tolist() == [0.0, 0.0, 0.0] and rec["nearest"].tolist() == [1, 0, 0] and rec["hit_samples"].tolist() == [1, 1, 1]
    # vehicle 1 between 0 and 2, 0.5 from each: a tie in d2, the lowest id is nearest
    count = collections.Counter()
    rec, _, _ = _run([np.array([[[0.5, 0.0, 1.0]], [[1.0, 0.0, 1.0]], [[1.5, 0.0, 1.0]]])], count=count)
    assert rec["nearest"].tolist() == [1, 0, 1] and rec["sep2_min"].tolist() == [0.25, 0.25, 0.25] and count["tie_lowest_id"] == 1
    # across samples: 0.75 apart, then 0.75 again with another peer (kept: not strictly smaller), then 0.5 (replaced)
    far = [5.0, 5.0, 4.0]
    s0 = [[0.0, 0.0, 1.0], [0.75, 0.0, 1.0], far]
    s1 = [[0.0, 0.0, 1.0], far, [0.0, 0.75, 1.0]]
    s2 = [[0.0, 0.0, 1.0], far, [0.0, 0.5, 1.0]]
    count = collections.Counter()
    one = np.array([s0, s1]).transpose(1, 0, 2)
    rec, _, _ = _run([one], count=count)
    assert rec["nearest"][0] == 1 and rec["sep2_min"][0] == 0.5625 and count["equal_not_replaced"] == 1
    rec, _, tick = _run([one, np.array([s2]).transpose(1, 0, 2)], count=count)
    assert rec["nearest"].tolist() == [2, 0, 0] and rec["sep2_min"].tolist() == [0.25, 0.5625, 0.25] and rec["near_samples"].tolist() == [1, 0, 1]
    assert rec["samples"].tolist() == [3, 3, 3] and tick == 2


def test_c_nan_inactive_outside_and_the_first_hit_counter():
    a, b = [0.0, 0.0, 1.0], [0.125, 0.0, 1.0]
    pos = np.array([[a, a], [b, [np.nan, 0.0, 1.0]], [[50.0, 0.0, 1.0], b], [b, b]])         # [4, 2, 3]
    active = np.array([1, 1, 1, 0], dtype=np.uint8)
    count = collections.Counter()
    first = np.zeros_like(pos)
    first[..., 0], first[..., 2] = 3.0 * np.arange(4)[:, None], 1.0          # call 0: 3 m apart, nobody near anybody
    rec, ents, tick = _run([first, pos, pos], active=active, count=count)
    assert ents[1].tolist() == [[True, True], [True, False], [False, True], [False, False]]
    assert count["nonfinite"] == 2 and count["outside_box"] == 2 and count["inactive"] == 6
    # call 0: nobody near anybody (tick 0); calls 1 and 2: 0 hits 1 in sample 0 and 2 in sample 1
    assert rec["samples"].tolist() == [6, 4, 4, 0] and rec["hit_samples"].tolist() == [4, 2, 2, 0] and rec["first_hit"].tolist() == [1, 1, 1, -1]
    assert rec["nearest"].tolist() == [1, 0, 0, -1] and rec["sep2_min"].tolist() == [0.015625, 0.015625, 0.015625, 1.0] and tick == 3
    assert count["first_hit_set"] == 3 and count["first_hit_kept"] == 5


def test_d_pairs_across_a_cell_face_a_corner_and_neighbouring_cells_more_than_r_apart():
    face = np.array([[[0.9375, 0.5, 1.5]], [[1.0625, 0.5, 1.5]]])                 # cells (9, 6, 1) and (10, 6, 1)
    corner = np.array([[[0.96875, 0.96875, 0.96875]], [[1.03125, 1.03125, 1.03125]]])  # cells (9, 6, 0) and (10, 7, 1)
    apart = np.array([[[0.25, 0.5, 1.5]], [[1.75, 0.5, 1.5]]])                    # neighbouring cells, 1.5 apart
    for pos, want in ((face, 0.015625), (corner, 3 * 0.0625 * 0.0625), (apart, None)):
        f = np.floor((pos[:, 0] - np.array(GRID["origin"])) / GRID["cell"])
        assert np.abs(f[0] - f[1]).max() == 1.0
        rec, _, _ = _run([pos])
        assert rec["sep2_min"].tolist() == ([want] * 2 if want is not None else [1.0, 1.0])
        assert rec["nearest"].tolist() == ([1, 0] if want is not None else [-1, -1])


def test_e_every_branch_of_the_separation_is_taken_by_the_cases():
    count = collections.Counter()
    for name in PC.CASES:
        for B in (5, 70):
            PC.replay(PC.flight(name, B, 5), GRID, B, count)
    test_a_two_vehicles_at_each_radius_and_one_ulp_beyond()
    for pos in ([np.array([[[0.5, 0.0, 1.0]], [[1.0, 0.0, 1.0]], [[1.5, 0.0, 1.0]]])],):
        _run(pos, count=count)
    missing = [n for n in PO.BRANCHES_SEPARATION if count[n] == 0]
    assert not missing, missing


def test_f_the_result_does_not_depend_on_the_grid_or_on_the_order_of_the_vehicles():
    for name in PC.CASES:
        B = 70
        frames = PC.flight(name, B, 5)
        base = PC.replay(frames, GRID, B)
        for g in ("coarse", "shifted", "wide"):
            other = PC.replay(frames, PC.GRIDS[g], B)
            for (r0, o0, t0), (r1, o1, t1) in zip(base, other):
                assert t0 == t1 and np.array_equal(o0, o1)
                for f in PO.FIELDS:
                    assert np.array_equal(r0[f].view(np.uint64) if f == "sep2_min" else r0[f], r1[f].view(np.uint64) if f == "sep2_min" else r1[f]), (name, g, f)
        perm = np.random.default_rng(5).permutation(B)                      # vehicle perm[i] flies as i
        shuffled = PC.replay([(pos[perm], None if act is None else act[perm]) for pos, act in frames], GRID, B)
        for (r0, o0, _), (r1, o1, _) in zip(base, shuffled):
            assert np.array_equal(o0[perm], o1)
            for f in ("sep2_min", "near_samples", "hit_samples", "samples", "first_hit"):
                assert np.array_equal(r0[f][perm], r1[f]), (name, f)
            # nearest with the ids mapped back: the same peer wherever no other peer ties with it (the tie goes to the lowest id, which a permutation moves)
            back = np.where(r1["nearest"] >= 0, perm[np.maximum(r1["nearest"], 0)], -1)
            differ = np.nonzero(back != r0["nearest"][perm])[0]
            assert len(differ) < B // 2
            for i in differ:
                assert name != "clusters", "only coincident vehicles tie"


def _cloud_inputs(scene, P=64, box=None, cc=None):
    B = scene["state"].shape[0]
    ent = PO.entered(scene["state"][:, None, :3], PC.CLOUD_GRID["origin"], PC.CLOUD_GRID["dims"], PC.CLOUD_GRID["cell"])[:, 0]
    lb = np.tile(np.array([0, 0, 0, 40, 40, 20], dtype=np.int32), (B, 1)) if box is None else box
    cloud = np.full((B, P, 3), -7.0)
    count = np.zeros((B,), dtype=np.int32) if cc is None else cc
    return ent, lb, cloud, count


def _cloud(scene, ent, lb, cloud, cc, count=None):
    return PO.cloud(scene["state"], ent, scene["pre_plan"], scene["have_traj"], scene["stages"], scene["r_body"], PC.CLOUD_R, lb, PC.MAP_ORIGIN, PC.MAP_RES,
                    cloud, cc, count)


def test_g_the_cloud_by_hand():
    # three planners in a row 0.25 apart; 1 has a plan, 0 and 2 have none; stages (0, 2); r_body = 0.125
    state = np.zeros((3, 9)); state[:, :3] = [[0.0, 0.0, 1.0], [0.25, 0.0, 1.0], [0.5, 0.0, 1.0]]
    plan = np.zeros((3, 4, 17)); plan[1, :, 8:11] = [[0.25, 0.0, 1.0], [9.0, 9.0, 9.0], [0.25, 0.5, 1.0], [9.0, 9.0, 9.0]]
    scene = dict(state=state, pre_plan=plan, have_traj=np.array([0, 1, 0], dtype=np.int32), stages=(0, 2), r_body=0.125)
    ent, lb, cloud, cc = _cloud_inputs(scene, P=64)
    cc[:] = [2, 0, -5]
    added, overflow = _cloud(scene, ent, lb, cloud, cc)
    seven = lambda c: [c, [c[0] + 0.125, c[1], c[2]], [c[0] - 0.125, c[1], c[2]], [c[0], c[1] + 0.125, c[2]], [c[0], c[1] - 0.125, c[2]],
                       [c[0], c[1], c[2] + 0.125], [c[0], c[1], c[2] - 0.125]]
    # planner 0: peers 1 (0.25, with a plan: three centres) and 2 (0.5, exactly R, no plan), after its two map points
    want0 = seven([0.25, 0.0, 1.0]) + seven([0.25, 0.0, 1.0]) + seven([0.25, 0.5, 1.0]) + seven([0.5, 0.0, 1.0])
    assert added.tolist() == [28, 14, 0] and overflow.tolist() == [0, 0, 0] and cc.tolist() == [30, 14, -5]
    assert cloud[0, 2:30].tolist() == want0 and (cloud[0, :2] == -7.0).all() and (cloud[0, 30:] == -7.0).all() and (cloud[2] == -7.0).all()
    assert cloud[1, :14].tolist() == seven([0.0, 0.0, 1.0]) + seven([0.5, 0.0, 1.0])      # a tie in d2: the lower id first


def test_h_the_cut_on_each_face_exact_fill_one_too_many_and_65_and_70_peers():
    count = collections.Counter()
    for name in PC.CLOUD_CASES + ("alone",):
        for B in (1, 5, 66, 71):
            scene = PC.cloud_scene(name, B)
            ent, lb, cloud, cc = _cloud_inputs(scene, P=700)
            added, overflow = _cloud(scene, ent, lb, cloud.copy(), cc.copy(), count)
            if name == "crowd" and B in (66, 71):           # 65 and 70 peers within R of planner 0; r_body = 0, one stage: 1 or 2 points a peer
                d2 = PO.dist2(scene["state"][:, :3])[0]
                kept = sorted(range(1, B), key=lambda q: (d2[q], q))[:64]
                assert (d2[1:] <= PC.CLOUD_R ** 2).all() and overflow[0] == 1 and added[0] == sum(1 + int(scene["have_traj"][q] != 0) for q in kept)
            if name == "alone":
                assert added.sum() == 0 and overflow.sum() == 0
            if B < 5 or name == "alone":
                continue
            # a box that ends in the middle of planner 0's peers, on each face in turn
            c0 = np.floor((scene["state"][0, :3] - np.array(PC.MAP_ORIGIN)) / PC.MAP_RES).astype(np.int32)
            for k in range(3):
                for side in (0, 1):
                    box = lb.copy()
                    box[0, k if side == 0 else 3 + k] = c0[k] + (0 if side == 0 else 1)
                    a2, _ = _cloud(scene, ent, box, cloud.copy(), cc.copy(), count)
                    assert a2[0] <= added[0]
            # exact fill, one too many, an already negative count
            n = int(added[0])
            if n:
                for P, want in ((n + 3, n + 3), (n + 2, -(n + 3))):
                    cl, c2 = np.full((B, P, 3), -7.0), np.zeros((B,), dtype=np.int32)
                    c2[0] = 3
                    if B > 1:
                        c2[1] = -9
                    _cloud(scene, ent, lb, cl, c2, count)
                    assert c2[0] == want and (want > 0 or (cl[0] == -7.0).all()) and (B == 1 or c2[1] == -9)
    missing = [n for n in PO.BRANCHES_CLOUD if count[n] == 0]
    assert not missing, missing


def test_i_the_kept_64_are_the_smallest_keys_whatever_the_order():
    scene = PC.cloud_scene("crowd", 71)
    ent, lb, cloud, cc = _cloud_inputs(scene, P=200)
    _cloud(scene, ent, lb, cloud, cc)
    d2 = PO.dist2(scene["state"][:, :3])[0]
    order = sorted(range(1, 71), key=lambda q: (d2[q], q))[:64]
    got = cloud[0, :cc[0]].tolist()
    want = []
    for q in order:
        want.append(scene["state"][q, :3].tolist())
        if scene["have_traj"][q]:
            want.append(scene["pre_plan"][q, 1, 8:11].tolist())
    assert got == want
    perm = np.random.default_rng(3).permutation(70) + 1                 # the same crowd with the peers renumbered: the same 64 positions
    sc2 = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in scene.items()}
    for k in ("state", "pre_plan", "have_traj"):
        sc2[k][1:] = scene[k][perm]
    ent2, lb2, cloud2, cc2 = _cloud_inputs(sc2, P=200)
    _cloud(sc2, ent2, lb2, cloud2, cc2)
    assert cc2[0] == cc[0] and sorted(cloud2[0, :cc2[0]].tolist()) == sorted(got)


# ---- the argument rules, through the library ----

def good():
    """(struct, view, keep): a frp_nmpc_peers and a frp_nmpc_peers_view no call refuses, on host scratch (never launched on: every call
    below is refused for its arguments, or answers FRP_ERR_NO_DEVICE on a machine without a device)."""
    k = (ctypes.c_double * 4096)()
    a = ctypes.addressof(k)
    p = capi.PeersArgs(4, 2, (ctypes.c_double * 3)(-9.0, -6.0, 0.0), (ctypes.c_int * 3)(18, 12, 5), 1.0, 1.0, 0.5, 0.25, *([a] * 14))
    v = capi.PeersViewArgs(20, 2, 64, 0.2, (ctypes.c_double * 3)(-2.0, -2.0, 0.0), 0.1, *([a] * 8))
    return p, v, k


def refusals():
    out, keep = [], []
    nan, inf = float("nan"), float("inf")

    def bad(what, call, **edit):
        p, v, k = good()
        for n, val in edit.items():
            tgt, name = (v, n[2:]) if n.startswith("v_") else (p, n)
            if isinstance(val, tuple):
                for i, x in enumerate(val):
                    getattr(tgt, name)[i] = x
            else:
                setattr(tgt, name, val)
        keep.extend([p, v, k])
        out.append((what, lambda l, p=p, v=v, k=k: call(l, ctypes.byref(p), ctypes.byref(v), ctypes.addressof(k))))

    build_ = lambda l, p, v, a: l.frp_nmpc_peers_build(p, a, 9, None, None)
    sep = lambda l, p, v, a: l.frp_nmpc_peers_separation(p, a, 9, 1, None)
    rst = lambda l, p, v, a: l.frp_nmpc_peers_reset(p, None, None)
    summ = lambda l, p, v, a: l.frp_nmpc_peers_summary(p, None, a, a, None)
    cld = lambda l, p, v, a: l.frp_nmpc_peers_cloud(p, v, a, 9, None)
    for nm, call in (("build", build_), ("separation", sep), ("cloud", cld)):
        one = dict(S=1) if nm == "cloud" else {}
        for what, edit in (("cell 0", dict(cell=0.0)), ("cell nan", dict(cell=nan)), ("cell inf", dict(cell=inf)), ("cell < 0", dict(cell=-1.0)),
                           ("R 0", dict(R=0.0, d_warn=0.0, d_hit=0.0)), ("R nan", dict(R=nan)), ("R inf", dict(R=inf, cell=inf)), ("R > cell", dict(R=1.5, cell=1.0)),
                           ("S 0", dict(S=0)), ("B < 0", dict(B=-1)), ("dim 0", dict(dims=(18, 0, 5))), ("origin nan", dict(origin=(0.0, nan, 0.0))),
                           ("too many cells", dict(dims=(2048, 2048, 2))), ("cells times S", dict(dims=(2048, 1024, 1), S=3)),
                           ("start NULL", dict(start=None)), ("items NULL", dict(items=None)), ("key NULL", dict(key=None)), ("slot NULL", dict(slot=None)),
                           ("block_sums NULL", dict(block_sums=None)), ("outside NULL", dict(outside=None))):
            if nm == "cloud" and what in ("S 0", "cells times S"):
                continue
            bad(f"{nm}: {what}", call, **{**one, **edit})
    out.append(("build: pos NULL", lambda l: l.frp_nmpc_peers_build(ctypes.byref(good()[0]), None, 9, None, None)))
    for stride in (2, 0, -1, 1 << 30):
        p, v, k = good(); keep.extend([p, k])
        out.append((f"build: stride {stride}", lambda l, p=p, k=k, s=stride: l.frp_nmpc_peers_build(ctypes.byref(p), ctypes.addressof(k), s, None, None)))
        out.append((f"separation: stride {stride}", lambda l, p=p, k=k, s=stride: l.frp_nmpc_peers_separation(ctypes.byref(p), ctypes.addressof(k), s, 1, None)))
    for nm, call in (("separation", sep), ("reset", rst), ("summary", summ)):
        for what, edit in (("d_hit > d_warn", dict(d_hit=0.75)), ("d_warn > R", dict(d_warn=1.25)), ("d_warn nan", dict(d_warn=nan)), ("d_hit nan", dict(d_hit=nan)),
                           ("d_hit < 0", dict(d_hit=-0.1)), ("R nan", dict(R=nan)), ("sep2_min NULL", dict(sep2_min=None)), ("nearest NULL", dict(nearest=None)),
                           ("near_samples NULL", dict(near_samples=None)), ("hit_samples NULL", dict(hit_samples=None)), ("samples NULL", dict(samples=None)),
                           ("first_hit NULL", dict(first_hit=None)), ("tick NULL", dict(tick=None)), ("sum_ws NULL", dict(sum_ws=None)), ("B < 0", dict(B=-2))):
            bad(f"{nm}: {what}", call, **edit)
    p, v, k = good(); keep.extend([p, k])
    out.append(("separation: advance < 0", lambda l, p=p, k=k: l.frp_nmpc_peers_separation(ctypes.byref(p), ctypes.addressof(k), 9, -1, None)))
    out.append(("summary: out_i NULL", lambda l, p=p, k=k: l.frp_nmpc_peers_summary(ctypes.byref(p), None, None, ctypes.addressof(k), None)))
    out.append(("summary: out_f NULL", lambda l, p=p, k=k: l.frp_nmpc_peers_summary(ctypes.byref(p), None, ctypes.addressof(k), None, None)))
    out.append(("reset: p NULL", lambda l: l.frp_nmpc_peers_reset(None, None, None)))
    out.append(("build: p NULL", lambda l, k=k: l.frp_nmpc_peers_build(None, ctypes.addressof(k), 9, None, None)))
    for what, edit in (("S 2", dict(S=2)), ("N 0", dict(S=1, v_N=0)), ("K < 0", dict(S=1, v_K=-1)), ("K 9", dict(S=1, v_K=9)), ("P < 0", dict(S=1, v_P=-1)),
                       ("r_body < 0", dict(S=1, v_r_body=-0.1)), ("r_body nan", dict(S=1, v_r_body=nan)), ("r_body inf", dict(S=1, v_r_body=inf)),
                       ("resolution 0", dict(S=1, v_resolution=0.0)), ("resolution nan", dict(S=1, v_resolution=nan)), ("map origin inf", dict(S=1, v_origin=(0.0, 0.0, inf))),
                       ("pre_plan NULL", dict(S=1, v_pre_plan=None)), ("have_traj NULL", dict(S=1, v_have_traj=None)), ("stages NULL with K", dict(S=1, v_stages=None)),
                       ("local_box NULL", dict(S=1, v_local_box=None)), ("cloud NULL with P", dict(S=1, v_cloud=None)), ("cloud_count NULL", dict(S=1, v_cloud_count=None)),
                       ("added NULL", dict(S=1, v_added=None)), ("overflow NULL", dict(S=1, v_overflow=None)), ("plans beyond int", dict(S=1, B=1 << 24, v_N=20))):
        bad(f"cloud: {what}", cld, **edit)
    p, v, k = good(); p.S = 1; keep.extend([p, v, k])
    out.append(("cloud: v NULL", lambda l, p=p, k=k: l.frp_nmpc_peers_cloud(ctypes.byref(p), None, ctypes.addressof(k), 9, None)))
    return out, keep


def test_j_the_c_abi_refuses_every_bad_argument_before_it_looks_for_a_device():
    l = solver.lib()
    table, keep = refusals()
    assert len(table) > 120
    for what, call in table:
        assert call(l) == capi.FRP_ERR_ARG, what
    if l.frp_nmpc_device_count() == 0:
        p, v, k = good()
        a = ctypes.addressof(k)
        assert l.frp_nmpc_peers_build(ctypes.byref(p), a, 9, None, None) == capi.FRP_ERR_NO_DEVICE
        assert l.frp_nmpc_peers_separation(ctypes.byref(p), a, 9, 0, None) == capi.FRP_ERR_NO_DEVICE
        assert l.frp_nmpc_peers_reset(ctypes.byref(p), None, None) == capi.FRP_ERR_NO_DEVICE
        assert l.frp_nmpc_peers_summary(ctypes.byref(p), None, a, a, None) == capi.FRP_ERR_NO_DEVICE
        p.S = 1
        assert l.frp_nmpc_peers_cloud(ctypes.byref(p), ctypes.byref(v), a, 9, None) == capi.FRP_ERR_NO_DEVICE
        v.K, v.stages, v.P, v.cloud = 0, None, 0, None
        assert l.frp_nmpc_peers_cloud(ctypes.byref(p), ctypes.byref(v), a, 9, None) == capi.FRP_ERR_NO_DEVICE


def test_k_the_python_class_refuses_what_the_library_would():
    for kw in (dict(R=1.5), dict(cell=0.0), dict(d_warn=1.5), dict(d_hit=0.75), dict(dims=(2048, 2048, 2)), dict(S=0), dict(r_body=-1.0), dict(stages=tuple(range(9))),
               dict(stages=(-1,)), dict(vehicle_or_B=0)):
        args = dict(vehicle_or_B=4, origin=(0.0, 0.0, 0.0), dims=(4, 4, 4), cell=1.0, R=1.0, d_warn=0.5, d_hit=0.25)
        args.update(kw)
        with pytest.raises((ValueError, RuntimeError, AssertionError)):
            solver.FleetPeers(device="cpu", **args)


def test_l_the_header_places_section_18_and_the_unit_is_built_like_its_neighbours():
    hdr = open(os.path.join(build.ROOT, "include", "frp_nmpc.h")).read()
    assert "#define FRP_NMPC_ABI_VERSION 7" in hdr and solver.ABI_VERSION == 7
    at = {n: hdr.index(f"---- ({n}) ") for n in (14, 15, 16, 17, 18)}
    assert hdr.rindex('#include "frp_nmpc_') < at[15] < at[18] < at[16] < at[17] < at[14]
    sec = hdr[at[18]:at[16]]
    assert "NO REFERENCE COUNTERPART" in sec and "CHOSEN, not derived" in sec and "typedef struct frp_nmpc_peers {" in sec
    names = ["frp_nmpc_peers_build", "frp_nmpc_peers_separation", "frp_nmpc_peers_reset", "frp_nmpc_peers_summary", "frp_nmpc_peers_cloud"]
    i = solver.EXPORTS.index(names[0])
    assert solver.EXPORTS[i:i + 5] == names and solver.EXPORTS[i - 1] == "frp_nmpc_vehicle_step_field" and solver.EXPORTS[i + 5] == "frp_nmpc_sensor_noise_states"
    assert all(hasattr(solver.lib(), n) for n in names)
    assert capi.C_TYPES[capi.PeersArgs] == ("frp_nmpc_peers", "frp_nmpc.h") and capi.C_TYPES[capi.PeersViewArgs] == ("frp_nmpc_peers_view", "frp_nmpc.h")
    assert solver.FleetPeers.__module__.endswith(".flight") and capi.PEERS_MAX_NEAR == PO.MAX_NEAR
    assert (capi.PEERS_I_NEAREST, capi.PEERS_I_WITH_HITS, capi.PEERS_I_NEAR, capi.PEERS_I_HIT, capi.PEERS_I_SAMPLES) == (PO.I_NEAREST, PO.I_WITH_HITS, PO.I_NEAR, PO.I_HIT, PO.I_SAMPLES)
    assert "frp_peers.hip" in build.SOURCES and build.PER_SOURCE_FLAGS["frp_peers.hip"] == ["-ffp-contract=off"]
    src = "\n".join(ln for ln in open(os.path.join(build.CSRC, "frp_peers.hip")).read().splitlines() if not ln.lstrip().startswith("//"))
    assert '#include "frp_fleet.hpp"' in src
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "FleetPeers" in open(os.path.join(build.ROOT, doc)).read() or "frp_nmpc_peers_build" in open(os.path.join(build.ROOT, doc)).read(), doc
