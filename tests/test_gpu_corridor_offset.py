"""GPU tests of the corridor with an anisotropic seed ellipsoid (frp_nmpc_corridor.offset_x != 0; include/frp_nmpc.h).  With
f = seed_len / 2 and r = f / (f + offset_x) the seed has semi-axes (f, f r, f r) along the heading: prolate for offset_x > 0, an oblate
disc for -f < offset_x < 0.  Every other corridor test runs a sphere.

  * the cases of tests/golden/corridor_mp.npz (tests/corridor_mp_cases.py: sphere, prolate, oblate; the world turned about z by 0, 45
    and 100 degrees; 6000 and 20000 points) through the plain-cloud launch and the grid launches (the workgroup kernels and the
    one-wavefront kernel with its shells): against the 50-digit reference on the decisive planners, against the oracle on all, bit for
    bit across the launches, and the polytope properties on the kernel's output;
  * obstacles inside an anisotropic seed ellipsoid: both shrink loops of find_ellipsoid start from unequal axes;
  * the list and cloud regimes of the workgroup kernel;
  * the cut, view and large routes, with the planners' kernels fixed by in-box and in-SEED-ELLIPSOID counts that are asserted;
  * offset_x = 0 passed explicitly is the default.
offset_x <= -seed_len / 2 is outside the domain and never launched: tests/test_corridor_mp_cpu.py tests the refusal."""
import functools
import sys

import numpy as np
import pytest

from forces_resilient_planner_amd import solver
from tests import corridor_mp_cases as CM
from tests.test_gpu_corridor_cut import _run, _same, ROOT
from tests.test_gpu_corridor_large import (CONSTS, EMPTY, FALLBACK, GRID, GRID_LIST, REG_TILE, STARTS, WAVE, WAVE_TILE, _counts, _main_case,
                                           _run_view)
from tests.test_gpu_parity import _check_corridor, _corridor_world

pytestmark = pytest.mark.gpu
CASES = CM.load()
IDS = [c.name for c in CASES]


def _polys_of(pi, A, b, nf, p):
    return [(A[p, k, :nf[p, k]], b[p, k, :nf[p, k]]) for k in range(int(pi[p].max()) + 1)]


def _seed_counts(vis, ref_p, yaw_p, consts):
    """Per stage: (points of `vis` in the local box of a decomposition seeded there, those inside its seed ELLIPSOID) --
    tests/test_gpu_corridor_large.py::_box_counts with the metric of the anisotropic seed."""
    bb, sl, off = consts["bbox"], consts["seed_len"], consts.get("offset_x", 0.0)
    f = sl / 2; r = f / (f + off)
    out = []
    for p1, y in zip(ref_p, yaw_p):
        h = np.array([np.cos(y), np.sin(y), 0.0]); dh = np.array([h[1], -h[0], 0.0]); dv = np.cross(h, dh)
        e = vis - p1
        a, t, v = e @ dh, e @ h, e @ dv
        inb = (np.abs(a) <= bb[1]) & (t >= -bb[0]) & (t <= sl + bb[0]) & (np.abs(v) <= bb[2])
        w = vis - (p1 + h * f); tw = w @ h
        d2 = tw ** 2 / f ** 2 + ((w ** 2).sum(1) - tw ** 2) / (f * r) ** 2
        out.append((int(inb.sum()), int((inb & (d2 <= 1)).sum())))
    return np.array(out).reshape(-1, 2)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture_case_against_the_mp_reference(case):
    """The plain-cloud launch (workgroup kernels) and the grid launches at 0.5 and 0.23 m cells (the one-wavefront kernel first), each
    against the fixture on the decisive planners -- indices, counts and row order exact, rows within 1e-9 -- and the properties on all."""
    cloud = case.cloud()                                            # (a digest mismatch fails here)
    for cell in (None, 0.5, 0.23):
        pi, A, b, nf, cnt = solver.corridor_batch_host(cloud, case.ref, case.yaw, case.E, consts=case.consts, grid_cell=cell)
        worst = 0.0
        for p in np.nonzero(case.decisive)[0]:
            worst = max(worst, CM.compare_with_fixture(case, p, pi[p], cnt[p], nf[p], lambda k: np.c_[A[p, k, :nf[p, k]], b[p, k, :nf[p, k]]]))
        print(f"{case.name}, grid cell {cell}: largest |kernel row - mp row| = {worst:.3g} on {int(case.decisive.sum())} decisive planners")
        for p in range(CM.B):
            CM.check_properties(case.name, case.consts, cloud, case.ref[p], case.yaw[p], pi[p], _polys_of(pi, A, b, nf, p))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture_case_against_the_oracle_and_across_the_launches(case):
    """All planners against the oracle, and the three launches bit for bit (both asserted by _check_corridor)."""
    _check_corridor(case.cloud(), case.ref, case.yaw, case.E, consts=case.consts)


def test_offset_zero_passed_explicitly_equals_the_default():
    a = CASES[0]
    assert a.name == "a_sphere" and a.consts["offset_x"] == 0.0
    cloud = a.cloud()
    base = {k: v for k, v in a.consts.items() if k != "offset_x"}
    for cell in (None, 0.5, 0.23):
        want = solver.corridor_batch_host(cloud, a.ref, a.yaw, a.E, grid_cell=cell)
        for consts in (base, dict(base, offset_x=0.0), dict(offset_x=0.0), dict(offset_x=-0.0)):
            got = solver.corridor_batch_host(cloud, a.ref, a.yaw, a.E, consts=consts, grid_cell=cell)
            assert all(np.array_equal(x, y) for x, y in zip(got, want)), (cell, consts)


SHRINK = (dict(seed_len=1.5, bbox=(2.0, 2.0, 1.0), inflation=1.1, offset_x=+0.4),      # semi-axes (0.75, 0.49, 0.49)
          dict(seed_len=0.8, bbox=(1.0, 1.5, 0.7), inflation=1.0, offset_x=-0.25))     # semi-axes (0.4, 1.07, 1.07): wider than the box is high


@pytest.mark.parametrize("world,k", [((7, 8000, 3), 0), ((7, 8000, 3), 1), ((23, 40000, 2), 1)],
                         ids=["world7-prolate", "world7-oblate", "world23-oblate"])
def test_obstacles_inside_an_anisotropic_seed_ellipsoid(world, k):
    """Worlds 7 and 23 of tests/test_gpu_parity.py's shrink tests (tunnel = 0.25): every stage's seed ellipsoid holds obstacles, so both
    shrink loops of find_ellipsoid (line_segment.h:156-208) run, from unequal axes.  ordered=False for _check_corridor's stated reason.
    In-seed counts, stage by stage: 6 .. 17 and 25 .. 41 on world 7; 150 .. 211 among 1300 .. 1380 in-box points on world 23 -- beyond
    the one-wavefront kernel's register tile, within its in-seed tile."""
    seed, P, B = world
    cloud, ref, yaw, E = _corridor_world(seed, P=P, B=B, tunnel=0.25)
    consts = SHRINK[k]
    counts = np.stack([_seed_counts(cloud, ref[p], yaw[p], consts) for p in range(B)])
    print("in-box", counts[..., 0].min(), counts[..., 0].max(), "in-seed", counts[..., 1].min(), counts[..., 1].max())
    assert counts[..., 1].min() >= 5                                # every decomposition shrinks
    if P == 40000:
        assert counts[..., 0].min() > REG_TILE and 100 < counts[..., 1].min() and counts[..., 1].max() < WAVE_TILE
    _check_corridor(cloud, ref, yaw, E, consts=consts, ordered=False)


@pytest.mark.parametrize("P,mode", [(9000, "list"), (40000, "cloud")])
def test_list_and_cloud_regimes_with_an_oblate_seed(P, mode):
    """The dense worlds of tests/test_gpu_parity.py::test_corridor_dense_boxes_use_the_list_and_cloud_paths at offset_x = -0.03."""
    rng = np.random.default_rng(P)
    cloud = np.c_[rng.uniform(-1.5, 4.5, P), rng.uniform(-2.2, 2.2, P), rng.uniform(0.0, 2.0, P)]
    N, B = 6, 2
    s = np.linspace(0.5, 2.5, N)
    centre = np.c_[s, 0.2 * np.sin(s), np.full(N, 1.0)]
    cx = np.interp(cloud[:, 0], centre[:, 0], centre[:, 1])
    cloud = cloud[np.hypot(cloud[:, 1] - cx, cloud[:, 2] - 1.0) > 0.45]
    ref = centre[None] + rng.normal(0, 0.02, (B, N, 3))
    yaw = rng.normal(0.1, 0.05, (B, N))
    E = np.tile(np.diag([0.2, 0.2, 0.05]), (B, N, 1, 1))
    consts = dict(solver.CORRIDOR_DEFAULTS, offset_x=-0.03)
    counts = np.stack([_seed_counts(cloud, ref[p], yaw[p], consts) for p in range(B)])
    assert (2048 < counts[:, 0, 0]).all() and (counts[:, 0, 0] <= 8192).all() if mode == "list" else (counts[:, 0, 0] > 8192).all()
    assert counts[..., 1].max() == 0                                # nothing inside the disc: the seed ellipsoid is the final one
    pi, A, b, nf = _check_corridor(cloud, ref, yaw, E, consts=dict(offset_x=-0.03))
    for p in range(B):
        CM.check_properties(mode, consts, cloud, ref[p], yaw[p], pi[p], _polys_of(pi, A, b, nf, p))


OBLATE = dict(CONSTS, offset_x=-0.6)                                # seed_len = 2: r = 2.5, a disc of radius 2.5 m across the heading


@functools.lru_cache(maxsize=None)
def _oblate_case():
    """tests/test_gpu_corridor_large.py's world and planners; ROUTE 1 (per-planner clouds) with the oblate seed; the kernel each planner
    ends in, from counts with the ellipsoid's metric.  Computed once, never modified."""
    dm, om, ref, yaw, E, c, whole, _ = _main_case()
    vis = [om.local_cloud(x) for x in c]
    counts = [_seed_counts(v, ref[p], yaw[p], OBLATE) for p, v in enumerate(vis)]
    print("in-box / in-seed-ellipsoid counts, stage 0 .. last:", [(k[0].tolist(), k[-1].tolist()) for k in counts])
    for p in WAVE:      # the one-wavefront kernel finishes the planner itself
        assert counts[p][:, 0].max() < 200 and 0 < counts[p][:, 1].min() and counts[p][:, 1].max() < WAVE_TILE // 4
    for p in GRID:      # handed on at stage 0, finished by the grid kernel
        assert counts[p][0, 1] > WAVE_TILE + 100 and REG_TILE < counts[p][:, 0].min() and counts[p][:, 0].max() < GRID_LIST - 500
    for p in FALLBACK:  # handed on twice
        assert counts[p][0, 1] > WAVE_TILE + 100 and counts[p][0, 0] > GRID_LIST + 500 and counts[p][:, 0].max() < solver.CORRIDOR_LARGE_LIST
    for p in EMPTY:
        assert len(vis[p]) == 0
    # the disc holds more than the sphere did: the anisotropic in-seed test is what places the planners
    sphere = [_seed_counts(v, ref[p], yaw[p], CONSTS) for p, v in enumerate(vis)]
    assert all(counts[p][0, 1] > sphere[p][0, 1] for p in WAVE + GRID + FALLBACK)
    lv = dm.local_view(c, solver.CORRIDOR_MAX_POINTS)
    want = _run(lv.cloud, ref, yaw, E, count=lv.cloud_count, consts=OBLATE)
    assert (want[4][list(WAVE + GRID + FALLBACK)] >= 1).all() and (want[2][list(EMPTY), 0] == 6).all()
    return dm, om, ref, yaw, E, c, whole, vis, want


def test_view_and_large_routes_with_the_cut_equal_route_1_with_an_oblate_seed():
    dm, om, ref, yaw, E, c, whole, vis, want = _oblate_case()
    assert len(STARTS) == 8
    cut = dm.cut(dm.local_view(c, 0).local_box)
    view = dm.shared_view_device(cap=131072, cell=0.5, planners=8)
    assert view.large
    view.update()
    assert _counts(view) == (len(whole), len(whole))
    _same(want, _run_view(view, ref, yaw, E, cut=cut, consts=OBLATE), "large view with the cut, oblate seed")
    assert np.array_equal(view.overflow.cpu().numpy(), np.zeros(8, dtype=np.int32))
    spherical = _main_case()[-1]
    assert not np.array_equal(spherical[1], want[1])                # (the offset is not ignored)


@pytest.mark.parametrize("group", ["wave", "grid", "fallback"])
def test_route_1_with_an_oblate_seed_against_the_oracle(group):
    """Two planners of each kernel group on om.local_cloud(...).  The wave group's seeds hold 4 .. 10 obstacles, the others 1500 .. 4300:
    every decomposition shrinks, so rows are matched as a set (tests/test_gpu_parity.py::_check_corridor, ordered=False)."""
    dm, om, ref, yaw, E, c, whole, vis, want = _oblate_case()
    sys.path.insert(0, ROOT)
    from oracle import corridor_oracle as C
    A, b, nf, pi, cnt = want
    for p in dict(wave=WAVE, grid=GRID, fallback=FALLBACK)[group][:2]:
        idx, polys = C.corridor_one(ref[p], yaw[p], E[p], vis[p], **OBLATE)
        assert np.array_equal(pi[p], idx), (p, pi[p], idx)
        assert cnt[p] == len(polys)
        for k, (Ao, bo) in enumerate(polys):
            assert nf[p, k] == len(bo), (p, k, nf[p, k], len(bo))
            G = np.c_[A[p, k, :len(bo)], b[p, k, :len(bo)]]; O = np.c_[Ao, bo]
            match = np.abs(G[:, None, :] - O[None, :, :]).max(axis=2).argmin(axis=0)
            assert sorted(match) == list(range(len(bo))), (p, k, match)
            assert np.max(np.abs(G[match] - O)) < 1e-9, (p, k)
        assert np.all(nf[p, len(polys):] == 0)
