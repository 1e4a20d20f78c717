"""GPU tests of peer avoidance (include/frp_nmpc.h section 19: csrc/frp_peers_boxes.hip, csrc/frp_astar_peers.hip, FleetPeers.boxes /
check_paths, AstarPlanner.overlay) against tests/peers_avoid_oracle.py and, for the search, oracle/astar_oracle.c run per planner on the
world with that planner's boxes written into occ.  Everything is exact.  What avoidance does to a crossing is not asserted: the
crossing test prints it."""
import types

import numpy as np
import pytest

from forces_resilient_planner_amd import layout as L, solver, workloads

from . import astar_gpu_lib as AG
from . import astar_lib as AL
from . import peers_avoid_cases as AV
from . import peers_avoid_oracle as AO
from . import peers_cases as PC
from . import peers_oracle as PO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAPS = dict(full=types.SimpleNamespace(origin=PC.MAP_ORIGIN, resolution=PC.MAP_RES, grid=(40, 40, 20)),
            tight=types.SimpleNamespace(origin=(-0.25, -0.15, 0.85), resolution=0.1, grid=(5, 4, 3)))     # most boxes clipped or outside


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


class StubFleet:
    def __init__(self, scene):
        self.N, self.pre_plan, self.have_traj = PC.N_PLAN, _dev(scene["pre_plan"], np.float64), _dev(scene["have_traj"], np.int32)


def _boxes_case(name, B, map_name, half=AV.HALF, Q=None):
    scene = PC.cloud_scene(name, B)
    g, m = PC.CLOUD_GRID, MAPS[map_name]
    fp = solver.FleetPeers(B, g["origin"], g["dims"], g["cell"], PC.CLOUD_R, 0.25, 0.125, S=1, stages=scene["stages"], device=DEV)
    fp.boxes(StubFleet(scene), _dev(scene["state"], np.float64), m, half, Q=Q)
    ent = PO.entered(scene["state"][:, None, :3], g["origin"], g["dims"], g["cell"])[:, 0]
    Qn = int(fp.box_rows.shape[1])
    want = AO.boxes(scene["state"], ent, scene["pre_plan"], scene["have_traj"], scene["stages"], half if hasattr(half, "__len__") else (half,) * 3, PC.CLOUD_R,
                    m.origin, m.resolution, m.grid, Qn)
    got = tuple(a.cpu().numpy() for a in (fp.box_rows, fp.box_count, fp.box_overflow, fp.dropped_own))
    return scene, fp, got, want


def _same_boxes(got, want, tag):
    for f, a, b in zip(("count", "overflow", "dropped_own"), got[1:], want[1:]):
        assert np.array_equal(a, b), (tag, f, a[:8], b[:8])
    for b in range(len(want[1])):
        n = max(int(want[1][b]), 0)
        assert np.array_equal(got[0][b, :n], want[0][b, :n]), (tag, b, got[0][b, :n], want[0][b, :n])


@pytest.mark.parametrize("map_name", sorted(MAPS))
@pytest.mark.parametrize("B", PC.SIZES)
@pytest.mark.parametrize("name", PC.CLOUD_CASES)          # k0: no stage of a plan; k8, k3, crowd: with plans
def test_a_the_boxes_are_the_oracle_to_the_bit(name, B, map_name):
    scene, fp, got, want = _boxes_case(name, B, map_name)
    _same_boxes(got, want, (name, B, map_name))
    if B >= 5 and map_name == "full":                      # (the crowd stands within a box's half edge: there every box holds the planner's own voxel)
        assert want[1].clip(min=0).sum() > 0 or (name == "crowd" and want[3].sum() > 0)
    if name == "crowd" and B >= 70:
        assert want[2][0] == 1
    # rows past a count were never written
    for b in range(B):
        assert not got[0][b, max(int(got[1][b]), 0):].any()


def test_a2_half_zero_exact_fill_and_one_row_too_few():
    scene, fp, got, want = _boxes_case("k3", 70, "full", half=0.0)
    _same_boxes(got, want, "half0")
    assert want[1].sum() > 0
    _, _, _, full = _boxes_case("k8", 70, "full")
    n = int(full[1].max())
    assert n > 1
    for Q in (n, n - 1):
        scene, fp, got, want = _boxes_case("k8", 70, "full", Q=Q)
        _same_boxes(got, want, Q)
        assert (want[1] == (n if Q == n else -n)).any()
        assert not got[0][want[1] < 0].any()                # an overflowing planner stored nothing


# ---- the search on the map plus a planner's boxes ----
def _overlay_planner(w, Bn, bx, cnt, **kw):
    pl = solver.AstarPlanner(w, Bn, K=2048, want_path_nodes=True, **kw)
    pl.overlay = types.SimpleNamespace(box_rows=_dev(bx, np.int32), box_count=_dev(cnt, np.int32))
    return pl


@pytest.mark.parametrize("Bn", (1, 4))
@pytest.mark.parametrize("name", AV.OVERLAY)
def test_b_the_overlay_search_is_the_oracle_on_the_planners_own_world(name, Bn):
    c = AV.overlay_case(name)
    rows = [2] if Bn == 1 else list(range(AV.B))            # (B = 1: the planner with the most boxes)
    q = {k: v[rows] for k, v in c["q"].items()}
    bx, cnt = c["boxes"][rows], c["count"][rows]
    lb = None if c["local_box"] is None else c["local_box"][rows]
    o = AO.plan_with_boxes(c["world"], q, bx, cnt, local_box=lb)
    plain = AL.plan_batch(c["world"], q["start_pt"], q["start_v"], q["start_a"], q["end_pt"], q["end_v"], q["f_ext"], local_box=lb)
    pl = AG.run_gpu(c["world"], q, Bn, planner=_overlay_planner(c["world"], Bn, bx, cnt), local_box=lb)
    AG.compare(pl, o, Bn)
    if Bn == 4:                                             # the boxes are in the way: some planner's search differs from the plain one
        assert any(o["results"][b].use_node_num != plain["results"][b].use_node_num or o["kino_size"][b] != plain["kino_size"][b] for b in range(Bn)), name
        assert cnt[1] == 0 and o["results"][1].use_node_num == plain["results"][1].use_node_num        # ... and a planner without boxes searches the map


def test_c_the_overlay_entry_without_boxes_is_the_plain_entry():
    import torch
    c = AV.overlay_case("pillars")
    ref = AG.run_gpu(c["world"], c["q"], AV.B)
    zero = _overlay_planner(c["world"], AV.B, c["boxes"], np.zeros_like(c["count"]))
    none = solver.AstarPlanner(c["world"], AV.B, K=2048, want_path_nodes=True)
    none.overlay = types.SimpleNamespace(box_rows=torch.zeros((AV.B, 0, 6), dtype=torch.int32, device=DEV), box_count=torch.zeros((AV.B,), dtype=torch.int32, device=DEV))
    neg = _overlay_planner(c["world"], AV.B, c["boxes"], -c["count"] - 1)
    for pl in (zero, none, neg):
        AG.run_gpu(c["world"], c["q"], AV.B, planner=pl)
        for f in ("status", "stats", "kino_size", "kino_path", "path_nodes"):
            a, b = getattr(ref, f).cpu().numpy(), getattr(pl, f).cpu().numpy()
            assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), f


def test_c2_a_count_above_q_reads_q_rows():
    """The arrays are device memory: the call cannot refuse a count above Q, so the search and the walk read Q rows -- count = Q + 1 and a
    far larger one give what count = Q gives, to the bit."""
    c = AV.overlay_case("pillars")
    Q = 2
    bx = np.ascontiguousarray(c["boxes"][:, :Q])
    outs = []
    for cnt in (Q, Q + 1, 1 << 30):
        pl = _overlay_planner(c["world"], AV.B, bx, np.full((AV.B,), cnt, dtype=np.int32))
        AG.run_gpu(c["world"], c["q"], AV.B, planner=pl)
        outs.append({f: getattr(pl, f).cpu().numpy() for f in ("status", "stats", "kino_size", "kino_path", "path_nodes")})
    for o in outs[1:]:
        for f, a in outs[0].items():
            assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, o[f].view(np.uint64) if o[f].dtype == np.float64 else o[f]), f
    o = AO.plan_with_boxes(c["world"], c["q"], bx, np.full((AV.B,), Q, dtype=np.int32))     # ... and that is the oracle on Q boxes
    pl = AG.run_gpu(c["world"], c["q"], AV.B, planner=_overlay_planner(c["world"], AV.B, bx, np.full((AV.B,), Q + 1, dtype=np.int32)))
    AG.compare(pl, o, AV.B)
    # the walk: the same first hits
    scene, fp, got, want = _boxes_case("k8", 70, "full")
    m = MAPS["full"]
    path = np.ascontiguousarray(np.repeat(scene["state"][:, None, :3], 8, axis=1) + 0.05 * np.arange(8)[None, :, None])
    held = types.SimpleNamespace(kino_path=_dev(path, np.float64), kino_size=_dev(np.full(70, 8), np.int32))
    Qn = int(fp.box_rows.shape[1])
    fp.box_count.fill_(Qn + 1)
    hit = fp.check_paths(held, None, stride=1).cpu().numpy()
    w = AO.check_paths(got[0], np.full(70, Qn), path, np.full(70, 8), None, 1, m.origin, m.resolution, m.grid)
    assert np.array_equal(hit, w)


# ---- the path walk ----
@pytest.mark.parametrize("B", (1, 5, 70, 260))
def test_d_the_path_walk_is_the_oracle(B):
    import torch
    scene, fp, got, want = _boxes_case("k8", B, "full")
    m = MAPS["full"]
    rng = np.random.default_rng(B)
    K = 37
    path = scene["state"][:, None, :3] + np.cumsum(0.06 * (rng.random((B, K, 3)) - 0.45), axis=1)
    path[::7, 3] = np.nan
    path[::5, 10] = (9.0, 0.0, 1.0)                                            # a sample outside the map
    size = rng.integers(0, K + 6, B).astype(np.int32)                         # (beyond K as well: min(size, K) samples)
    have = (rng.random(B) < 0.8).astype(np.int32)
    pl = types.SimpleNamespace(kino_path=_dev(path, np.float64), kino_size=_dev(size, np.int32))
    fsm = types.SimpleNamespace(have_traj=_dev(have, np.int32), safety_verdict=lambda *a: None)
    for stride, f, h in ((5, fsm, have), (1, fsm, have), (3, None, None)):
        hit = fp.check_paths(pl, f, stride=stride).cpu().numpy()
        w = AO.check_paths(got[0], got[1], path, size, h, stride, m.origin, m.resolution, m.grid)
        assert np.array_equal(hit, w), (B, stride, hit[:8], w[:8])
    if B >= 70:
        assert (w >= 0).any() and (w < 0).any()


# ---- the closed loop: tests/test_gpu_peers.py's 8-planner flight with avoidance attached ----
FB, PERIODS = 8, 40
LANES = np.array([-8.05, -6.55, -5.05, -3.55, -2.05, 2.05, 3.55, 5.05])
WEIGHTS = (15.0, 3.0, 80.0, 15.0, 0.0)
LOOP_GRID = dict(origin=(-12.0, -12.0, -1.0), dims=(24, 24, 5), cell=1.0)
BOX_HALF = (0.3, 0.3, 0.3)


def _flight(mode, crossing):
    """PERIODS periods of Mission.clock -> Mission.step -> [FleetPeers.boxes -> check_paths + verdict] -> FleetFSM.period (the planner's
    overlay attached) -> FleetPeers.update.  mode: "plain" (nothing bracketed, no overlay), "avoid" (eager) or "graph" (avoidance, everything
    after period 0 one captured graph)."""
    import torch
    w = workloads.astar_world(0, "empty", allocate_num=12000)
    dm = solver.OccupancyMap(w)
    pillar = np.array([(x, y, z) for x in np.arange(-0.25, 0.26, 0.1) for y in np.arange(-0.25, 0.26, 0.1) for z in np.arange(-0.95, 2.96, 0.1)], dtype=np.float32)
    dm.insert_cloud(pillar)
    fleet = solver.DeviceFleet(FB, 20, 30, 64, L.MODEL_NORMAL, WEIGHTS, weights_final=WEIGHTS)
    fleet.poly_index = torch.zeros((FB, 20), dtype=torch.int32, device=DEV)
    fsm = solver.FleetFSM(fleet)
    pl = solver.AstarPlanner(dm, FB, K=512)
    fsm.bind(pl)
    cloud = _dev(pillar.astype(np.float64), np.float64)
    veh = solver.Vehicle(fleet, trace=True)
    start = np.zeros((FB, 9)); start[:, 0] = -6.05; start[:, 1] = LANES; start[:, 2] = 1.2
    route = np.array([[[-3.05, y, 1.2]] for y in LANES])
    if crossing:
        route[0, 0, 1], route[1, 0, 1] = LANES[1], LANES[0]
    veh.reset(_dev(start, np.float64))
    veh.odometry(fsm)
    m = solver.Mission(fsm, route=route, arrive_radius=0.3, dwell=0.1, leg_timeout=30.0)
    fp = solver.FleetPeers(veh, LOOP_GRID["origin"], LOOP_GRID["dims"], LOOP_GRID["cell"], PC.R, PC.D_WARN, PC.D_HIT, S=5, stages=(2, 5, 9))
    clock = m.clock_out[:3]
    avoid = mode != "plain"
    if avoid:
        pl.overlay = fp
    hits = []

    def period(stream=None):
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            m.clock(0.0, 1, stream=stream)
            m.step(veh.state, clock, None, stream=stream)
            if avoid:
                fp.boxes(fleet, veh.state, dm, BOX_HALF, stream=stream)
                fp.check_paths(pl, fsm, stream=stream)
            fsm.period(pl, dm, None, clock, cloud, goal=m.goal, goal_fresh=m.fresh, fsm_steps=1, vehicle=veh, stream=stream)
            fp.update(stream=stream)

    g = None
    for k in range(PERIODS + 1 if mode == "graph" else PERIODS):
        if mode == "graph" and k > 0:
            if g is None:
                torch.cuda.synchronize()
                side = torch.cuda.Stream()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    period(torch.cuda.current_stream())
                torch.cuda.synchronize()
            else:
                g.replay()
        else:
            period()
            if mode == "avoid":
                hits.append((int(fp.box_count.clamp(min=0).sum().item()), int((fp.path_hit >= 0).sum().item())))
    torch.cuda.synchronize()
    out = {"fsm." + n: a for n, a in fsm.arrays().items()}
    out.update({"peers." + n: a for n, a in fp.arrays().items()})
    out.update({"vehicle.x": veh.x.cpu().numpy(), "z": fleet.solver.z.cpu().numpy(), "poly_A": fleet.poly_A.cpu().numpy(), "poly_b": fleet.poly_b.cpu().numpy(),
                "kino_path": pl.kino_path.cpu().numpy(), "kino_size": pl.kino_size.cpu().numpy(), "astar.status": pl.status.cpu().numpy()})
    if avoid:
        out.update({"boxes.count": fp.box_count.cpu().numpy(), "boxes.path_hit": fp.path_hit.cpu().numpy(), "boxes.dropped_own": fp.dropped_own.cpu().numpy()})
    return out, hits


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)


def test_e_a_crossing_flight_with_avoidance_captured_is_the_eager_one():
    eager, hits = _flight("avoid", True)
    print("crossing flight with avoidance: (boxes, paths hit) per period", hits, "sep2_min", eager["peers.sep2_min"].tolist(), "hit_samples",
          eager["peers.hit_samples"].tolist())
    assert sum(h[0] for h in hits) > 0                      # the two crossing vehicles came within R: boxes existed
    replay, _ = _flight("graph", True)
    assert set(eager) == set(replay)
    for n in sorted(eager):
        assert _same(eager[n], replay[n]), (n, eager[n], replay[n])


def test_f_without_a_crossing_the_attachment_changes_no_plan_and_no_state():
    avoid, hits = _flight("avoid", False)
    plain, _ = _flight("plain", False)
    assert sum(h[0] for h in hits) == 0 and sum(h[1] for h in hits) == 0
    for n in sorted(plain):
        assert _same(avoid[n], plain[n]), n
