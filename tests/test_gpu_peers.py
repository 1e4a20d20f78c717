"""GPU tests of the fleet peers (include/frp_nmpc.h section 18, csrc/frp_peers.hip, solver.FleetPeers) against tests/peers_oracle.py, the
brute force over all pairs: every flight of tests/peers_cases.py at B = 1, 2, 5, 70 and 260 with S = 1 and 5, every array bit for bit
after each call; the same flight under four grids; one S = 5 call against five S = 1 calls; a fleet against its halves; the peer cloud on
the 40 x 40 x 20 map; no peer, nothing changed; everything captured into one graph; and an 8-planner closed loop with two vehicles on
crossing routes.  Everything is exact: there is no transcendental on this path."""
import numpy as np
import pytest

from forces_resilient_planner_amd import layout as L, solver, workloads

from . import peers_cases as PC
from . import peers_oracle as PO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIELDS = PO.FIELDS + ("outside", "tick")


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)


def _peers(B, S, grid="unit", **kw):
    g = PC.GRIDS[grid]
    return solver.FleetPeers(B, g["origin"], g["dims"], g["cell"], PC.R, PC.D_WARN, PC.D_HIT, S=S, device=DEV, **kw)


def _play(frames, B, S, grid="unit", stride=9, split=False):
    """A flight on the device, call by call; every call's arrays.  split: every call of S samples as S calls of one."""
    import torch
    fp = _peers(B, S, grid)
    pos = torch.zeros((B, S, stride), dtype=torch.float64, device=DEV)
    out = []
    for p, active in frames:
        full = np.full((B, S, stride), 7.5)
        full[:, :, :3] = p
        act = None if active is None else _dev(active, np.uint8)
        if split:
            for s in range(S):
                one = _dev(full[:, s:s + 1], np.float64)
                fp.build(one, act)
                fp.separation(advance=1 if s == S - 1 else 0)
        else:
            pos.copy_(_dev(full, np.float64))
            fp.update(pos, act)
        out.append(fp.arrays())
    return out, fp


def _want(frames, B, grid="unit"):
    out = []
    for rec, outside, tick in PC.replay(frames, PC.GRIDS[grid], B):
        out.append(dict(rec, outside=outside, tick=np.array([tick], dtype=np.int64)))
    return out


@pytest.mark.parametrize("S", (1, 5))
@pytest.mark.parametrize("B", PC.SIZES)
@pytest.mark.parametrize("name", PC.CASES)
def test_a_every_flight_is_the_oracle_to_the_bit_after_every_call(name, B, S):
    frames = PC.flight(name, B, S)
    got, fp = _play(frames, B, S)
    want = _want(frames, B)
    for n, (have, w) in enumerate(zip(got, want)):
        for f in FIELDS:
            assert _same(have[f], w[f]), (name, B, S, n, f, have[f][:8], w[f][:8])
    if B >= 70:                                     # (the cases do what they are for: peers within d_warn, and within d_hit in the crowded ones)
        assert want[-1]["near_samples"].sum() > 0 and (name == "clusters" or want[-1]["hit_samples"].sum() > 0)
    out_i, out_f = (a.cpu().numpy() for a in fp.summary())
    wi, wf = PO.summary(want[-1])
    assert _same(out_i, wi) and _same(out_f, wf), (out_i, wi, out_f, wf)
    mask = (np.arange(B) % 3 != 0).astype(np.int32)
    out_i, out_f = (a.cpu().numpy() for a in fp.summary(_dev(mask, np.int32)))
    wi, wf = PO.summary(want[-1], mask)
    assert _same(out_i, wi) and _same(out_f, wf), (out_i, wi, out_f, wf)
    fp.reset(_dev(mask, np.int32))
    rec = {f: want[-1][f].copy() for f in PO.FIELDS}
    PO.reset(rec, PC.R, mask)
    have = fp.arrays()
    for f in PO.FIELDS:
        assert _same(have[f], rec[f]), f


@pytest.mark.parametrize("name", PC.CASES)
def test_b_the_grid_is_invisible_and_one_call_of_five_samples_is_five_calls_of_one(name):
    B, S = 260, 5
    frames = PC.flight(name, B, S)
    base, _ = _play(frames, B, S)
    for grid, stride in (("coarse", 3), ("shifted", 9), ("wide", 4)):
        other, _ = _play(frames, B, S, grid, stride)
        for a, b in zip(base, other):
            for f in FIELDS:
                assert _same(a[f], b[f]), (name, grid, f)
    one, _ = _play(frames, B, S, split=True)
    for a, b in zip(base, one):
        for f in PO.FIELDS + ("tick",):
            assert _same(a[f], b[f]), (name, f)


def test_c_a_fleet_is_its_halves_where_the_halves_do_not_interact():
    B, S = 140, 5
    a, b = PC.flight("dense", 70, S, seed=1), PC.flight("dense", 70, S, seed=2)
    shift = np.array([5.0, 4.0, 1.0])                                          # the second cluster: more than R from the first
    whole = [(np.concatenate([p, q + shift]), None) for (p, _), (q, _) in zip(a, b)]
    assert all(np.sqrt(PO.dist2(np.concatenate([p[:70, s], p[70:, s]]))[:70, 70:].min()) > PC.R for p, _ in whole for s in range(S))
    got, _ = _play(whole, B, S)
    lo, _ = _play([(p[:70], None) for p, _ in whole], 70, S)
    hi, _ = _play([(p[70:], None) for p, _ in whole], 70, S)
    for n in range(len(whole)):
        for f in PO.FIELDS:
            h = hi[n][f] + 70 * (hi[n][f] >= 0) if f == "nearest" else hi[n][f]
            assert _same(got[n][f], np.concatenate([lo[n][f], h])), (n, f)


# ---- the peer cloud ----
P_CLOUD = 700


class StubFleet:
    def __init__(self, scene):
        self.N, self.pre_plan, self.have_traj = PC.N_PLAN, _dev(scene["pre_plan"], np.float64), _dev(scene["have_traj"], np.int32)


@pytest.fixture(scope="module")
def occmap():
    dm = solver.OccupancyMap(origin=PC.MAP_ORIGIN, map_size=PC.MAP_SIZE, resolution=PC.MAP_RES, device=DEV)
    dm.insert_cloud(PC.MAP_POINTS.astype(np.float32))
    assert tuple(dm.grid) == (40, 40, 20)
    return dm


def _cloud_case(dm, name, B, P=P_CLOUD, edit=None, fp=None):
    """A scene through local_view + FleetPeers.cloud and through the oracle; edit(local_box, cloud_count) changes the view first."""
    scene = PC.cloud_scene(name, B)
    g = PC.CLOUD_GRID
    fp = fp or solver.FleetPeers(B, g["origin"], g["dims"], g["cell"], PC.CLOUD_R, 0.25, 0.125, S=1, r_body=scene["r_body"], stages=scene["stages"], device=DEV)
    state = _dev(scene["state"], np.float64)
    centres = np.nan_to_num(scene["state"][:, :3], nan=0.0)
    view = dm.local_view(_dev(centres, np.float64), P)
    lb, cc, cl = view.local_box.cpu().numpy().copy(), view.cloud_count.cpu().numpy().copy(), view.cloud.cpu().numpy().copy()
    if edit is not None:
        edit(scene, lb, cc)
        view.local_box.copy_(_dev(lb, np.int32)); view.cloud_count.copy_(_dev(cc, np.int32))
    ent = PO.entered(scene["state"][:, None, :3], g["origin"], g["dims"], g["cell"])[:, 0]
    before = cl.copy()
    added, overflow = PO.cloud(scene["state"], ent, scene["pre_plan"], scene["have_traj"], scene["stages"], scene["r_body"], PC.CLOUD_R, lb, PC.MAP_ORIGIN,
                               PC.MAP_RES, cl, cc)
    fp.cloud(StubFleet(scene), state, view, dm)
    got = dict(cloud=view.cloud.cpu().numpy(), cloud_count=view.cloud_count.cpu().numpy(), added=fp.added.cpu().numpy(), overflow=fp.overflow.cpu().numpy(),
               outside=fp.cloud_outside.cpu().numpy())
    want = dict(cloud=cl, cloud_count=cc, added=added, overflow=overflow, outside=(~ent).astype(np.int32))
    return scene, before, got, want


def _narrow(scene, lb, cc):
    """Boxes that end inside the peers of every seventh planner (each face in turn) and a negative count for planner 2."""
    B = len(cc)
    c = np.floor((np.nan_to_num(scene["state"][:, :3]) - np.array(PC.MAP_ORIGIN)) / PC.MAP_RES).astype(np.int32)
    for b in range(0, B, 7):
        k = (b // 7) % 3
        lb[b, k if (b // 21) % 2 == 0 else 3 + k] = c[b, k] + ((b // 21) % 2)
    if B > 2:
        cc[2] = -11


# (B = 1100 in one crowd: more than FRP_PEERS_MAX_CAND candidates of planner 0, the list's reduction in place)
@pytest.mark.parametrize("name,B", [(n, B) for n in PC.CLOUD_CASES for B in PC.SIZES] + [("crowd", 1100)])
def test_d_the_peer_cloud_is_the_oracle_to_the_bit(occmap, name, B):
    for edit in (None, _narrow):
        scene, before, got, want = _cloud_case(occmap, name, B, edit=edit)
        for f in want:
            assert _same(got[f], want[f]), (name, B, f, got[f][:4], want[f][:4])
        if B >= 5:
            assert want["added"].sum() > 0
        if name == "crowd" and B >= 70:
            assert want["overflow"][0] == 1


@pytest.mark.parametrize("name", PC.CLOUD_CASES)
def test_d2_exact_fill_and_one_row_too_few(occmap, name):
    """P chosen so that planner 0's peers fill its rows exactly, and one row less: nothing stored, the count negated.  The other planners'
    counts follow the smaller P through local_view and the oracle alike.  Checked at the sizes at which planner 0 has peers and room."""
    ran = 0
    for B in (5, 70):
        scene, before, got, want = _cloud_case(occmap, name, B, edit=_narrow)
        n, filled = int(want["added"][0]), int(want["cloud_count"][0])
        if n == 0 or filled <= 0:
            continue
        for P in (filled, filled - 1):
            scene, before, got, want2 = _cloud_case(occmap, name, B, P=P, edit=_narrow)
            assert want2["cloud_count"][0] == (filled if P == filled else -filled) and want2["added"][0] == n
            for f in want2:
                assert _same(got[f], want2[f]), (name, B, P, f)
        ran += 1
    assert ran >= 1, name


def test_e_no_peer_within_r_changes_nothing(occmap):
    scene, before, got, want = _cloud_case(occmap, "alone", 70)
    assert want["added"].sum() == 0 and _same(got["cloud"], before) and _same(got["cloud"], want["cloud"]) and _same(got["cloud_count"], want["cloud_count"])
    assert got["added"].sum() == 0 and got["overflow"].sum() == 0


def test_f_build_separation_and_cloud_in_one_graph_replayed_with_moved_positions(occmap):
    import torch
    B, S = 70, 5
    scene = PC.cloud_scene("k3", B)
    g = PC.CLOUD_GRID
    mk = lambda: solver.FleetPeers(B, g["origin"], g["dims"], g["cell"], PC.CLOUD_R, 0.25, 0.125, S=S, r_body=scene["r_body"], stages=scene["stages"], device=DEV)
    eager, cap = mk(), mk()
    fleet = StubFleet(scene)
    rng = np.random.default_rng(9)
    trace, state = torch.zeros((B, S, 9), dtype=torch.float64, device=DEV), torch.zeros((B, 9), dtype=torch.float64, device=DEV)
    views = [occmap.local_view(_dev(scene["state"][:, :3], np.float64), P_CLOUD) for _ in range(3)]
    base = views[2]

    def launch(fp, view, stream=None):
        view.cloud.copy_(base.cloud); view.cloud_count.copy_(base.cloud_count)
        fp.cloud(fleet, state, view, occmap, stream=stream)
        fp.update(trace, stream=stream)
        fp.summary(stream=stream)

    gr = None
    for k in range(6):
        p = scene["state"][:, None, :] + 0.05 * (k + 1) * (rng.random((B, S, 9)) - 0.5)
        trace.copy_(_dev(p, np.float64)); state.copy_(_dev(p[:, S - 1], np.float64))
        launch(eager, views[0])
        if k == 0:
            launch(cap, views[1])
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            gr = torch.cuda.CUDAGraph()
            cap.reset(); cap.tick.zero_()
            torch.cuda.synchronize()
            with torch.cuda.graph(gr, stream=side):
                with torch.cuda.stream(torch.cuda.current_stream()):
                    launch(cap, views[1], torch.cuda.current_stream())
            torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        a, b = eager.arrays(), cap.arrays()
        for f in a:
            assert _same(a[f], b[f]), (k, f)
        for f in ("added", "overflow", "out_i", "out_f"):
            assert _same(getattr(eager, f).cpu().numpy(), getattr(cap, f).cpu().numpy()), (k, f)
        assert _same(views[0].cloud.cpu().numpy(), views[1].cloud.cpu().numpy()) and _same(views[0].cloud_count.cpu().numpy(), views[1].cloud_count.cpu().numpy())
    assert eager.added.sum().item() > 0 and int(eager.tick.item()) == 6


# ---- the closed loop ----
FB = 8
PERIODS = 40
LANES = np.array([-8.05, -6.55, -5.05, -3.55, -2.05, 2.05, 3.55, 5.05])
WEIGHTS = (15.0, 3.0, 80.0, 15.0, 0.0)
LOOP_GRID = dict(origin=(-12.0, -12.0, -1.0), dims=(24, 24, 5), cell=1.0)
P_LOOP = 4096


def _flight(mode, crossing):
    """PERIODS periods of Mission.clock -> Mission.step -> [local_view -> FleetPeers.cloud] -> FleetFSM.period -> FleetPeers.update.
    mode: "eager", "graph" (everything after period 0 is one captured graph), "cloud" (eager, with the bracketed launches and the
    per-planner view as the corridor's cloud) or "view" (the same view without FleetPeers.cloud).  Returns the arrays at the end and, for
    the eager modes, the oracle's record over the traces read back."""
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
    if crossing:                                                # vehicles 0 and 1 swap lanes: their straight lines cross halfway
        route[0, 0, 1], route[1, 0, 1] = LANES[1], LANES[0]
    veh.reset(_dev(start, np.float64))
    veh.odometry(fsm)
    m = solver.Mission(fsm, route=route, arrive_radius=0.3, dwell=0.1, leg_timeout=30.0)
    fp = solver.FleetPeers(veh, LOOP_GRID["origin"], LOOP_GRID["dims"], LOOP_GRID["cell"], PC.R, PC.D_WARN, PC.D_HIT, S=5, r_body=0.2, stages=(2, 5, 9))
    clock = m.clock_out[:3]
    view = dm.local_view(veh.state[:, :3].contiguous(), P_LOOP) if mode in ("cloud", "view") else None
    centres = torch.zeros((FB, 3), dtype=torch.float64, device=DEV)

    def period(stream=None):
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            m.clock(0.0, 1, stream=stream)
            m.step(veh.state, clock, None, stream=stream)
            if view is not None:
                centres.copy_(veh.state[:, :3])
                dm.local_view(centres, P_LOOP, out=view, stream=stream)
                if mode == "cloud":
                    fp.cloud(fleet, veh.state, view, dm, stream=stream)
                fsm.period(pl, dm, None, clock, view.cloud, goal=m.goal, goal_fresh=m.fresh, fsm_steps=1, vehicle=veh, stream=stream, cloud_count=view.cloud_count)
            else:
                fsm.period(pl, dm, None, clock, cloud, goal=m.goal, goal_fresh=m.fresh, fsm_steps=1, vehicle=veh, stream=stream)
            fp.update(stream=stream)

    rec, tick, g = PO.new_record(FB, PC.R), 0, None
    added = 0
    for k in range(PERIODS + 1 if mode == "graph" else PERIODS):    # (one pass of the graph flight is the capture, which launches nothing)
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
            if mode != "graph":
                tr = veh.trace.cpu().numpy()
                ent = PO.entered(tr, LOOP_GRID["origin"], LOOP_GRID["dims"], LOOP_GRID["cell"])
                tick = PO.separation(rec, tr, ent, PC.R, PC.D_WARN, PC.D_HIT, tick)
                added += int(fp.added.sum().item())
    torch.cuda.synchronize()
    out = {"fsm." + n: a for n, a in fsm.arrays().items()}
    out.update({"peers." + n: a for n, a in fp.arrays().items()})
    out.update({"vehicle.x": veh.x.cpu().numpy(), "z": fleet.solver.z.cpu().numpy(), "poly_A": fleet.poly_A.cpu().numpy(), "poly_b": fleet.poly_b.cpu().numpy()})
    return out, rec, tick, added


def test_g_a_crossing_flight_captured_is_the_eager_one_and_its_record_is_the_oracles():
    eager, rec, tick, _ = _flight("eager", True)
    for f in PO.FIELDS:
        assert _same(eager["peers." + f], rec[f]), (f, eager["peers." + f], rec[f])
    assert int(eager["peers.tick"][0]) == tick == PERIODS and eager["peers.samples"].tolist() == [5 * PERIODS] * FB
    print("crossing flight without the peer cloud: sep2_min", eager["peers.sep2_min"].tolist(), "nearest", eager["peers.nearest"].tolist(),
          "hit_samples", eager["peers.hit_samples"].tolist())
    assert set(eager["peers.nearest"][:2].tolist()) <= {-1, 0, 1} and (eager["peers.nearest"][2:] == -1).all()      # lanes 2 ... 7 stay 1.5 m apart
    replay = _flight("graph", True)[0]
    assert set(eager) == set(replay)
    for n in sorted(eager):
        assert _same(eager[n], replay[n]), (n, eager[n], replay[n])


def test_i_without_a_peer_within_r_the_peer_cloud_changes_no_polytope_and_no_plan():
    with_cloud, _, _, added = _flight("cloud", False)
    without, _, _, _ = _flight("view", False)
    assert added == 0
    for n in sorted(with_cloud):
        assert _same(with_cloud[n], without[n]), n
    assert (with_cloud["peers.nearest"] == -1).all()
