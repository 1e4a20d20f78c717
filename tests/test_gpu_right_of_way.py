"""GPU tests of right of way (include/frp_nmpc.h section 20: csrc/frp_peers_yield.hip, FleetPeers.boxes(priority=...), solver.RightOfWay)
against tests/right_of_way_oracle.py.  Everything is exact.  What right of way does to the separation of a crossing pair is not asserted:
the crossing test prints it."""
import collections
import ctypes
import types

import numpy as np
import pytest

from forces_resilient_planner_amd import capi, layout as L, solver, workloads

from . import peers_cases as PC
from . import peers_oracle as PO
from . import right_of_way_oracle as RO
from .test_gpu_peers_avoid import BOX_HALF, DEV, FB, LANES, LOOP_GRID, MAPS, PERIODS, WEIGHTS, StubFleet, _dev, _same
from .peers_avoid_cases import HALF

pytestmark = pytest.mark.gpu

PATTERNS = ("equal", "reversed", "two_classes")


def _priority(pattern, B):
    if pattern == "equal":
        return np.full((B,), 3, dtype=np.int32)
    if pattern == "reversed":
        return np.arange(B, dtype=np.int32)                     # the higher id wins
    return (np.arange(B) % 3 == 0).astype(np.int32) * 7         # every third vehicle is of the upper class


def _ranked_case(name, B, map_name, pattern, Q=None, stages=None):
    scene = PC.cloud_scene(name, B)
    st = scene["stages"] if stages is None else stages
    g, m = PC.CLOUD_GRID, MAPS[map_name]
    pr = _priority(pattern, B)
    fp = solver.FleetPeers(B, g["origin"], g["dims"], g["cell"], PC.CLOUD_R, 0.25, 0.125, S=1, stages=st, device=DEV)
    fleet, state = StubFleet(scene), _dev(scene["state"], np.float64)
    fp.boxes(fleet, state, m, HALF, Q=Q, priority=_dev(pr, np.int32))
    ent = PO.entered(scene["state"][:, None, :3], g["origin"], g["dims"], g["cell"])[:, 0]
    want = RO.boxes_ranked(scene["state"], ent, scene["pre_plan"], scene["have_traj"], st, HALF, PC.CLOUD_R, m.origin, m.resolution, m.grid, int(fp.box_rows.shape[1]), pr)
    got = tuple(a.cpu().numpy() for a in (fp.box_rows, fp.box_count, fp.box_overflow, fp.dropped_own, fp.outrank_boxes, fp.outrank_d2))
    return types.SimpleNamespace(scene=scene, fp=fp, fleet=fleet, state=state, map=m, priority=pr, ent=ent, got=got, want=want)


def _same_ranked(got, want, tag, fresh=True):
    for f, a, b in zip(("count", "overflow", "dropped_own", "outrank_boxes"), got[1:5], want[1:5]):
        assert np.array_equal(a, b), (tag, f, a[:8], b[:8])
    assert np.array_equal(got[5].view(np.uint64), want[5].view(np.uint64)), (tag, "outrank_d2", got[5][:8], want[5][:8])
    for b in range(len(want[1])):
        n = max(int(want[1][b]), 0)
        assert np.array_equal(got[0][b, :n], want[0][b, :n]), (tag, b, got[0][b, :n], want[0][b, :n])
        assert not (fresh and got[0][b, n:].any()), (tag, b)     # rows past a count were never written (fresh: into zeroed tensors)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("map_name", sorted(MAPS))
@pytest.mark.parametrize("B", PC.SIZES)
def test_a_the_ranked_boxes_are_the_oracle_to_the_bit(B, map_name, pattern):
    c = _ranked_case("crowd" if B == 70 else "k3", B, map_name, pattern)
    _same_ranked(c.got, c.want, (B, map_name, pattern))
    if B == 70:
        assert c.want[2][0] == 1                                 # planner 0 has more than 64 peers
    if B in (5, 260) and map_name == "full":                    # (the crowd stands within a box's half edge: there every box holds the planner's own voxel)
        assert c.want[4].sum() > 0 and (c.want[5] < PC.CLOUD_R * PC.CLOUD_R).any() and (c.want[5] == PC.CLOUD_R * PC.CLOUD_R).any()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("B", (5, 70, 260))
def test_b_the_two_identities_against_the_peer_boxes_launch_itself(B, pattern):
    c = _ranked_case("k8", B, "full", pattern)
    _same_ranked(c.got, c.want, (B, pattern))
    c.fp.boxes(c.fleet, c.state, c.map, HALF)                   # the existing launch, into the same tensors
    full = tuple(a.cpu().numpy() for a in (c.fp.box_rows, c.fp.box_count, c.fp.box_overflow, c.fp.dropped_own))
    g = PC.CLOUD_GRID
    f0 = solver.FleetPeers(B, g["origin"], g["dims"], g["cell"], PC.CLOUD_R, 0.25, 0.125, S=1, stages=(), device=DEV)
    f0.boxes(c.fleet, c.state, c.map, HALF, Q=int(c.fp.box_rows.shape[1]))
    bodies = tuple(a.cpu().numpy() for a in (f0.box_rows, f0.box_count, f0.box_overflow, f0.dropped_own))
    with np.errstate(invalid="ignore"):
        D2 = PO.dist2(c.scene["state"][:, :3])
    seen = collections.Counter()
    for b in range(B):
        peers = [q for q in range(B) if q != b and c.ent[b] and c.ent[q] and D2[b, q] <= PC.CLOUD_R * PC.CLOUD_R]
        up = [RO.outranks(c.priority, q, b) for q in peers]
        for cond, other, tag in ((all(up), full, "all_outrank"), (not any(up), bodies, "outranks_all")):
            if peers and cond:
                seen[tag] += 1
                n = max(int(other[1][b]), 0)
                assert all(c.got[i][b] == other[i][b] for i in (1, 2, 3)) and np.array_equal(c.got[0][b, :n], other[0][b, :n]), (tag, b)
    assert seen["all_outrank"] >= 1 and seen["outranks_all"] >= 1, seen


def test_c_exact_fill_and_one_row_too_few():
    n = int(_ranked_case("k8", 70, "full", "reversed").want[1].max())
    assert n > 1
    for Q in (n, n - 1):
        c = _ranked_case("k8", 70, "full", "reversed", Q=Q)
        _same_ranked(c.got, c.want, Q)
        assert (c.want[1] == (n if Q == n else -n)).any()
        assert not c.got[0][c.want[1] < 0].any()                # an overflowing planner stored nothing


# ---- hold and release: a scripted sequence through the library on plain tensors ----
PAR = dict(r_release=0.5, n_clear=2, a_brake=2.0, hold_timeout=4)
STEPS = 14
OWN = [n for n, _ in capi.YieldArgs._fields_[13:]]            # the arrays the rule owns, in the struct's order


def _script(B, seed):
    """Per step: what the state machine, the search, the boxes and the caller hand the rule -- drawn so that every branch is taken."""
    rng = np.random.default_rng([seed, B])
    out = []
    for k in range(STEPS):
        i = lambda lo, hi: rng.integers(lo, hi, B).astype(np.int32)
        odom = rng.random((B, 9)) * 4.0 - 2.0
        odom[rng.random(B) < 0.08, int(rng.integers(0, 6))] = (np.nan, np.inf)[k % 2]
        out.append(dict(fsm=dict(state=rng.choice([1, 3, 4, 5, 5], B).astype(np.int32), have_target=i(0, 2), have_traj=i(0, 2), exec_mpc=i(0, 2), plan_fail_count=i(0, 5),
                                 cmd_status=i(0, 5), pub_end=i(0, 2)),
                        status=rng.choice([0, 2, 3, 3, 3], B).astype(np.int32), up_boxes=rng.choice([0, 1, 6], B).astype(np.int32),
                        up_d2=rng.choice([0.1, 0.25, np.nextafter(0.25, 1.0), 0.6], B), end_pt=rng.random((B, 3)) * 9.0, odom=odom, fleet_have=i(0, 2),
                        goal_in=rng.random((B, 3)) * 5.0, fresh_in=(rng.random(B) < 0.2).astype(np.int32), no_goals=k % 5 == 4,
                        mask=(rng.random(B) < 0.5).astype(np.int32) if k == 8 else None))
    return out


def _run_script(B, a_brake, count):
    import torch
    l = solver.lib()
    par = dict(PAR, a_brake=a_brake)
    y = RO.new_yield(B)
    dy = {n: _dev(v, v.dtype) for n, v in y.items()}
    cmd_end = np.zeros((B, 3))
    filler = torch.zeros((B, 9), dtype=torch.float64, device=DEV)           # the state machine's fields the rule does not touch
    for k, s in enumerate(_script(B, 11)):
        status = s["status"].copy()
        fsm = {n: v.copy() for n, v in s["fsm"].items()}
        fleet_have = s["fleet_have"].copy()
        d = dict(fsm={n: _dev(v, np.int32) for n, v in fsm.items()}, status=_dev(status, np.int32), cmd_end=_dev(cmd_end, np.float64), fleet_have=_dev(fleet_have, np.int32),
                 end_pt=_dev(s["end_pt"], np.float64), odom=_dev(s["odom"], np.float64), up_boxes=_dev(s["up_boxes"], np.int32), up_d2=_dev(s["up_d2"], np.float64),
                 goal_in=_dev(s["goal_in"], np.float64), fresh_in=_dev(s["fresh_in"], np.int32))
        goals = (None, None) if s["no_goals"] else (s["goal_in"], s["fresh_in"])
        if s["mask"] is not None:                                          # one reset under a mask in between
            ya = capi.YieldArgs(B, par["n_clear"], par["hold_timeout"], par["r_release"], par["a_brake"], *([None] * 8), *[dy[n].data_ptr() for n in OWN])
            d["mask"] = _dev(s["mask"], np.int32)
            assert l.frp_nmpc_yield_reset(ctypes.byref(ya), d["mask"].data_ptr(), None) == 0
            RO.yield_reset(y, s["mask"])
        RO.yield_step(y, fsm, s["end_pt"], cmd_end, s["odom"], status, s["up_boxes"], s["up_d2"], goals[0], goals[1], fleet_have, count=count, **par)
        ya = capi.YieldArgs(B, par["n_clear"], par["hold_timeout"], par["r_release"], par["a_brake"], d["odom"].data_ptr(), d["status"].data_ptr(), d["up_boxes"].data_ptr(),
                            d["up_d2"].data_ptr(), None if s["no_goals"] else d["goal_in"].data_ptr(), None if s["no_goals"] else d["fresh_in"].data_ptr(),
                            d["fleet_have"].data_ptr(), d["cmd_end"].data_ptr(), *[dy[n].data_ptr() for n in OWN])
        fields = {n: filler.data_ptr() for n, _ in capi.Fsm._fields_[1:]}
        fields.update({n: t.data_ptr() for n, t in d["fsm"].items()})
        fields["end_pt"] = d["end_pt"].data_ptr()
        fs = capi.Fsm(B, *[fields[n] for n, _ in capi.Fsm._fields_[1:]])
        assert l.frp_nmpc_yield_step(ctypes.byref(ya), ctypes.byref(fs), None) == 0
        torch.cuda.synchronize()
        for n in y:
            assert _same(dy[n].cpu().numpy(), y[n]), (B, k, n, dy[n].cpu().numpy()[:8], y[n][:8])
        for n in fsm:
            assert np.array_equal(d["fsm"][n].cpu().numpy(), fsm[n]), (B, k, n)
        assert np.array_equal(d["status"].cpu().numpy(), status) and np.array_equal(d["fleet_have"].cpu().numpy(), fleet_have), (B, k)
        assert _same(d["cmd_end"].cpu().numpy(), cmd_end), (B, k, "cmd_end_pt")
        assert not filler.any()
    return y


@pytest.mark.parametrize("B", PC.SIZES)
def test_d_the_step_is_the_oracle_to_the_bit_on_a_script_that_takes_every_branch(B):
    count = collections.Counter()
    y = _run_script(B, PAR["a_brake"], count)
    if B >= 70:
        missing = [n for n in RO.BRANCHES_STEP if count[n] == 0 and n != "brake_inf"]
        assert not missing, missing
        assert y["holds"].sum() > 0 and y["releases"].sum() > 0 and y["timeouts"].sum() > 0 and y["bad"].sum() > 0
    if B == 5:
        _run_script(B, float("inf"), count)
        assert count["brake_inf"] > 0


# ---- the closed loop: tests/test_gpu_peers_avoid.py's 8-planner flight with right of way attached ----
ROW = dict(r_release=0.8, n_clear=3, a_brake=2.0, hold_timeout=12)


def _flight(mode, crossing):
    """PERIODS periods of Mission.clock -> Mission.step -> FleetPeers.boxes -> [RightOfWay.step] -> check_paths -> FleetFSM.period -> FleetPeers.update.
    mode: "avoid" (symmetric boxes, no RightOfWay), "row" (eager, the oracle applied period by period) or "graph" (everything after
    period 0 one captured graph)."""
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
    stages = (2, 5, 9)
    fp = solver.FleetPeers(veh, LOOP_GRID["origin"], LOOP_GRID["dims"], LOOP_GRID["cell"], PC.R, PC.D_WARN, PC.D_HIT, S=5, stages=stages)
    clock = m.clock_out[:3]
    pl.overlay = fp
    row = solver.RightOfWay(fp, fsm, pl, **ROW) if mode != "avoid" else None
    log, oracle = [], RO.new_yield(FB)
    host = lambda a: a.cpu().numpy().copy()

    def period(stream=None, check=False):
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            m.clock(0.0, 1, stream=stream)
            m.step(veh.state, clock, None, stream=stream)
            if row is None:
                fp.boxes(fleet, veh.state, dm, BOX_HALF, stream=stream)
                goal, fresh = m.goal, m.fresh
            else:
                fp.boxes(fleet, veh.state, dm, BOX_HALF, stream=stream, priority=row.priority)
                if check:                                                   # the oracle on what the device is about to read
                    st, have, plan = host(veh.state), host(fleet.have_traj), host(fleet.pre_plan)
                    ent = PO.entered(st[:, None, :3], LOOP_GRID["origin"], LOOP_GRID["dims"], LOOP_GRID["cell"])[:, 0]
                    want = RO.boxes_ranked(st, ent, plan, have, stages, BOX_HALF, PC.R, dm.origin, dm.resolution, dm.grid, int(fp.box_rows.shape[1]), None)
                    got = tuple(host(a) for a in (fp.box_rows, fp.box_count, fp.box_overflow, fp.dropped_own, fp.outrank_boxes, fp.outrank_d2))
                    _same_ranked(got, want, ("period", len(log)), fresh=False)
                    f = {n: host(getattr(fsm, n)) for n in RO.FSM_FIELDS}
                    status, cmd_end = host(pl.status), host(fsm.tick.cmd_end_pt)
                    RO.yield_step(oracle, f, host(fsm.end_pt), cmd_end, st, status, want[4], want[5], host(m.goal), host(m.fresh), have, **ROW)
                row.step(veh.state, m.goal, m.fresh, stream=stream)
                if check:
                    for n, a in row.arrays().items():
                        assert _same(a, oracle[n]), (len(log), n, a, oracle[n])
                    for n in RO.FSM_FIELDS:
                        assert np.array_equal(host(getattr(fsm, n)), f[n]), (len(log), n)
                    assert np.array_equal(host(pl.status), status) and np.array_equal(host(fleet.have_traj), have) and _same(host(fsm.tick.cmd_end_pt), cmd_end), len(log)
                    log.append((int(fp.box_count.clamp(min=0).sum().item()), host(row.holding).tolist()))
                goal, fresh = row.goal, row.fresh
            fp.check_paths(pl, fsm, stream=stream)
            fsm.period(pl, dm, None, clock, cloud, goal=goal, goal_fresh=fresh, fsm_steps=1, vehicle=veh, stream=stream)
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
            period(check=mode == "row")
    torch.cuda.synchronize()
    out = {"fsm." + n: a for n, a in fsm.arrays().items()}
    out.update({"peers." + n: a for n, a in fp.arrays().items()})
    out.update({"mission." + n: a for n, a in m.arrays().items()})
    out.update({"vehicle.x": veh.x.cpu().numpy(), "z": fleet.solver.z.cpu().numpy(), "poly_A": fleet.poly_A.cpu().numpy(), "poly_b": fleet.poly_b.cpu().numpy(),
                "kino_path": pl.kino_path.cpu().numpy(), "kino_size": pl.kino_size.cpu().numpy(), "astar.status": pl.status.cpu().numpy(),
                "boxes.count": fp.box_count.cpu().numpy(), "boxes.path_hit": fp.path_hit.cpu().numpy(), "boxes.dropped_own": fp.dropped_own.cpu().numpy()})
    if row is not None:
        out.update({"row." + n: a for n, a in row.arrays().items()})
    if mode == "row":                                           # RightOfWay.reset under a mask, against the oracle's
        mask = np.array([0, 1] * (FB // 2), dtype=np.int32)
        row.reset(_dev(mask, np.int32))
        RO.yield_reset(oracle, mask)
        for n, a in row.arrays().items():
            assert _same(a, oracle[n]), ("reset", n)
        row.reset()
        assert not any(a.any() for a in row.arrays().values())
    return out, log


def test_e_a_crossing_flight_with_right_of_way_captured_is_the_eager_one_and_the_oracle():
    eager, log = _flight("row", True)
    print("crossing flight with right of way: (boxes, holding) per period", log, "sep2_min", eager["peers.sep2_min"].tolist(), "hit_samples",
          eager["peers.hit_samples"].tolist(), {n: eager["row." + n].tolist() for n in ("holds", "releases", "timeouts", "hold_periods", "longest_hold", "bad")})
    assert sum(h[0] for h in log) > 0                          # the two crossing vehicles came within R: boxes existed
    assert eager["row.holds"][1] >= 1 and eager["row.releases"][1] + eager["row.timeouts"][1] >= 1       # the outranked vehicle held and was let go
    assert eager["row.holds"][0] == 0                          # the outranking one never held
    replay, _ = _flight("graph", True)
    assert set(eager) == set(replay)
    for n in sorted(eager):
        assert _same(eager[n], replay[n]), (n, eager[n], replay[n])


def test_f_without_a_crossing_right_of_way_changes_no_plan_no_state_and_no_counter():
    with_row, log = _flight("row", False)
    without, _ = _flight("avoid", False)
    assert sum(h[0] for h in log) == 0 and not any(any(h[1]) for h in log)
    for n in ("holds", "releases", "timeouts", "hold_periods", "longest_hold", "bad", "holding"):
        assert not with_row["row." + n].any(), n
    for n in sorted(without):
        assert _same(with_row[n], without[n]), n
