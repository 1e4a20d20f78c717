"""GPU tests of the mission (include/frp_nmpc.h section 17, csrc/frp_mission.hip, solver.Mission): every synthetic case of
tests/mission_cases.py at B = 1, 5 (a partly filled workgroup) and 260 (65 workgroups) against tests/mission_oracle.py, every state array
and output bit for bit after each of eight consecutive calls; a fleet against its halves and one call of four tries against four calls of
one, on the device, eager and replayed from a hipGraph; the clock replayed five times; and a closed loop: Mission.clock -> Mission.step ->
FleetFSM.period captured once and replayed for a whole flight with nothing written by the host, against an eager flight in which the host
reads the state machine back every period, runs the oracle and feeds goal, fresh and clock itself.  Everything is exact: there is no
transcendental on this path."""
import numpy as np
import pytest

from forces_resilient_planner_amd import capi, layout as L, solver, workloads

from . import mission_cases as MC
from . import mission_oracle as MO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIELDS = MO.INT_FIELDS + MO.F64_FIELDS


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)


class StubFsm:
    """What solver.Mission takes of a FleetFSM, for the synthetic cases: have_odom, have_target and end_pt of B planners (every other array
    of the struct points at one scratch tensor: the step reads these three alone)."""

    def __init__(self, B):
        import torch
        self.torch, self.B = torch, B
        self.state = torch.zeros((max(B, 1) * 9,), dtype=torch.int32, device=DEV)
        self.have_odom, self.have_target = (torch.zeros((B,), dtype=torch.int32, device=DEV) for _ in range(2))
        self.end_pt = torch.zeros((B, 3), dtype=torch.float64, device=DEV)

    def struct(self):
        own = dict(have_odom=self.have_odom, have_target=self.have_target, end_pt=self.end_pt)
        return capi.Fsm(self.B, *[own.get(n, self.state).data_ptr() for n, _ in capi.Fsm._fields_[1:]])


@pytest.fixture(scope="module")
def occmap():
    dm = solver.OccupancyMap(origin=MC.MAP_ORIGIN, map_size=MC.MAP_SIZE, resolution=MC.MAP_RES, device=DEV)
    dm.insert_cloud(MC.map_points())
    assert tuple(dm.grid) == (40, 40, 20)
    return dm


def _mission(par, B):
    kw = {n: par[n] for n in ("loop", "arrive_radius", "dwell", "leg_timeout", "seed", "id0")}
    if par["route"] is not None:
        kw.update(route=par["route"], route_len=par["route_len"])
    else:
        kw.update({n: par[n] for n in ("goal_box", "z_goal", "min_dist", "max_dist", "R", "inflate_ratio")})
    return solver.Mission(StubFsm(B), **kw)


def _load(m, state, clock, inputs):
    f = m.fsm
    f.have_odom.copy_(_dev(inputs["have_odom"], np.int32)); f.have_target.copy_(_dev(inputs["have_target"], np.int32))
    f.end_pt.copy_(_dev(inputs["end_pt"], np.float64)); state.copy_(_dev(inputs["state"], np.float64))
    clock.copy_(_dev([inputs["now"], inputs["now"] + 0.01, inputs["now"] + 0.02], np.float64))


def _play(name, B, dm, id0=0, R=None, step=None):
    """A case on the device, call by call; returns every call's arrays.  step(m, state, clock, occ): the launch (default: eager)."""
    import torch
    par, frames, _ = MC.run(name, B, id0, R)
    m = _mission(par, B)
    occ = dm if MC.CASES[name][1] else None
    state, clock = torch.zeros((B, 9), dtype=torch.float64, device=DEV), torch.zeros((3,), dtype=torch.float64, device=DEV)
    launch = step(m, state, clock, occ) if step else (lambda: m.step(state, clock, occ))
    out = []
    for inputs, _ in frames:
        _load(m, state, clock, inputs)
        launch()
        out.append(m.arrays())
    return frames, out


@pytest.mark.parametrize("B", MC.SIZES)
@pytest.mark.parametrize("name", list(MC.CASES))
def test_a_every_synthetic_case_is_the_oracle_to_the_bit_after_every_call(occmap, name, B):
    frames, got = _play(name, B, occmap)
    assert len(got) == MC.CALLS
    for n, ((_, want), have) in enumerate(zip(frames, got)):
        for f in FIELDS:
            assert _same(have[f], want[f]), (name, B, n, f, have[f][:8], want[f][:8])
    last = frames[-1][1]
    if B > 1 and not name.endswith(("walled", "edge")):
        assert last["issued"].sum() > 0 and (name == "route_w1" or last["reached"].sum() + last["dropped"].sum() > 0)


def _graph_step(m, state, clock, occ):
    import torch
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                     # (a first launch outside the capture)
        m.reset(stream=side)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        m.step(state, clock, occ, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    return g.replay


@pytest.mark.parametrize("name", ["random_r4_open", "random_r4", "route_w3"])
def test_b_a_fleet_is_its_halves_and_a_replayed_step_is_the_eager_one(occmap, name):
    _, whole = _play(name, 10, occmap)
    _, lo = _play(name, 5, occmap, 0)
    _, hi = _play(name, 5, occmap, 5)
    _, replayed = _play(name, 10, occmap, step=_graph_step)
    for n in range(MC.CALLS):
        for f in FIELDS:
            assert _same(whole[n][f], np.concatenate([lo[n][f], hi[n][f]])), (name, n, f)
            assert _same(whole[n][f], replayed[n][f]), (name, n, f)
    assert whole[-1]["issued"].sum() > 10


@pytest.mark.parametrize("name", ["random_r4_open", "random_r4_walled", "random_r4"])
def test_c_one_call_of_four_tries_is_four_calls_of_one(occmap, name):
    import torch
    B = 12
    occ = occmap if MC.CASES[name][1] else None
    par4, _ = MC.case_params(name, B)
    par1, _ = MC.case_params(name, B, R=1)
    a, c = _mission(par4, B), _mission(par1, B)
    state = _dev([MC.start_pos(b) + [0.0] * 6 for b in range(B)], np.float64)
    clock = _dev([1.0, 1.01, 1.02], np.float64)
    for m in (a, c):
        m.fsm.have_odom.fill_(1)
    a.step(state, clock, occ)
    for _ in range(4):
        c.fsm.have_target.copy_((c.phase == solver.MISSION_FLYING).to(torch.int32))      # (once it flies, the target is held)
        c.step(state, clock, occ)
    x, y = a.arrays(), c.arrays()
    for f in ("phase", "leg", "tries", "issued", "t_mark", "goal"):
        assert _same(x[f], y[f]), (name, f)
    assert np.all((x["blocked"] == 0) | ((x["blocked"] == 1) & (y["blocked"] == 4)))
    # ... and both are the oracle's
    for b in range(B):
        v = MO.new_vehicle()
        MO.step(v, par4, b, 1.0, 1, 0, [0.0] * 3, MC.start_pos(b), MC.map_oracle() if occ is not None else None)
        for f in FIELDS:
            assert _same(np.array(v[f]), x[f][b]) or f == "fresh", (name, b, f)


def test_d_the_clock_replayed_five_times_and_at_large_counters():
    import torch
    m = _mission(MC.case_params("route_w1", 1)[0], 1)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        m.clock(MC.T0, 1, advance=0, stream=side)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        view = m.clock(MC.T0, 1, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert tuple(view.shape) == (3,) and int(m.k.item()) == 0
    for k in range(5):
        g.replay()
        torch.cuda.synchronize()
        want = solver.FleetFSM.clock_for(MC.T0 + 0.05 * k, 1)
        assert _same(view.cpu().numpy(), np.array(want)) and _same(np.array(MO.clock(k, MC.T0, 0.05, 0.01, 3)), np.array(want)) and int(m.k.item()) == k + 1, k
    for k in (7, 2 ** 20, 2 ** 40):
        m.k.fill_(k)
        got = m.clock(0.125, 5, advance=3).cpu().numpy()
        assert _same(got, np.array(solver.FleetFSM.clock_for(0.125 + 0.05 * k, 5))) and int(m.k.item()) == k + 3, k


def test_e_reset_under_a_mask(occmap):
    frames, _ = _play("random_r4_open", 5, occmap)
    par, _, _ = MC.run("random_r4_open", 5)
    m = _mission(par, 5)
    for f in FIELDS:
        getattr(m, f).copy_(_dev(frames[-1][1][f], np.int32 if f in MO.INT_FIELDS else np.float64))
    m.reset(mask=_dev([1, 0, 1, 0, 0], np.int32))
    got, fresh = m.arrays(), MC.arrays([MO.new_vehicle() for _ in range(5)])
    for f in FIELDS:
        want = frames[-1][1][f].copy()
        want[[0, 2]] = fresh[f][[0, 2]]
        assert _same(got[f], want), f


# ---- the closed loop in one graph ----
FB = 8
PERIODS = 260
# CHOSEN ON THE GPU: three waypoints 1.5 m apart along x.  Measured on an MI355X: the route vehicles arrive in periods 48, 105 and 150,
# the vehicle on seeded goals in 50, 149 and 234 (printed below) -- 260 periods hold every route's three arrivals with a margin
LEG = 1.5
LANES = np.array([-8.05, -6.55, -5.05, -3.55, -2.05, 2.05, 3.55, 5.05])
RANDOM_VEHICLE = 7
RANDOM_BOX = (-7.0, -3.0, 4.5, 5.6)
WEIGHTS = (15.0, 3.0, 80.0, 15.0, 0.0)


def _flight(graph):
    """PERIODS periods of clock -> step (a route mission and a random one) -> FleetFSM.period(goal, goal_fresh, clock, vehicle).
    graph: everything after period 0 is ONE captured graph, replayed; the host writes nothing.  Otherwise the host reads the state machine
    back before every period, runs the oracle and uploads goal, fresh and clock.  Returns every array at the end, and the oracle's vehicles."""
    import torch
    w = workloads.astar_world(0, "empty", allocate_num=12000)
    dm = solver.OccupancyMap(w)
    pillar = np.array([(x, y, z) for x in np.arange(-0.25, 0.26, 0.1) for y in np.arange(-0.25, 0.26, 0.1) for z in np.arange(-0.95, 2.96, 0.1)], dtype=np.float32)
    dm.insert_cloud(pillar)                                                                     # (the other closed-loop tests' world: one pillar at the origin, far from every lane)
    fleet = solver.DeviceFleet(FB, 20, 30, 64, L.MODEL_NORMAL, WEIGHTS, weights_final=WEIGHTS)
    fleet.poly_index = torch.zeros((FB, 20), dtype=torch.int32, device=DEV)
    fsm = solver.FleetFSM(fleet)
    pl = solver.AstarPlanner(dm, FB, K=512)
    fsm.bind(pl)
    cloud = _dev(pillar.astype(np.float64), np.float64)
    veh = solver.Vehicle(fleet)
    start = np.zeros((FB, 9)); start[:, 0] = -6.05; start[:, 1] = LANES; start[:, 2] = 1.2
    route = np.array([[[-6.05 + LEG * (k + 1), y, 1.2] for k in range(3)] for y in LANES])
    veh.reset(_dev(start, np.float64))
    veh.odometry(fsm)
    common = dict(arrive_radius=0.3, dwell=0.1, leg_timeout=30.0)
    par_r = MO.params(route=route.tolist(), route_len=[3] * FB, **common)
    par_x = MO.params(goal_box=RANDOM_BOX, min_dist=1.0, max_dist=2.5, R=4, seed=11, id0=100, **common)
    m_r = solver.Mission(fsm, route=route, **common)
    m_x = solver.Mission(fsm, goal_box=RANDOM_BOX, min_dist=1.0, max_dist=2.5, R=4, seed=11, id0=100, **common)
    pick = torch.zeros((FB,), dtype=torch.bool, device=DEV); pick[RANDOM_VEHICLE] = True
    goal, fresh = torch.zeros((FB, 3), dtype=torch.float64, device=DEV), torch.zeros((FB,), dtype=torch.int32, device=DEV)
    clock = m_r.clock_out[:3]
    v_r, v_x = [MO.new_vehicle() for _ in range(FB)], [MO.new_vehicle() for _ in range(FB)]
    occ = MC.OO.from_world(w)
    occ.insert_cloud(pillar)

    def missions(stream=None):
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            m_r.clock(0.0, 1, stream=stream)
            m_r.step(veh.state, clock, None, stream=stream)
            m_x.step(veh.state, clock, dm, stream=stream)
            torch.where(pick[:, None], m_x.goal, m_r.goal, out=goal)
            torch.where(pick, m_x.fresh, m_r.fresh, out=fresh)

    def period(stream=None):
        return fsm.period(pl, dm, None, clock, cloud, goal=goal, goal_fresh=fresh, fsm_steps=1, vehicle=veh, stream=stream)

    def host_missions(k):
        a = fsm.arrays()
        pos = veh.state.cpu().numpy()
        now = MO.clock(k, 0.0, 0.05, 0.01, 3)
        for b in range(FB):
            MO.step(v_r[b], par_r, b, now[0], int(a["have_odom"][b]), int(a["have_target"][b]), a["end_pt"][b], pos[b, 0:3])
            MO.step(v_x[b], par_x, b, now[0], int(a["have_odom"][b]), int(a["have_target"][b]), a["end_pt"][b], pos[b, 0:3], occ)
        src = [v_x[b] if b == RANDOM_VEHICLE else v_r[b] for b in range(FB)]
        goal.copy_(_dev([v["goal"] for v in src], np.float64)); fresh.copy_(_dev([v["fresh"] for v in src], np.int32))
        m_r.clock_out[:3].copy_(_dev(now, np.float64))

    g = None
    arrivals = {}
    for k in range(PERIODS):
        if graph:
            if g is None:
                missions(); period()
                torch.cuda.synchronize()
                side = torch.cuda.Stream()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    missions(torch.cuda.current_stream()); period(torch.cuda.current_stream())
                torch.cuda.synchronize()
            else:
                g.replay()                                  # ---- the host writes nothing and reads nothing ----
        else:
            host_missions(k)
            period()
            for b in range(FB):
                if v_r[b]["reached"] > len(arrivals.get(b, ())):
                    arrivals.setdefault(b, []).append(k)
    torch.cuda.synchronize()
    out = {"fsm." + n: a for n, a in fsm.arrays().items()}
    out["vehicle.x"] = veh.x.cpu().numpy()
    if graph:
        out.update({"route." + n: a for n, a in m_r.arrays().items() if n != "k"})
        out.update({"random." + n: a for n, a in m_x.arrays().items() if n != "k"})
        assert int(m_r.k.item()) == PERIODS
    else:
        out.update({"route." + n: a for n, a in MC.arrays(v_r).items()})
        out.update({"random." + n: a for n, a in MC.arrays(v_x).items()})
        print("arrivals of the route vehicles (periods):", arrivals)
    return out


def test_f_a_whole_flight_of_graph_replays_is_the_flight_the_host_steers_with_the_oracle():
    eager = _flight(False)
    replay = _flight(True)
    print("reached", eager["route.reached"].tolist(), "issued", eager["route.issued"].tolist(), "dropped", eager["route.dropped"].tolist(),
          "random vehicle: issued", int(eager["random.issued"][RANDOM_VEHICLE]), "reached", int(eager["random.reached"][RANDOM_VEHICLE]), "blocked",
          int(eager["random.blocked"][RANDOM_VEHICLE]))
    assert set(eager) == set(replay)
    for n in sorted(eager):
        assert _same(eager[n], replay[n]), (n, eager[n], replay[n])
    assert eager["route.reached"][:RANDOM_VEHICLE].max() >= 2, eager["route.reached"]
    assert eager["random.issued"][RANDOM_VEHICLE] >= 1
