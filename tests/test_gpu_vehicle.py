"""GPU tests of the vehicle (include/frp_nmpc_vehicle.h, csrc/frp_vehicle.hip, solver.Vehicle): the kernels against the 50-digit scheme of
tests/golden/vehicle_mp.npz tiled over one full workgroup plus one vehicle, the trace against one-sample calls, the argument checks and
the masks, step -> message -> odometry replayed from a hipGraph, and FleetFSM.period(vehicle=...) flying a small fleet to its goals on a
map with nothing copied to the host inside the loop.

The parity bound is the fixture's: 8 times the error of tests/vehicle_oracle.py on the same case (tol_case; tol_hold, tol_msg, tol_odo
for the kept yaw, the message and the callback), the margin tests/golden/astar_mp.npz set -- it covers the device's sincos, sqrt,
division, asin and atan2, each within an ulp or so of libm's, over S * n_sub steps."""
import os
import types

import numpy as np
import pytest

from forces_resilient_planner_amd import layout as L, solver, workloads

from . import vehicle_cases as VC
from . import vehicle_oracle as VO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, S = 257, VC.S
FRP_ERR_ARG = -1003
SCALARS = dict(mass=VC.MASS, g=VC.G, dt_cmd=VC.DT_CMD, **VC.GAINS)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "vehicle_mp.npz"))


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _err(got, pair):
    got = np.asarray(got, dtype=np.float64)
    return np.abs((got - pair[..., 0]) - pair[..., 1])


def _vehicle(n, n_sub, trace=True, odom_type=solver.ODOM_BODY, S_=S):
    """A solver.Vehicle for n vehicles without a fleet behind it (the class reads the fleet's size and device alone)."""
    import torch
    fleet = types.SimpleNamespace(torch=torch, B=n, solver=types.SimpleNamespace(device=torch.device(DEV)))
    return solver.Vehicle(fleet, n_sub=n_sub, odom_type=odom_type, trace=trace, S=S_, **SCALARS)


def _tiled(fx, n_sub, n=B):
    """Vehicle b flies case (b mod 32) of the fixture's cases with this n_sub."""
    idx = np.nonzero(fx["n_sub"] == n_sub)[0]
    assert len(idx) == VC.PER_N_SUB
    return idx[np.arange(n) % len(idx)]


def _load(veh, fx, c):
    veh.x.copy_(_dev(fx["x0"][c], np.float64)); veh.hold.copy_(_dev(fx["hold0"][c], np.float64)); veh.f_true.copy_(_dev(fx["f_true"][c], np.float64))
    return solver.Commands(_dev(fx["cmd"][c], np.float64), _dev(fx["kind"][c], np.int32), None, None, None)


@pytest.fixture(scope="module")
def flown(fx):
    """Both step counts flown once over the tiled cases: {n_sub: (case index [B], x, hold, trace, sat)} on the host, shared and not modified."""
    import torch
    out = {}
    for n_sub in VC.N_SUBS:
        c = _tiled(fx, n_sub)
        veh = _vehicle(B, n_sub)
        veh.step(_load(veh, fx, c))
        torch.cuda.synchronize()
        out[n_sub] = (c, veh.x.cpu().numpy(), veh.hold.cpu().numpy(), veh.trace.cpu().numpy(), veh.sat.cpu().numpy())
    return out


@pytest.mark.parametrize("n_sub", VC.N_SUBS)
def test_a_kernel_against_the_scheme_in_50_digits(fx, flown, n_sub):
    c, x, hold, trace, sat = flown[n_sub]
    factor = float(fx["tol_factor"].reshape(-1)[0])
    e = _err(trace, fx["trace"][c]).reshape(B, -1).max(axis=1)
    bound = factor * fx["tol_case"][c]
    worst = int(np.argmax(e / bound))
    print("n_sub = %d: worst error over bound %.3f (vehicle %d, case %d: %.3e against %.3e)" % (n_sub, e[worst] / bound[worst], worst, c[worst], e[worst], bound[worst]))
    assert np.all(e <= bound), (worst, int(c[worst]), e[worst], bound[worst])
    # exact: the clamps that engaged, the final state = the last trace row, the kept position and zeros; the copies of a case agree to the bit
    assert np.array_equal(sat, fx["sat"][c])
    assert np.array_equal(_bits(x), _bits(trace[:, -1]))
    assert np.array_equal(_bits(hold[:, 0:3]), _bits(fx["hold"][c, 0:3, 0])) and np.array_equal(_bits(hold[:, 4:8]), _bits(np.zeros((B, 4))))
    for b in range(VC.PER_N_SUB, B):
        assert np.array_equal(_bits(trace[b]), _bits(trace[b - VC.PER_N_SUB])) and np.array_equal(_bits(hold[b]), _bits(hold[b - VC.PER_N_SUB])), b
    # the kept yaw: a copy where the last publishing sample was a YAW or nothing was published, an atan2 otherwise
    kind = fx["kind"][c]
    for b in range(B):
        pub = [s for s in range(S) if kind[b, s] in (VO.TRAJ, VO.END, VO.YAW)]
        if not pub:
            assert hold[b, 3] == fx["hold0"][c[b], 3]
        elif kind[b, pub[-1]] == VO.YAW:
            assert hold[b, 3] == fx["cmd"][c[b], pub[-1], 12]
    assert np.all(_err(hold[:, 3], fx["hold"][c, 3]) <= factor * float(fx["tol_hold"].reshape(-1)[0]))


@pytest.mark.parametrize("n_sub", VC.N_SUBS)
def test_b_trace_equals_one_sample_calls(fx, flown, n_sub):
    import torch
    c, x, hold, trace, sat = flown[n_sub]
    veh = _vehicle(B, n_sub, S_=1)
    cmds = _load(veh, fx, c)
    for s in range(S):
        veh.step(solver.Commands(cmds.cmd[:, s:s + 1].contiguous(), cmds.kind[:, s:s + 1].contiguous(), None, None, None))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(veh.x.cpu().numpy()), _bits(trace[:, s])), s
        assert np.array_equal(_bits(veh.trace.cpu().numpy()[:, 0]), _bits(trace[:, s])) and np.array_equal(veh.sat.cpu().numpy()[:, 0], sat[:, s]), s
    assert np.array_equal(_bits(veh.hold.cpu().numpy()), _bits(hold))
    # and without the optional outputs the flight is the same
    bare = _vehicle(B, n_sub, trace=False)
    bare.step(_load(bare, fx, c))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(bare.x.cpu().numpy()), _bits(x)) and np.array_equal(_bits(bare.hold.cpu().numpy()), _bits(hold))


@pytest.mark.parametrize("odom_type", [solver.ODOM_WORLD, solver.ODOM_BODY])
def test_c_message_and_callback_against_the_multiprecision_values(fx, odom_type):
    import torch
    c = np.arange(B) % len(fx["n_sub"])
    veh = _vehicle(B, 4, trace=False, odom_type=odom_type)
    veh.x.copy_(_dev(fx["x_link"][c], np.float64))
    fsm = types.SimpleNamespace(have_odom=torch.zeros((B,), dtype=torch.int32, device=DEV))
    fresh = np.ones(B, dtype=np.int32); fresh[3::7] = 0
    veh.state.fill_(-5.5); veh.state_prev.fill_(6.5)
    veh.odometry(fsm, fresh=_dev(fresh, np.int32))
    torch.cuda.synchronize()
    factor = float(fx["tol_factor"].reshape(-1)[0])
    msg, st, prev, have = veh.msg.cpu().numpy(), veh.state.cpu().numpy(), veh.state_prev.cpu().numpy(), fsm.have_odom.cpu().numpy()
    key = "msg_world" if odom_type == solver.ODOM_WORLD else "msg_body"
    assert np.all(_err(msg, fx[key][c]) <= factor * float(fx["tol_msg"].reshape(-1)[0])), float(_err(msg, fx[key][c]).max())
    assert np.array_equal(_bits(msg[:, 0:3]), _bits(fx["x_link"][c, 0:3])) and np.array_equal(_bits(msg[:, 10:13]), _bits(np.zeros((B, 3))))
    m = fresh != 0
    assert np.all(_err(st[m], fx["odo"][c[m]]) <= factor * float(fx["tol_odo"].reshape(-1)[0])), float(_err(st[m], fx["odo"][c[m]]).max())
    assert np.array_equal(_bits(st[m, 0:3]), _bits(fx["x_link"][c[m], 0:3])) and np.all(prev[m] == -5.5) and np.all(have[m] == 1)
    if odom_type == solver.ODOM_WORLD:
        assert np.array_equal(_bits(st[m, 3:6]), _bits(fx["x_link"][c[m], 3:6]))      # copied
    # a planner without a message keeps its state, its previous state and its flag
    assert np.all(st[~m] == -5.5) and np.all(prev[~m] == 6.5) and np.all(have[~m] == 0) and (~m).sum() >= 30


def test_d_bad_arguments_launch_nothing_and_a_masked_reset_touches_nothing_else(fx):
    import ctypes
    import torch
    n = 8
    veh = _vehicle(n, 4)
    c = _tiled(fx, 4, n)
    cmds = _load(veh, fx, c)
    keep = [t.clone() for t in (veh.x, veh.hold, veh.trace, veh.sat)]
    good = dict(VC.GOOD_STEP, B=n, x=veh.x.data_ptr(), f_true=veh.f_true.data_ptr(), cmd=cmds.cmd.data_ptr(), kind=cmds.kind.data_ptr(),
                hold=veh.hold.data_ptr(), trace=veh.trace.data_ptr(), sat=veh.sat.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for bad in VC.BAD_STEP:
        a = dict(good); a.update(bad)
        vals = [(ctypes.c_double * 3)(*a[f]) if f in ("kp", "kv", "ka") else a[f] for f, _ in solver.VehicleArgs._fields_]
        assert solver.lib().frp_nmpc_vehicle_step(ctypes.byref(solver.VehicleArgs(*vals)), stream) == FRP_ERR_ARG, bad
    l, vp = solver.lib(), ctypes.c_void_p
    x0 = _dev(np.arange(n * 9, dtype=np.float64).reshape(n, 9), np.float64)
    p = lambda t: vp(t.data_ptr())
    have = torch.zeros((n,), dtype=torch.int32, device=DEV)
    assert l.frp_nmpc_vehicle_reset(0, p(x0), None, p(veh.x), p(veh.hold), stream) == FRP_ERR_ARG
    assert l.frp_nmpc_vehicle_reset(n, None, None, p(veh.x), p(veh.hold), stream) == FRP_ERR_ARG
    assert l.frp_nmpc_vehicle_message(n, 3, p(veh.x), p(veh.msg), stream) == FRP_ERR_ARG
    assert l.frp_nmpc_vehicle_message(n, 1, p(veh.x), None, stream) == FRP_ERR_ARG
    assert l.frp_nmpc_vehicle_odometry(n, 0, p(veh.msg), p(veh.fresh), p(veh.state), None, p(have), stream) == FRP_ERR_ARG
    assert l.frp_nmpc_vehicle_odometry(n, 2, p(veh.msg), None, p(veh.state), None, p(have), stream) == FRP_ERR_ARG
    with pytest.raises(ValueError):
        solver.Vehicle(veh.fleet, odom_type=0)
    torch.cuda.synchronize()
    for t, k in zip((veh.x, veh.hold, veh.trace, veh.sat), keep):
        assert torch.equal(t, k)
    assert float(veh.msg.abs().sum()) == 0.0 and float(veh.state.abs().sum()) == 0.0 and int(have.sum()) == 0
    # the masked reset
    mask = np.array([1, 0, 0, 1, 0, 1, 0, 0], dtype=np.int32)
    veh.reset(x0, _dev(mask, np.int32))
    torch.cuda.synchronize()
    x, hold, x0h = veh.x.cpu().numpy(), veh.hold.cpu().numpy(), x0.cpu().numpy()
    m = mask != 0
    assert np.array_equal(x[m], x0h[m]) and np.array_equal(hold[m, 0:3], x0h[m, 0:3]) and np.array_equal(hold[m, 3], x0h[m, 8]) and np.all(hold[m, 4:8] == 0.0)
    assert np.array_equal(_bits(x[~m]), _bits(keep[0].cpu().numpy()[~m])) and np.array_equal(_bits(hold[~m]), _bits(keep[1].cpu().numpy()[~m]))
    assert torch.equal(veh.trace, keep[2]) and torch.equal(veh.sat, keep[3])
    veh.reset(x0)                                                               # no mask: everybody
    torch.cuda.synchronize()
    assert torch.equal(veh.x, x0) and torch.equal(veh.hold[:, 3], x0[:, 8])
    # a reset vehicle hovers: at rest on its own setpoint the speed stays within rounding
    rest = np.zeros((n, 9)); rest[:, 0:3] = fx["x0"][c, 0:3]; rest[:, 8] = fx["x0"][c, 8]
    veh.reset(_dev(rest, np.float64)); veh.f_true.zero_()
    veh.step(solver.Commands(torch.zeros((n, S, 16), dtype=torch.float64, device=DEV), torch.zeros((n, S), dtype=torch.int32, device=DEV), None, None, None))
    torch.cuda.synchronize()
    v = veh.x.cpu().numpy()[:, 3:6]
    assert np.all(np.linalg.norm(v, axis=1) <= S * 4 * (VC.DT_CMD / 4) * VC.G * 2.0 ** -50) and int(veh.sat.abs().sum()) == 0


def test_e_step_message_odometry_replayed_from_a_hipgraph_equals_eager_launches(fx):
    """Captured once on one stream with the default queue count; replayed with new cmd / kind / f_true contents."""
    import torch
    rounds = [_tiled(fx, 4), _tiled(fx, 4)[::-1].copy(), np.roll(_tiled(fx, 4), 5)]

    def feed(veh, cmds, c):
        cmds.cmd.copy_(_dev(fx["cmd"][c], np.float64)); cmds.kind.copy_(_dev(fx["kind"][c], np.int32)); veh.f_true.copy_(_dev(fx["f_true"][c], np.float64))

    def chain(veh, fsm, cmds, stream=None):
        veh.step(cmds, stream)
        veh.odometry(fsm, stream=stream)

    def start(veh, fsm):
        veh.x.copy_(_dev(fx["x0"][rounds[0]], np.float64)); veh.hold.copy_(_dev(fx["hold0"][rounds[0]], np.float64))
        veh.state.zero_(); veh.state_prev.zero_(); veh.msg.zero_(); fsm.have_odom.zero_()

    def make():
        veh = _vehicle(B, 4)
        fsm = types.SimpleNamespace(have_odom=torch.zeros((B,), dtype=torch.int32, device=DEV))
        cmds = solver.Commands(torch.zeros((B, S, 16), dtype=torch.float64, device=DEV), torch.zeros((B, S), dtype=torch.int32, device=DEV), None, None, None)
        return veh, fsm, cmds

    def run(veh, fsm, cmds, fn):
        res = []
        start(veh, fsm)
        for c in rounds:
            feed(veh, cmds, c)
            fn()
            torch.cuda.synchronize()
            res.append([t.clone() for t in (veh.x, veh.hold, veh.trace, veh.sat, veh.msg, veh.state, veh.state_prev, fsm.have_odom)])
        return res

    veh, fsm, cmds = make()
    ref = run(veh, fsm, cmds, lambda: chain(veh, fsm, cmds))
    assert int(fsm.have_odom.sum()) == B and float((ref[2][5] - ref[2][6]).abs().max()) > 0.0     # the states moved, and state_prev follows them
    gv, gf, gc = make()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        chain(gv, gf, gc, side)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        chain(gv, gf, gc, torch.cuda.current_stream())
    torch.cuda.synchronize()
    got = run(gv, gf, gc, g.replay)
    view = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t
    for r, (a, b) in enumerate(zip(got, ref)):
        for i, (p, q) in enumerate(zip(a, b)):
            assert torch.equal(view(p), view(q)), (r, i)


# ---- FleetFSM.period(vehicle=...) on a map ----
WEIGHTS = (15.0, 3.0, 80.0, 15.0, 0.0)
FB = 12
PERIODS = 180
FORCE_AT = 20
FORCED = {1: (1.0, 0.0, 0.0), 6: (0.0, -0.9, 0.0)}            # a force step, true and told, on two planners in flight
NO_GOAL = 11
GOAL_THRESHOLD = 0.15                                           # solveNMPC's "reach the goal" distance (nmpc_solver.cpp:466)
LANES = np.array([-8.05, -6.55, -5.05, -3.55, -2.05, 2.05, 3.55, 5.05, 6.55, 8.05])


def _layout():
    """Ten planners fly 3 m along x in lanes of their own, planner 10 flies 5 m past the pillar at the origin, planner 11 gets no goal."""
    start = np.zeros((FB, 9)); goal = np.zeros((FB, 3))
    start[:10, 0] = -6.05; start[:10, 1] = LANES; goal[:10, 0] = -3.05; goal[:10, 1] = LANES
    start[10, 0:2] = (-2.55, 0.05); goal[10, 0:2] = (2.55, 0.05)
    start[11, 0:2] = (6.05, 0.05)
    start[:, 2] = 1.2; goal[:, 2] = 1.2                                       # goalCallback fixes z at 1.2
    d = goal[:, 0:2] - start[:, 0:2]
    start[:, 8] = np.arctan2(d[:, 1], d[:, 0]); start[NO_GOAL, 8] = 0.4
    return start, goal


def test_f_a_fleet_flies_to_its_goals_with_the_loop_closed_on_the_device(fx):
    """FleetFSM.period(vehicle=...) for PERIODS periods; inside the loop the host writes the period's messages and clock and reads nothing.
    Every period's commands, hold and states are kept in device tensors and read back once after the loop:
      * the oracle, fed a period's commands from the state and hold the device held before them, reproduces the device's next state within
        8 times the oracle's own worst error over the fixture's cases (each period restarts from the device's state: one call's bound);
      * every planner with a goal ends in WAIT_TARGET without a target, its TRUE position inside the reference's goal threshold -- for the
        two under a force plus |f| / kp: on the end point the timer publishes no feed-forward, and a proportional position loop under a
        constant unmodelled acceleration f settles |f| / kp away;
      * the force step, told to the planner as well, makes those two search again at that period; they arrive all the same;
      * the planner without a goal hovers where it was reset."""
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
    veh = solver.Vehicle(fleet)
    start, goal = _layout()
    veh.reset(_dev(start, np.float64))
    veh.odometry(fsm)                                                          # the first message: have_odom, and the state the planner starts from
    f64 = dict(dtype=torch.float64, device=DEV)
    d_goal, d_force = _dev(goal, np.float64), torch.zeros((FB, 3), **f64)
    fresh_goal, fresh_force = torch.zeros((FB,), dtype=torch.int32, device=DEV), torch.zeros((FB,), dtype=torch.int32, device=DEV)
    clock = torch.zeros((3,), **f64)
    hist = dict(x=torch.zeros((PERIODS + 1, FB, 9), **f64), hold=torch.zeros((PERIODS + 1, FB, 8), **f64), cmd=torch.zeros((PERIODS, FB, S, 16), **f64),
                kind=torch.zeros((PERIODS, FB, S), dtype=torch.int32, device=DEV), search=torch.zeros((PERIODS, FB), dtype=torch.int32, device=DEV),
                state=torch.zeros((PERIODS, FB, 9), **f64), fsm=torch.zeros((PERIODS, FB), dtype=torch.int32, device=DEV))
    hist["x"][0].copy_(veh.x); hist["hold"][0].copy_(veh.hold)
    has_goal = np.ones(FB, dtype=np.int32); has_goal[NO_GOAL] = 0
    forced = np.zeros(FB, dtype=np.int32); forced[list(FORCED)] = 1
    f_step = np.zeros((FB, 3))
    for b, f in FORCED.items():
        f_step[b] = f
    for k in range(PERIODS):                                                   # ---- nothing is copied to the host in here ----
        fresh_goal.copy_(_dev(has_goal if k == 0 else 0 * has_goal, np.int32))
        fresh_force.copy_(_dev(forced if k == FORCE_AT else 0 * forced, np.int32))
        if k == FORCE_AT:
            d_force.copy_(_dev(f_step, np.float64)); veh.f_true.copy_(_dev(f_step, np.float64))
        clock.copy_(_dev(solver.FleetFSM.clock_for(0.05 * k, 1), np.float64))
        cmd = fsm.period(pl, dm, None, clock, cloud, goal=d_goal, goal_fresh=fresh_goal, force=d_force, force_fresh=fresh_force, fsm_steps=1, vehicle=veh)
        hist["cmd"][k].copy_(cmd.cmd); hist["kind"][k].copy_(cmd.kind); hist["x"][k + 1].copy_(veh.x); hist["hold"][k + 1].copy_(veh.hold)
        hist["search"][k].copy_(fsm.search); hist["state"][k].copy_(veh.state); hist["fsm"][k].copy_(fsm.state)
    torch.cuda.synchronize()
    h = {n: t.cpu().numpy() for n, t in hist.items()}
    end_pt, final, have_target, have_odom = fsm.end_pt.cpu().numpy(), fsm.state.cpu().numpy(), fsm.have_target.cpu().numpy(), fsm.have_odom.cpu().numpy()
    x = h["x"][-1]
    dist = np.linalg.norm(x[:, 0:3] - end_pt, axis=1)
    print("final FSM states", final.tolist(), "distance to the goal", np.round(dist, 4).tolist())
    print("first period in WAIT_TARGET after the flight", [int(np.argmax((h["fsm"][5:, b] == solver.FSM_WAIT_TARGET))) + 5 for b in range(FB)])
    print("kinds seen", sorted(set(h["kind"].reshape(-1).tolist())), "searches per planner", h["search"].sum(axis=0).tolist())
    # the oracle period by period
    bound = float(fx["tol_factor"].reshape(-1)[0]) * float(np.max(fx["tol_case"]))
    worst = 0.0
    f_true = np.zeros((PERIODS, FB, 3)); f_true[FORCE_AT:] = f_step
    for k in range(PERIODS):
        for b in range(FB):
            xo, ho, _, _ = VO.step(h["x"][k, b], h["hold"][k, b], f_true[k, b], h["cmd"][k, b], h["kind"][k, b], n_sub=solver.VEHICLE_DEFAULTS["n_sub"], **SCALARS)
            worst = max(worst, float(np.max(np.abs(np.array(xo) - h["x"][k + 1, b]))))
            assert ho[0:3] == h["hold"][k + 1, b, 0:3].tolist() and abs(ho[3] - h["hold"][k + 1, b, 3]) <= bound, (k, b)
    print("oracle against the device over %d periods: worst %.3e, bound %.3e" % (PERIODS, worst, bound))
    assert worst <= bound
    # the callbacks handed the planner what the vehicle flew
    assert np.max(np.abs(h["state"] - h["x"][1:])) <= float(fx["tol_factor"].reshape(-1)[0]) * float(fx["tol_odo"].reshape(-1)[0]) and np.all(have_odom == 1)
    assert set(h["kind"].reshape(-1).tolist()) >= {solver.COMMAND_NONE, solver.COMMAND_TRAJ, solver.COMMAND_END}
    # arrival
    with_goal = has_goal != 0
    assert np.all(final[with_goal] == solver.FSM_WAIT_TARGET) and np.all(have_target[with_goal] == 0), (final.tolist(), have_target.tolist())
    assert np.all(np.linalg.norm(start[with_goal, 0:3] - goal[with_goal], axis=1) > 2.9) and np.array_equal(end_pt[with_goal], goal[with_goal])
    allow = np.full(FB, GOAL_THRESHOLD)
    for b, f in FORCED.items():
        allow[b] += np.linalg.norm(f) / min(VC.GAINS["kp"])
    assert np.all(dist[with_goal] < allow[with_goal]), (dist.tolist(), allow.tolist())
    free = with_goal & (forced == 0)
    assert np.all(dist[free] < GOAL_THRESHOLD)
    # the force step: in flight when it came, a new search in that very period, and planners without one did not search then
    for b in FORCED:
        assert h["fsm"][FORCE_AT - 1, b] == solver.FSM_EXEC_TRAJ and h["search"][FORCE_AT, b] == 1, (b, h["fsm"][FORCE_AT - 3:FORCE_AT + 2, b].tolist())
    assert int(h["search"][FORCE_AT][forced == 0].sum()) == 0
    # the planner nobody sent anywhere
    assert final[NO_GOAL] == solver.FSM_INIT and np.linalg.norm(x[NO_GOAL, 0:3] - start[NO_GOAL, 0:3]) < 1e-9 and abs(x[NO_GOAL, 8] - start[NO_GOAL, 8]) < 1e-9
    assert set(h["kind"][:, NO_GOAL].reshape(-1).tolist()) == {solver.COMMAND_NONE}
