"""GPU tests of the disturbance model (include/frp_nmpc.h section 15, csrc/frp_disturbance.hip, csrc/frp_vehicle.hip's field step,
solver.Disturbance): the stand-alone evaluation against the exact scheme (to the bit) and the 50-digit gusts of
tests/golden/disturbance_mp.npz tiled over one full workgroup plus one lane, one S = 5 call against five S = 1 calls and a fleet against its
halves (device against device, to the bit), the fused step against eval + one-sample plain steps, the masks among NaN-poisoned neighbours,
field step -> estimator update -> force callback replayed from a hipGraph, and FleetFSM.period flown for 120 periods through a zone and
an event -- captured once and replayed against eager launches, and held to the chain of the four oracles.

The gust bound is test_gpu_vehicle's rule: 8 times the error of tests/disturbance_oracle.py on the same case (tol_case, which the generator
keeps at or above one unit in the last place of the quantities compared) -- it covers the device's log and cos against libm's; every other
operation of the model is an IEEE one, and without gusts the device is the oracle to the bit."""
import os
import types

import numpy as np
import pytest

from forces_resilient_planner_amd import layout as L, solver

from . import disturbance_cases as DC
from . import disturbance_oracle as DO
from . import vehicle_cases as VC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = DC.B_GPU
SCALARS = dict(mass=VC.MASS, g=VC.G, dt_cmd=VC.DT_CMD, **VC.GAINS)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "disturbance_mp.npz"))


@pytest.fixture(scope="module")
def vfx(golden_dir):
    return np.load(os.path.join(golden_dir, "vehicle_mp.npz"))


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _err(got, pair):
    got = np.asarray(got, dtype=np.float64)
    return np.abs((got - pair[..., 0]) - pair[..., 1])


def _vehicle(n, n_sub=4, trace=True, S_=5):
    import torch
    fleet = types.SimpleNamespace(torch=torch, B=n, solver=types.SimpleNamespace(device=torch.device(DEV)))
    return solver.Vehicle(fleet, n_sub=n_sub, trace=trace, S=S_, **SCALARS)


def _tile(fx, name, n=B, first=0):
    """Lane b takes the scene's case that was built for it (its `lane`), or else case (b mod C): (case index [n], the lanes the fixture
    has values for).  first: the lane of this launch's vehicle 0 (a half of a fleet)."""
    lane = fx[f"{name}_lane"]
    C = len(lane)
    by_lane = {int(l): i for i, l in enumerate(lane)}
    c = np.array([by_lane.get(first + b, (first + b) % C) for b in range(n)])
    return c, np.array([b for b in range(n) if first + b in by_lane], dtype=np.int64)


def _scene(fx, name, n=B, S_=5, first=0, id_shift=0):
    """A solver.Disturbance for scene `name` on n vehicles, loaded with the tiled cases: (dist, case index, fixture lanes, pos, base)."""
    c, known = _tile(fx, name, n, first)
    E, gust, seed, id0 = (int(v) for v in fx[f"{name}_ints"])
    sc = fx[f"{name}_scalars"]
    kw = {}
    if gust:
        src = next(s for s in DC.scenes() if s["name"] == name)["gust"]
        kw = dict(gust_sigma=src["sigma"], gust_tau=src["tau"])
    dist = solver.Disturbance(_vehicle(n, trace=False, S_=S_), zones=fx[f"{name}_zones"], events=fx[f"{name}_events"][c] if E else None, seed=seed, id0=id0 + id_shift,
                              t_epoch=float(sc[0]), **kw)
    if gust:
        assert list(dist.gust_a) == list(sc[2:5]) and list(dist.gust_c) == list(sc[5:8])
        dist.gust.copy_(_dev(fx[f"{name}_g0"][c], np.float64))
    dist.tick.copy_(_dev(fx[f"{name}_tick0"][c], np.int64))
    return dist, c, known, _dev(fx[f"{name}_pos"][c][:, :S_], np.float64), _dev(fx[f"{name}_base"][c], np.float64)


PLAIN = ("box", "many", "bare")
GUSTY = ("box_gust", "bare_gust", "wrap_gust")


@pytest.mark.parametrize("S_", [5, 1])
@pytest.mark.parametrize("name", PLAIN)
def test_a_eval_without_gusts_is_the_exact_scheme_to_the_bit(fx, name, S_):
    import torch
    dist, c, _, pos, base = _scene(fx, name, S_=S_)
    out = torch.full((B, S_, 3), 7.0, dtype=torch.float64, device=DEV)
    dist.eval(pos, advance=True, base=base, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(fx[f"{name}_det"][c][:, :S_]))
    assert np.array_equal(dist.tick.cpu().numpy(), fx[f"{name}_tick0"][c] + S_) and dist.gust is None
    # base NULL is a zero constant part
    zero = dist.eval(pos, base=None)
    again = dist.eval(pos, base=torch.zeros((B, 3), dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(zero.view(torch.int64), again.view(torch.int64))


@pytest.fixture(scope="module")
def gusty(fx):
    """Every gust scene evaluated once with S = 5, advancing: {name: (case index, fixture lanes, force, gust, tick)} on the host, shared."""
    import torch
    out = {}
    for name in GUSTY:
        dist, c, known, pos, base = _scene(fx, name)
        f = dist.eval(pos, advance=True, base=base)
        torch.cuda.synchronize()
        out[name] = (c, known, f.cpu().numpy(), dist.gust.cpu().numpy(), dist.tick.cpu().numpy())
    return out


@pytest.mark.parametrize("name", GUSTY)
def test_b_eval_with_gusts_against_the_50_digit_draws(fx, gusty, name):
    """Within tol_factor = 8 times tol_case on every lane the fixture holds (lanes 0 ... 10 and 255, 256: both sides of the workgroup
    boundary); the other lanes draw other numbers, which test_c holds to these, device against device."""
    import torch
    c, known, f, g, tick = gusty[name]
    factor = float(fx["tol_factor"].reshape(-1)[0])
    assert len(known) == len(DC.GUST_LANES) and np.array_equal(c[known], np.arange(len(known)))
    bound = factor * fx[f"{name}_tol_case"][c[known]]
    e = np.maximum(_err(f[known], fx[f"{name}_force"][c[known]]).reshape(len(known), -1).max(axis=1), _err(g[known], fx[f"{name}_gust"][c[known]][:, 4]).max(axis=1))
    worst = int(np.argmax(e / bound))
    print("%s: worst error over bound %.3f (lane %d: %.3e against %.3e)" % (name, e[worst] / bound[worst], known[worst], e[worst], bound[worst]))
    assert np.all(e <= bound), (worst, e[worst], bound[worst])
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(g)) and np.array_equal(tick, fx[f"{name}_tick0"][c] + 5)
    assert len(np.unique(_bits(g[:, 0]))) == B                                   # every lane draws its own stream
    # S = 1: the first sample alone
    dist, c1, known1, pos, base = _scene(fx, name, S_=1)
    f1 = dist.eval(pos, advance=True, base=base)
    torch.cuda.synchronize()
    e1 = np.maximum(_err(f1.cpu().numpy()[known1, 0], fx[f"{name}_force"][c1[known1]][:, 0]).max(axis=1), _err(dist.gust.cpu().numpy()[known1], fx[f"{name}_gust"][c1[known1]][:, 0]).max(axis=1))
    assert np.all(e1 <= bound), (e1 / bound).max()
    assert np.array_equal(_bits(f1.cpu().numpy()[:, 0]), _bits(f[:, 0]))
    # a pure query leaves gust and tick untouched, and answers what the advancing call answers
    dist, c2, _, pos, base = _scene(fx, name)
    g0, t0 = dist.gust.clone(), dist.tick.clone()
    q = dist.eval(pos, advance=False, base=base)
    torch.cuda.synchronize()
    assert torch.equal(dist.gust.view(torch.int64), g0.view(torch.int64)) and torch.equal(dist.tick, t0)
    assert np.array_equal(_bits(q.cpu().numpy()), _bits(f))


@pytest.mark.parametrize("name", GUSTY)
def test_c_layout_independence_device_against_device(fx, gusty, name):
    import torch
    c, _, f, g, tick = gusty[name]
    # one S = 5 call is five S = 1 calls
    dist, c1, _, _, base = _scene(fx, name, S_=1)
    pos = _dev(fx[f"{name}_pos"][c1], np.float64)
    for s in range(5):
        fs = dist.eval(pos[:, s:s + 1].contiguous(), advance=True, base=base)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(fs.cpu().numpy()[:, 0]), _bits(f[:, s])), s
    assert np.array_equal(_bits(dist.gust.cpu().numpy()), _bits(g)) and np.array_equal(dist.tick.cpu().numpy(), tick)
    # B vehicles at id0 are the two halves with id0 shifted
    for first, n in ((0, 128), (128, B - 128)):
        half, ch, _, pos_h, base_h = _scene(fx, name, n=n, first=first, id_shift=first)
        assert np.array_equal(ch, c[first:first + n])
        fh = half.eval(pos_h, advance=True, base=base_h)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(fh.cpu().numpy()), _bits(f[first:first + n])) and np.array_equal(_bits(half.gust.cpu().numpy()), _bits(g[first:first + n])), first


# ---- the fused step ----
# zones across the fixture's vehicles (vehicle_cases starts them within a few metres of the origin and moves them by centimetres per sample):
# a ramped slab whose face and ramp the vehicles cross while they fly, a hard box around everything, a box that opens at the third sample
def _zones_for(x0):
    med = np.median(x0[:, 0:3], axis=0)
    return [[med[0], -50.0, -50.0, 50.0, 50.0, 50.0, 1.25, -0.5, 0.25, 0.05, -np.inf, np.inf],
            [-50.0, -50.0, -50.0, 50.0, 50.0, 50.0, 0.0, 0.25, 0.0, 0.0, -np.inf, np.inf],
            [-50.0, -50.0, -50.0, 50.0, med[1], 50.0, 0.0, 0.0, -1.5, 2.0, DC.t_of(2, 0.0), np.inf]]


def _load(veh, vfx, c, S_=5):
    veh.x.copy_(_dev(vfx["x0"][c], np.float64)); veh.hold.copy_(_dev(vfx["hold0"][c], np.float64)); veh.f_true.copy_(_dev(vfx["f_true"][c], np.float64))
    return solver.Commands(_dev(vfx["cmd"][c][:, :S_], np.float64), _dev(vfx["kind"][c][:, :S_], np.int32), None, None, None)


def _events(n):
    ev = np.tile(np.array([[DC.t_of(1, 0.0), DC.t_of(4, 0.0), 0.0, 0.75, -0.25], DC.UNUSED]), (n, 1, 1))
    ev[::2, 0, 0] = np.inf
    return ev


@pytest.mark.parametrize("n_sub,with_thrust", [(4, False), (1, False), (4, True)])
def test_d_field_step_equals_eval_then_one_sample_plain_steps(vfx, n_sub, with_thrust):
    import torch
    idx = np.nonzero(vfx["n_sub"] == n_sub)[0]
    c = idx[np.arange(B) % len(idx)]
    zones = _zones_for(vfx["x0"][c])
    kw = dict(zones=zones, events=_events(B), gust_sigma=(0.5, 0.3, 0.2), gust_tau=(0.5, 1.0, 0.25), seed=99, id0=-100)
    fused = _vehicle(B, n_sub)
    dist = solver.Disturbance(fused, **kw)
    est = solver.ForceEstimator(fused) if with_thrust else None
    dist.force.fill_(7.0)
    fused.step(_load(fused, vfx, c))
    torch.cuda.synchronize()
    # the sequence: eval at the position before the sample, then the plain (or observed) step with S = 1 under that force
    seq = _vehicle(B, n_sub, S_=1)
    sd = solver.Disturbance(seq, **kw)
    seq.disturbance = None                                       # (eval alone: seq.step launches the plain step)
    se = solver.ForceEstimator(seq) if with_thrust else None
    cmds = _load(seq, vfx, c)
    base = seq.f_true.clone()
    trace, sat, force, thrust = [], [], [], []
    for s in range(5):
        f = sd.eval(seq.x[:, None, 0:3].contiguous(), advance=True, base=base)
        seq.f_true.copy_(f[:, 0])
        seq.step(solver.Commands(cmds.cmd[:, s:s + 1].contiguous(), cmds.kind[:, s:s + 1].contiguous(), None, None, None))
        torch.cuda.synchronize()
        trace.append(seq.trace[:, 0].clone()); sat.append(seq.sat[:, 0].clone()); force.append(f[:, 0].clone())
        if with_thrust:
            thrust.append(se.thrust[:, 0].clone())
    eq = lambda a, b: torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))
    assert eq(fused.x, seq.x) and eq(fused.hold, seq.hold) and eq(fused.trace, torch.stack(trace, dim=1)) and torch.equal(fused.sat, torch.stack(sat, dim=1))
    assert eq(dist.force, torch.stack(force, dim=1)) and eq(dist.gust, sd.gust) and torch.equal(dist.tick, sd.tick) and int(dist.tick.min()) == int(dist.tick.max()) == 5
    if with_thrust:
        assert eq(est.thrust, torch.stack(thrust, dim=1))
    assert eq(fused.f_true, base)                                # the constant part is read, not written
    # the zones were placed where it matters: within the five samples vehicles see the slab's weight change, ramp values included
    f_host, tr = dist.force.cpu().numpy(), fused.trace.cpu().numpy()
    p_before = np.concatenate([vfx["x0"][c][:, None, 0:3], tr[:, :-1, 0:3]], axis=1)
    w = np.array([[DO.zone_weight(zones[0], p_before[b, s], DC.t_of(s, 0.0))[0] for s in range(5)] for b in range(B)])
    assert np.any((w > 0.0) & (w < 1.0)) and np.any(w == 0.0) and np.any(w == 1.0) and np.any(w.min(axis=1) != w.max(axis=1))
    assert len(np.unique(_bits(f_host[:, :, 0]))) > B


@pytest.mark.parametrize("with_thrust", [False, True])
def test_e_an_empty_disturbance_flies_the_plain_steps_flight(vfx, with_thrust):
    import torch
    idx = np.nonzero(vfx["n_sub"] == 4)[0]
    c = idx[np.arange(B) % len(idx)]
    plain, field = _vehicle(B), _vehicle(B)
    dist = solver.Disturbance(field)
    assert (dist.Z, dist.E, dist.gust) == (0, 0, None)
    if with_thrust:
        pe, fe = solver.ForceEstimator(plain), solver.ForceEstimator(field)
    plain.step(_load(plain, vfx, c)); field.step(_load(field, vfx, c))
    torch.cuda.synchronize()
    eq = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert eq(plain.x, field.x) and eq(plain.hold, field.hold) and eq(plain.trace, field.trace) and torch.equal(plain.sat, field.sat)
    assert int(dist.tick.min()) == int(dist.tick.max()) == 5 and eq(dist.force, field.f_true[:, None, :].expand(B, 5, 3).contiguous())
    if with_thrust:
        assert eq(pe.thrust, fe.thrust) and eq(pe.f_hat, fe.f_hat) and torch.equal(pe.count, fe.count)


def test_f_masks_among_nan_poisoned_neighbours(fx, gusty):
    import torch
    name = "box_gust"
    c, _, f, g, tick = gusty[name]
    dist, _, _, pos, base = _scene(fx, name)
    odd = np.arange(B) % 2 == 1
    m = _dev(odd, np.bool_)
    pos[m] = float("nan"); base[m] = float("nan"); dist.gust[m] = float("nan")
    out = dist.eval(pos, advance=True, base=base)
    torch.cuda.synchronize()
    o, go = out.cpu().numpy(), dist.gust.cpu().numpy()
    assert np.array_equal(_bits(o[~odd]), _bits(f[~odd])) and np.array_equal(_bits(go[~odd]), _bits(g[~odd])) and np.all(np.isnan(o[odd]))
    assert np.array_equal(dist.tick.cpu().numpy(), tick)
    # reset under a mask: the unmasked vehicles keep every bit, NaNs included
    mask = (np.arange(B) % 3 == 0).astype(np.int32)
    keep_g, keep_t = dist.gust.clone(), dist.tick.clone()
    dist.vehicle.reset(torch.zeros((B, 9), dtype=torch.float64, device=DEV), _dev(mask, np.int32))      # Vehicle.reset resets it under the same mask
    torch.cuda.synchronize()
    mm = _dev(mask != 0, np.bool_)
    assert float(dist.gust[mm].abs().sum()) == 0.0 and int(dist.tick[mm].abs().sum()) == 0
    assert torch.equal(dist.gust[~mm].view(torch.int64), keep_g[~mm].view(torch.int64)) and torch.equal(dist.tick[~mm], keep_t[~mm])
    dist.reset()
    torch.cuda.synchronize()
    assert float(dist.gust.abs().sum()) == 0.0 and int(dist.tick.abs().sum()) == 0


# ---- the chain in a graph ----
WEIGHTS = (15.0, 3.0, 80.0, 15.0, 0.0)


def test_g_field_step_update_and_force_callback_replayed_from_a_hipgraph_equal_eager_launches(vfx):
    """Captured once on one stream with the default queue count; replayed with new cmd / kind / f_true contents.  The disturbance's own
    state (tick, gust) lives on the device and moves on from replay to replay as it does from launch to launch."""
    import torch
    idx = np.nonzero(vfx["n_sub"] == 4)[0]
    tile = idx[np.arange(B) % len(idx)]
    rounds = [tile, tile[::-1].copy(), np.roll(tile, 5)]
    zones = _zones_for(vfx["x0"][tile])

    def make():
        fleet = solver.DeviceFleet(B, 20, 30, 64, L.MODEL_NORMAL, WEIGHTS, weights_final=WEIGHTS)
        fsm = solver.FleetFSM(fleet)
        veh = solver.Vehicle(fleet, n_sub=4, trace=True, **SCALARS)
        est = solver.ForceEstimator(veh, tau=0.01, min_samples=2, residual=True)
        dist = solver.Disturbance(veh, zones=zones, events=_events(B), gust_sigma=0.2, gust_tau=0.5, seed=3)
        cmds = solver.Commands(torch.zeros((B, 5, 16), dtype=torch.float64, device=DEV), torch.zeros((B, 5), dtype=torch.int32, device=DEV), None, None, None)
        return fsm, veh, est, dist, cmds

    def chain(fsm, veh, est, dist, cmds, stream=None):
        veh.step(cmds, stream)
        fsm.force(est.force, est.fresh, stream)

    def run(fsm, veh, est, dist, cmds, fn):
        veh.reset(_dev(vfx["x0"][rounds[0]], np.float64)); veh.hold.copy_(_dev(vfx["hold0"][rounds[0]], np.float64))       # (estimator and disturbance with it)
        fsm.consider_force.fill_(1); fsm.have_target.fill_(1); fsm.state.fill_(solver.FSM_EXEC_TRAJ)
        for n in ("external_acc", "last_external_acc", "surpass_count", "replan_force_surpass"):
            getattr(fsm, n).zero_()
        res = []
        for c in rounds:
            cmds.cmd.copy_(_dev(vfx["cmd"][c], np.float64)); cmds.kind.copy_(_dev(vfx["kind"][c], np.int32)); veh.f_true.copy_(_dev(vfx["f_true"][c], np.float64))
            fn()
            torch.cuda.synchronize()
            res.append([t.clone() for t in (veh.x, veh.hold, veh.trace, veh.sat, dist.force, dist.gust, dist.tick, est.thrust, est.f_hat, est.force, est.fresh,
                                            fsm.external_acc, fsm.surpass_count, fsm.state)])
        return res

    a = make()
    ref = run(*a, lambda: chain(*a))
    assert int(ref[-1][6].min()) == int(ref[-1][6].max()) == 15 and int(ref[-1][10].sum()) == B
    g_ = make()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        chain(*g_, side)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        chain(*g_, torch.cuda.current_stream())
    torch.cuda.synchronize()
    got = run(*g_, g.replay)
    view = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t
    for r, (p, q) in enumerate(zip(got, ref)):
        for i, (u, v) in enumerate(zip(p, q)):
            assert torch.equal(view(u), view(v)), (r, i)


# ---- the closed loop in one graph ----
from .test_gpu_estimator import FB, _layout                     # noqa: E402  (the estimator's 8-planner world: lanes along x, one pillar)
from . import estimator_oracle as EO                            # noqa: E402
from . import fsm_oracle as FO                                  # noqa: E402
from . import vehicle_oracle as VO                              # noqa: E402
from forces_resilient_planner_amd import workloads              # noqa: E402

PERIODS = 120
ZONE_PLANNER, EVENT_PLANNER = 1, 6
ZONE_F, EVENT_F = (1.5, 0.0, 0.0), (0.0, -1.8, 0.0)             # the estimator test's two force steps: max-norm above ext_noise_bound
# a slab across planner 1's lane (y = -6.55) from x = -5 on: it flies in through the face at x = -5 and up a 0.25 m ramp, and stays inside
LOOP_ZONE = [-5.0, -6.9, 0.0, 50.0, -6.2, 3.0, *ZONE_F, 0.25, 0.0, float("inf")]
EVENT_TICK = 100                                                # the event: planner 6, from sample 100 (period 20) on
RING_PRE = ("x", "hold", "consider_force", "have_target", "last_external_acc", "surpass_count", "state")


def _closed_loop(graph):
    """PERIODS periods of FleetFSM.period(force=est.force, force_fresh=est.fresh, vehicle=veh) with a Disturbance attached.  Period 0 runs
    eagerly in both modes (every lazy allocation happens there); with graph=True the period is then captured ONCE and replayed for periods
    1 ... PERIODS - 1 with new contents of clock and goal_fresh.  Inside the loop nothing is copied to the host: the rings are device
    tensors, filled by device-to-device copies between the periods and read back once after the loop."""
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
    est = solver.ForceEstimator(veh)
    events = np.tile(np.array([DC.UNUSED]), (FB, 1, 1))
    events[EVENT_PLANNER, 0] = [DC.t_of(EVENT_TICK, 0.0), np.inf, *EVENT_F]
    dist = solver.Disturbance(veh, zones=[LOOP_ZONE], events=events)
    start, goal = _layout()
    veh.reset(_dev(start, np.float64))                                           # (the estimator and the disturbance with it)
    veh.odometry(fsm)
    f64, i32 = dict(dtype=torch.float64, device=DEV), dict(dtype=torch.int32, device=DEV)
    d_goal, fresh_goal = _dev(goal, np.float64), torch.zeros((FB,), **i32)
    clock = torch.zeros((3,), **f64)
    post = dict(f_hat=est.f_hat, force=est.force, fresh=est.fresh, external_acc=fsm.external_acc, search=fsm.search, meas=est.meas, thrust=est.thrust, fsm=fsm.state,
                field=dist.force, tick=dist.tick, x_after=veh.x)
    pre = {n: getattr(veh if n in ("x", "hold") else fsm, n) for n in RING_PRE}
    ring = {n: torch.zeros((PERIODS,) + tuple(t.shape), dtype=t.dtype, device=DEV) for n, t in list(post.items()) + list(pre.items())}
    ring["cmd"], ring["kind"] = torch.zeros((PERIODS, FB, 5, 16), **f64), torch.zeros((PERIODS, FB, 5), **i32)
    ones, zeros = torch.ones((FB,), **i32), torch.zeros((FB,), **i32)
    clocks = [_dev(solver.FleetFSM.clock_for(0.05 * k, 1), np.float64) for k in range(PERIODS)]

    def period(stream=None):
        return fsm.period(pl, dm, None, clock, cloud, goal=d_goal, goal_fresh=fresh_goal, force=est.force, force_fresh=est.fresh, fsm_steps=1, vehicle=veh, stream=stream)

    g = None
    torch.cuda.synchronize()
    for k in range(PERIODS):                                                   # ---- nothing is copied to the host in here ----
        fresh_goal.copy_(ones if k == 0 else zeros)
        clock.copy_(clocks[k])
        for n, t in pre.items():
            ring[n][k].copy_(t)
        if g is None:
            cmds = period()
        else:
            g.replay()
        for n, t in post.items():
            ring[n][k].copy_(t)
        ring["cmd"][k].copy_(cmds.cmd); ring["kind"][k].copy_(cmds.kind)
        if graph and k == 0:
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                again = period(torch.cuda.current_stream())
            assert again.cmd.data_ptr() == cmds.cmd.data_ptr() and again.kind.data_ptr() == cmds.kind.data_ptr()
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    h = {n: t.cpu().numpy() for n, t in ring.items()}
    return h, dict(alpha=est.alpha, dt=est.dt, min_samples=est.min_samples, nb=fsm.ext_noise_bound, n_sub=veh.n_sub, mass=veh.mass, g=veh.g, kp=veh.kp, kv=veh.kv, ka=veh.ka,
                   events=events)


def test_h_a_zone_and_an_event_close_the_force_loop_in_one_replayed_graph(golden_dir, vfx):
    """The estimator's 8-planner world with its hand-switched force steps replaced by a zone across planner 1's route and an event on planner
    6.  (1) The period captured once and replayed equals the eager run bit for bit, every ring.  (2) The oracle chain per period, from the
    state, hold and commands the device held before it: disturbance_oracle + vehicle_oracle (disturbance_oracle.fly) give the force of every
    sample TO THE BIT (no gusts: IEEE operations alone) and the trace within the vehicle's bound; estimator_oracle on that trace and its
    thrusts gives force / fresh; fsm_oracle's force callback on them says in which period the planner hears a loud force and replans -- and
    the device replans in that period.  (3) Inside the zone the estimate ends within ext_noise_bound of the zone's force (the bound of
    test_gpu_estimator's loop test).
    Bounds.  Trace: the vehicle fixture's, tol_factor x max tol_case, scaled by max(1, largest |state| here / largest |state| there): the
    rounding error of S x n_sub Heun steps is a number of units in the last place of the state.  Chained force: the estimator fixture's bound
    plus 2 x trace bound / dt: the residual divides a difference of two velocities by dt, and the filter is a convex combination."""
    import torch
    eager, par = _closed_loop(False)
    replay, _ = _closed_loop(True)
    for n in eager:                                                               # (1)
        a, b = eager[n], replay[n]
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), n
    h = eager
    assert np.all(np.isfinite(h["meas"])) and np.all(np.isfinite(h["thrust"])) and np.all(h["tick"] == 5 * (np.arange(PERIODS)[:, None] + 1))
    efx = np.load(os.path.join(golden_dir, "estimator_mp.npz"))
    scale = max(1.0, float(np.abs(h["meas"]).max()) / float(np.abs(vfx["trace"][..., 0]).max()))
    b_trace = float(vfx["tol_factor"].reshape(-1)[0]) * float(np.max(vfx["tol_case"])) * scale
    b_force = float(efx["tol_factor"].reshape(-1)[0]) * float(np.max(efx["tol_case"])) + 2.0 * b_trace / par["dt"]
    kw = dict(mass=par["mass"], g=par["g"], dt_cmd=par["dt"], n_sub=par["n_sub"], kp=par["kp"], kv=par["kv"], ka=par["ka"])
    ctl = {k: kw[k] for k in ("mass", "g", "kp", "kv", "ka")}
    worst_t = worst_f = 0.0
    heard = {}
    weights = []
    for b in range(FB):                                                           # (2)
        count, y_prev = -1, [0.0] * 9
        o_force, o_fresh = [0.0] * 3, 0
        for k in range(PERIODS):
            # the fsm oracle's force callback of period k hears what the chain left at the end of period k - 1
            p = FO.Planner(state=int(h["state"][k, b]), consider_force=int(h["consider_force"][k, b]), have_target=int(h["have_target"][k, b]),
                           last_external_acc=list(h["last_external_acc"][k, b]), surpass_count=int(h["surpass_count"][k, b]))
            p.force(o_force, o_fresh, par["nb"])
            if "force:replan" in p.met and b not in heard:
                heard[b] = k
            loud = bool(p.met & {"force:loud_changed", "force:loud_steady"})       # what the callback left in external_acc: the force, or zero
            if loud or "force:quiet" in p.met:                                    # (a callback that returns early leaves external_acc as it was)
                assert loud == bool(np.any(h["external_acc"][k, b] != 0.0)), (b, k, p.met)
            if o_fresh and int(h["consider_force"][k, b]):                        # the decision is not a coin toss: the norm is off the threshold by more than the chain's error
                assert abs(FO.max_abs3(*o_force) - par["nb"]) > b_force, (b, k, o_force)
            x0, hold0 = list(h["x"][k, b]), list(h["hold"][k, b])
            _, _, trace, _, forces, _, tick = DO.fly(x0, hold0, [0.0] * 3, h["cmd"][k, b], h["kind"][k, b], 5 * k, b, [LOOP_ZONE], par["events"][b], None, None, None, 0, 0, 0.0, **kw)
            assert np.array_equal(_bits(forces), _bits(h["field"][k, b])), (b, k)     # the force each sample flew under, to the bit
            worst_t = max(worst_t, float(np.abs(np.array(trace) - h["meas"][k, b]).max()))
            if b == ZONE_PLANNER:
                before = [x0] + trace[:-1]
                weights += [DO.zone_weight(LOOP_ZONE, q[0:3], DC.t_of(5 * k + s, 0.0))[0] for s, q in enumerate(before)]
            thrust = EO.thrusts(x0, hold0, h["cmd"][k, b], h["kind"][k, b], trace, **ctl)
            f0 = h["f_hat"][k - 1, b] if k else [0.0] * 3
            _, y_prev, count, o_force, o_fresh, _, _ = EO.update(trace, thrust, f0, y_prev, count, par["dt"], par["alpha"], par["min_samples"])
            worst_f = max(worst_f, float(np.abs(np.array(o_force) - h["force"][k, b]).max()))
            assert o_fresh == h["fresh"][k, b]
            y_prev = list(h["meas"][k, b, -1])                                    # (the next call starts from the measurement the device kept)
    print("oracle chain over %d periods: trace worst %.3e (bound %.3e), chained force worst %.3e (bound %.3e)" % (PERIODS, worst_t, b_trace, worst_f, b_force))
    assert worst_t <= b_trace and worst_f <= b_force
    # the vehicle crossed the face and the ramp: no weight, a ramp value and full weight were flown
    weights = np.array(weights)
    assert np.any(weights == 0.0) and np.any((weights > 0.0) & (weights < 1.0)) and np.any(weights == 1.0) and weights[-1] == 1.0
    enter = int(np.argmax(np.any(h["field"][:, ZONE_PLANNER].reshape(PERIODS, -1) != 0.0, axis=1)))
    assert set(heard) == {ZONE_PLANNER, EVENT_PLANNER}, heard
    for b in (ZONE_PLANNER, EVENT_PLANNER):
        # the device replans on a force where its callback takes the loud-and-changed branch: last_external_acc, which the next period's
        # ring shows, becomes the loud force (a quiet force stores a quiet one there, a loud steady one leaves it)
        last = np.max(np.abs(h["last_external_acc"][1:, b]), axis=1)
        first = int(np.argmax(last > par["nb"]))
        since = enter if b == ZONE_PLANNER else EVENT_TICK // 5
        print("planner %d: the force acts from period %d, the device replans on it in period %d, the oracle chain says %d" % (b, since, first, heard[b]))
        assert last[first] > par["nb"] and first == heard[b] > since and h["search"][first, b] == 1 and h["state"][first, b] == solver.FSM_EXEC_TRAJ
        assert np.array_equal(_bits(h["external_acc"][first, b]), _bits(h["force"][first - 1, b]))
        assert np.array_equal(_bits(h["last_external_acc"][first + 1, b]), _bits(h["force"][first - 1, b]))
    free = np.array([b not in heard for b in range(FB)])
    assert np.all(h["external_acc"][:, free] == 0.0) and np.all(h["field"][:, free] == 0.0)
    # (3)
    err = np.max(np.abs(h["f_hat"][-1] - h["field"][-1, :, -1]), axis=1)
    print("|f_hat - force|_inf at the end:", ["%.3e" % v for v in err])
    assert np.all(err < par["nb"]) and np.array_equal(h["field"][-1, ZONE_PLANNER, -1], np.array(ZONE_F)) and np.array_equal(h["field"][-1, EVENT_PLANNER, -1], np.array(EVENT_F))
