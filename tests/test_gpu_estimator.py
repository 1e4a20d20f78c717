"""GPU tests of the force estimator (include/frp_nmpc_estimator.h, csrc/frp_estimator.hip, solver.ForceEstimator): the observed step against the
plain one and the controller's thrust, the update against the 50-digit scheme of tests/golden/estimator_mp.npz tiled over one full workgroup
plus one lane, one S = 5 call against five S = 1 calls, the masks among NaN-poisoned neighbours, observed step -> update -> force callback
replayed from a hipGraph, and FleetFSM.period(force=est.force, force_fresh=est.fresh, vehicle=veh) closing the loop on a map with nothing
copied to the host inside it.

The parity bound is test_gpu_vehicle's rule: 8 times the error of tests/estimator_oracle.py on the same case (tol_case, which the generator
keeps at or above one unit in the last place of the quantities compared) -- it covers the device's sincos, within an ulp or so of libm's;
every other operation of the update is an IEEE one."""
import math
import os
import types

import numpy as np
import pytest

from forces_resilient_planner_amd import layout as L, solver, workloads

from . import estimator_cases as EC
from . import estimator_oracle as EO
from . import vehicle_cases as VC
from . import vehicle_oracle as VO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, S = 257, VC.S
SCALARS = dict(mass=VC.MASS, g=VC.G, dt_cmd=VC.DT_CMD, **VC.GAINS)
CTL = dict(mass=VC.MASS, g=VC.G, **VC.GAINS)


@pytest.fixture(scope="module")
def vfx(golden_dir):
    return np.load(os.path.join(golden_dir, "vehicle_mp.npz"))


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "estimator_mp.npz"))


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _err(got, pair):
    got = np.asarray(got, dtype=np.float64)
    return np.abs((got - pair[..., 0]) - pair[..., 1])


def _vehicle(n, n_sub=4, trace=True, S_=S):
    """A solver.Vehicle for n vehicles without a fleet behind it (the class reads the fleet's size and device alone)."""
    import torch
    fleet = types.SimpleNamespace(torch=torch, B=n, solver=types.SimpleNamespace(device=torch.device(DEV)))
    return solver.Vehicle(fleet, n_sub=n_sub, trace=trace, S=S_, **SCALARS)


def _load(veh, vfx, c, S_=S):
    veh.x.copy_(_dev(vfx["x0"][c], np.float64)); veh.hold.copy_(_dev(vfx["hold0"][c], np.float64)); veh.f_true.copy_(_dev(vfx["f_true"][c], np.float64))
    return solver.Commands(_dev(vfx["cmd"][c][:, :S_], np.float64), _dev(vfx["kind"][c][:, :S_], np.int32), None, None, None)


# ---- the observed step ----
@pytest.mark.parametrize("n_sub,S_", [(1, 5), (4, 5), (4, 1)])
def test_a_observed_step_flies_the_plain_steps_flight_and_stores_the_controllers_thrust(vfx, n_sub, S_):
    import torch
    idx = np.nonzero(vfx["n_sub"] == n_sub)[0]
    c = idx[np.arange(B) % len(idx)]
    plain, obs = _vehicle(B, n_sub, S_=S_), _vehicle(B, n_sub, S_=S_)
    est = solver.ForceEstimator(obs)
    est.thrust.fill_(float("nan"))
    plain.step(_load(plain, vfx, c, S_)); obs.step(_load(obs, vfx, c, S_))
    torch.cuda.synchronize()
    for n in ("x", "hold", "trace"):
        assert np.array_equal(_bits(getattr(plain, n).cpu().numpy()), _bits(getattr(obs, n).cpu().numpy())), n
    assert torch.equal(plain.sat, obs.sat) and int((obs.sat & (VO.SAT_THRUST_LO | VO.SAT_THRUST_HI)).ne(0).sum()) > 0
    thrust, trace = est.thrust.cpu().numpy(), obs.trace.cpu().numpy()
    # vehicle_oracle.control on the device's own state and hold before every sample: products, sums, one sqrt and a clamp -- IEEE
    # operations alone reach T (the attitude branch with its asin and atan2 does not), so the device's double is the oracle's
    want = np.array([EO.thrusts(vfx["x0"][c[b]], vfx["hold0"][c[b]], vfx["cmd"][c[b]][:S_], vfx["kind"][c[b]][:S_], trace[b], **CTL) for b in range(B)])
    assert np.array_equal(_bits(thrust), _bits(want)), float(np.max(np.abs(thrust - want)))
    sat = obs.sat.cpu().numpy()
    assert np.all(thrust[(sat & VO.SAT_THRUST_LO) != 0] == VO.THRUST_LO) and np.all(thrust[(sat & VO.SAT_THRUST_HI) != 0] == VO.THRUST_HI)
    # the update ran behind the step: a first measurement and S - 1 residuals
    assert np.all(est.count.cpu().numpy() == S_ - 1) and np.array_equal(_bits(est.y_prev.cpu().numpy()), _bits(trace[:, -1]))


# ---- the update against the fixture ----
def _estimator(n, S_, alpha, residual=True):
    est = solver.ForceEstimator(_vehicle(n, trace=False, S_=S_), min_samples=EC.MIN_SAMPLES, residual=residual)
    est.alpha = float(alpha)
    return est


def _feed(est, fx, c):
    S_ = est.S
    est.meas.copy_(_dev(fx["meas"][c][:, :S_], np.float64)); est.thrust.copy_(_dev(fx["thrust"][c][:, :S_], np.float64))
    est.f_hat.copy_(_dev(fx["f_hat0"][c], np.float64)); est.y_prev.copy_(_dev(fx["y_prev0"][c], np.float64)); est.count.copy_(_dev(fx["count0"][c], np.int32))


def _host(est):
    return {n: getattr(est, n).cpu().numpy() for n in ("f_hat", "y_prev", "count", "force", "fresh", "residual", "status")}


@pytest.fixture(scope="module")
def updated(fx):
    """Every (alpha, S) of the fixture run once over its cases tiled over B estimators: {(alpha, S): (case index [B], outputs)}, shared."""
    import torch
    out = {}
    for alpha in EC.ALPHAS:
        for S_ in (1, 5):
            idx = np.nonzero((fx["alpha"] == alpha) & (fx["S"] == S_))[0]
            c = idx[np.arange(B) % len(idx)]
            est = _estimator(B, S_, alpha)
            _feed(est, fx, c)
            est.force.fill_(7.0); est.fresh.fill_(7); est.residual.fill_(7.0); est.status.fill_(7)
            est.update()
            torch.cuda.synchronize()
            out[(alpha, S_)] = (c, _host(est))
    return out


@pytest.mark.parametrize("alpha", EC.ALPHAS)
@pytest.mark.parametrize("S_", [5, 1])
def test_b_update_against_the_scheme_in_50_digits(fx, updated, alpha, S_):
    c, o = updated[(alpha, S_)]
    bound = float(fx["tol_factor"].reshape(-1)[0]) * fx["tol_case"][c]
    e = np.maximum(np.maximum(_err(o["f_hat"], fx["f_hat"][c]).max(axis=1), _err(o["force"], fx["force"][c]).max(axis=1)),
                   _err(o["residual"], fx["residual"][c][:, :S_]).reshape(B, -1).max(axis=1))
    worst = int(np.argmax(e / bound))
    print("alpha = %.4f, S = %d: worst error over bound %.3f (estimator %d, case %d: %.3e against %.3e)" % (alpha, S_, e[worst] / bound[worst], worst, c[worst], e[worst], bound[worst]))
    assert np.all(e <= bound), (worst, int(c[worst]), e[worst], bound[worst])
    # exact: the measurement kept, the counter, the flag, what every sample did, force = f_hat; the copies of a case agree to the bit
    assert np.array_equal(_bits(o["y_prev"]), _bits(fx["y_prev"][c])) and np.array_equal(o["count"], fx["count"][c]) and np.array_equal(o["fresh"], fx["fresh"][c])
    assert np.array_equal(o["status"], fx["status"][c][:, :S_]) and np.array_equal(_bits(o["force"]), _bits(o["f_hat"]))
    n = len(np.unique(c))
    for k in ("f_hat", "residual"):
        assert np.array_equal(_bits(o[k][n:]), _bits(o[k][:B - n])), k
    # a skipped sample leaves the estimate to the bit, forms no residual; a first one too
    idle = np.all(o["status"] != EC.ABSORBED, axis=1)
    if S_ == 1:
        assert idle.sum() >= 2 * (B // n)
    assert np.array_equal(_bits(o["f_hat"][idle]), _bits(fx["f_hat0"][c][idle]))
    assert np.all(o["residual"][o["status"] != EC.ABSORBED] == 0.0)


@pytest.mark.parametrize("alpha", EC.ALPHAS)
def test_c_one_call_of_five_samples_equals_five_calls_of_one(fx, updated, alpha):
    import torch
    c, o = updated[(alpha, 5)]
    one = _estimator(B, 1, alpha)
    _feed(one, fx, c)                                                            # (sample 0's rows; f_hat0, y_prev0, count0)
    meas, thrust = _dev(fx["meas"][c], np.float64), _dev(fx["thrust"][c], np.float64)
    for s in range(5):
        one.update(meas=meas[:, s:s + 1].contiguous(), thrust=thrust[:, s:s + 1].contiguous())
        torch.cuda.synchronize()
        h = _host(one)
        assert np.array_equal(_bits(h["residual"][:, 0]), _bits(o["residual"][:, s])) and np.array_equal(h["status"][:, 0], o["status"][:, s]), s
    for k in ("f_hat", "y_prev", "force"):
        assert np.array_equal(_bits(h[k]), _bits(o[k])), k
    assert np.array_equal(h["count"], o["count"]) and np.array_equal(h["fresh"], o["fresh"])
    # and without the optional outputs the estimate is the same
    bare = _estimator(B, 5, alpha, residual=False)
    _feed(bare, fx, c)
    bare.update()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(bare.f_hat.cpu().numpy()), _bits(o["f_hat"])) and np.array_equal(bare.count.cpu().numpy(), o["count"])


def test_d_masks_among_nan_poisoned_neighbours(fx, updated):
    import torch
    alpha = EC.ALPHAS[1]
    c, o = updated[(alpha, 5)]
    # every other estimator is fed NaNs alone: it skips, keeps its estimate to the bit, and its neighbours compute what they computed
    est = _estimator(B, 5, alpha)
    _feed(est, fx, c)
    odd = np.arange(B) % 2 == 1
    est.meas[_dev(odd, np.bool_)] = float("nan")
    est.update()
    torch.cuda.synchronize()
    h = _host(est)
    for k in ("f_hat", "y_prev", "force", "residual"):
        assert np.array_equal(_bits(h[k][~odd]), _bits(o[k][~odd])), k
    assert np.array_equal(h["count"][~odd], o["count"][~odd]) and np.array_equal(h["status"][~odd], o["status"][~odd])
    assert np.array_equal(_bits(h["f_hat"][odd]), _bits(fx["f_hat0"][c][odd])) and np.array_equal(_bits(h["y_prev"][odd]), _bits(fx["y_prev0"][c][odd]))
    assert np.all(h["count"][odd] == -1) and np.all(h["fresh"][odd] == 0) and np.all(h["status"][odd] == EC.SKIPPED) and np.all(h["residual"][odd] == 0.0)
    assert not np.any(np.isnan(h["f_hat"])) and not np.any(np.isnan(h["force"]))
    # the masked reset: the unmasked rows hold NaNs and odd counters, and keep every bit
    mask = (np.arange(B) % 3 == 0).astype(np.int32)
    m = mask != 0
    poison = lambda shape: np.where(m.reshape((-1,) + (1,) * (len(shape) - 1)), 3.25, np.nan) * np.ones(shape)
    est.f_hat.copy_(_dev(poison((B, 3)), np.float64)); est.force.copy_(_dev(poison((B, 3)), np.float64)); est.y_prev.copy_(_dev(poison((B, 9)), np.float64))
    est.count.fill_(41); est.fresh.fill_(1)
    keep = _host(est)
    est.vehicle.reset(torch.zeros((B, 9), dtype=torch.float64, device=DEV), _dev(mask, np.int32))      # Vehicle.reset resets it under the same mask
    torch.cuda.synchronize()
    h = _host(est)
    assert np.all(h["f_hat"][m] == 0.0) and np.all(h["force"][m] == 0.0) and np.all(h["count"][m] == -1) and np.all(h["fresh"][m] == 0)
    for k in ("f_hat", "force"):
        assert np.array_equal(_bits(h[k][~m]), _bits(keep[k][~m])), k
    assert np.array_equal(_bits(h["y_prev"]), _bits(keep["y_prev"])) and np.all(h["count"][~m] == 41) and np.all(h["fresh"][~m] == 1)
    assert np.array_equal(_bits(h["residual"]), _bits(keep["residual"])) and np.array_equal(h["status"], keep["status"])
    est.reset()                                                                  # no mask: everybody
    torch.cuda.synchronize()
    assert float(est.f_hat.abs().sum()) == 0.0 and float(est.force.abs().sum()) == 0.0 and int((est.count + 1).abs().sum()) == 0 and int(est.fresh.sum()) == 0


# ---- the chain in a graph ----
WEIGHTS = (15.0, 3.0, 80.0, 15.0, 0.0)


def test_e_observed_step_update_and_force_callback_replayed_from_a_hipgraph_equal_eager_launches(vfx):
    """Captured once on one stream with the default queue count; replayed with new cmd / kind / f_true contents."""
    import torch
    idx = np.nonzero(vfx["n_sub"] == 4)[0]
    tile = idx[np.arange(B) % len(idx)]
    rounds = [tile, tile[::-1].copy(), np.roll(tile, 5)]

    def make():
        fleet = solver.DeviceFleet(B, 20, 30, 64, L.MODEL_NORMAL, WEIGHTS, weights_final=WEIGHTS)
        fsm = solver.FleetFSM(fleet)
        veh = solver.Vehicle(fleet, n_sub=4, trace=True, **SCALARS)
        est = solver.ForceEstimator(veh, tau=0.01, min_samples=2, residual=True)
        cmds = solver.Commands(torch.zeros((B, S, 16), dtype=torch.float64, device=DEV), torch.zeros((B, S), dtype=torch.int32, device=DEV), None, None, None)
        return fsm, veh, est, cmds

    def chain(fsm, veh, est, cmds, stream=None):
        veh.step(cmds, stream)
        fsm.force(est.force, est.fresh, stream)

    def run(fsm, veh, est, cmds, fn):
        veh.reset(_dev(vfx["x0"][rounds[0]], np.float64)); veh.hold.copy_(_dev(vfx["hold0"][rounds[0]], np.float64))
        fsm.consider_force.fill_(1); fsm.have_target.fill_(1); fsm.state.fill_(solver.FSM_EXEC_TRAJ)
        for n in ("external_acc", "last_external_acc", "surpass_count", "replan_force_surpass"):
            getattr(fsm, n).zero_()
        res = []
        for c in rounds:
            cmds.cmd.copy_(_dev(vfx["cmd"][c], np.float64)); cmds.kind.copy_(_dev(vfx["kind"][c], np.int32)); veh.f_true.copy_(_dev(vfx["f_true"][c], np.float64))
            fn()
            torch.cuda.synchronize()
            res.append([t.clone() for t in (veh.x, veh.hold, veh.trace, veh.sat, est.thrust, est.f_hat, est.y_prev, est.count, est.force, est.fresh, est.residual,
                                            est.status, fsm.external_acc, fsm.last_external_acc, fsm.surpass_count, fsm.replan_force_surpass, fsm.state)])
        return res

    a = make()
    ref = run(*a, lambda: chain(*a))
    assert int(ref[-1][9].sum()) == B and int((ref[-1][12].abs().amax(dim=1) > 0).sum()) > B // 4 and int((ref[-1][16] == solver.FSM_REPLAN_TRAJ).sum()) > 0
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


# ---- FleetFSM.period with the estimate as the force callback's message ----
FB = 8
PERIODS = 120
FORCE_AT = 20
FORCED = {1: (1.5, 0.0, 0.0), 6: (0.0, -1.8, 0.0)}             # force steps with max-norm above ext_noise_bound, on two planners in flight
LANES = np.array([-8.05, -6.55, -5.05, -3.55, -2.05, 2.05, 3.55])


def _layout():
    """Seven planners fly 3 m along x in lanes of their own, planner 7 flies 5 m past the pillar at the origin."""
    start = np.zeros((FB, 9)); goal = np.zeros((FB, 3))
    start[:7, 0] = -6.05; start[:7, 1] = LANES; goal[:7, 0] = -3.05; goal[:7, 1] = LANES
    start[7, 0:2] = (-2.55, 0.05); goal[7, 0:2] = (2.55, 0.05)
    start[:, 2] = 1.2; goal[:, 2] = 1.2
    d = goal[:, 0:2] - start[:, 0:2]
    start[:, 8] = np.arctan2(d[:, 1], d[:, 0])
    return start, goal


def test_f_the_estimate_closes_the_force_loop_on_the_device(fx):
    """FleetFSM.period(force=est.force, force_fresh=est.fresh, vehicle=veh) for PERIODS periods; inside the loop the host writes the period's
    messages, clock and true force and reads nothing; every period's f_hat, force, fresh, external_acc, search, measurements and thrusts go
    into preallocated device rings, read back once after the loop.  The force callback of period p hears what period p - 1 left.
    Measured on an MI355X: the oracle reproduces every period's force to 3.9e-16 (bound 4.1e-14); both forced planners hear a loud force in
    period 21, the oracle's and the analytic one; |f_hat - f_true|_inf at the end is 8.1e-5 at worst over the eight planners (2.4e-8 for
    the unforced ones; bound: ext_noise_bound = 0.5)."""
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
    start, goal = _layout()
    veh.reset(_dev(start, np.float64))                                           # (the estimator with it)
    veh.odometry(fsm)
    f64, i32 = dict(dtype=torch.float64, device=DEV), dict(dtype=torch.int32, device=DEV)
    d_goal, fresh_goal = _dev(goal, np.float64), torch.zeros((FB,), **i32)
    clock = torch.zeros((3,), **f64)
    ring = dict(f_hat=torch.zeros((PERIODS, FB, 3), **f64), force=torch.zeros((PERIODS, FB, 3), **f64), fresh=torch.zeros((PERIODS, FB), **i32),
                external_acc=torch.zeros((PERIODS, FB, 3), **f64), search=torch.zeros((PERIODS, FB), **i32), meas=torch.zeros((PERIODS, FB, S, 9), **f64),
                thrust=torch.zeros((PERIODS, FB, S), **f64), fsm=torch.zeros((PERIODS, FB), **i32), consider=torch.zeros((PERIODS, FB), **i32))
    f_step = np.zeros((FB, 3))
    for b, f in FORCED.items():
        f_step[b] = f
    d_step, ones, zeros = _dev(f_step, np.float64), torch.ones((FB,), **i32), torch.zeros((FB,), **i32)
    clocks = [_dev(solver.FleetFSM.clock_for(0.05 * k, 1), np.float64) for k in range(PERIODS)]
    torch.cuda.synchronize()
    for k in range(PERIODS):                                                   # ---- nothing is copied to the host in here ----
        fresh_goal.copy_(ones if k == 0 else zeros)
        if k == FORCE_AT:
            veh.f_true.copy_(d_step)
        clock.copy_(clocks[k])
        ring["consider"][k].copy_(fsm.consider_force)
        fsm.period(pl, dm, None, clock, cloud, goal=d_goal, goal_fresh=fresh_goal, force=est.force, force_fresh=est.fresh, fsm_steps=1, vehicle=veh)
        for n, t in (("f_hat", est.f_hat), ("force", est.force), ("fresh", est.fresh), ("external_acc", fsm.external_acc), ("search", fsm.search),
                     ("meas", est.meas), ("thrust", est.thrust), ("fsm", fsm.state)):
            ring[n][k].copy_(t)
    torch.cuda.synchronize()
    h = {n: t.cpu().numpy() for n, t in ring.items()}
    assert np.all(np.isfinite(h["meas"])) and np.all(np.isfinite(h["thrust"]))
    # the oracle replays the estimator period by period, each call from the estimate the device held before it (one call's bound)
    alpha, dt, ms = est.alpha, est.dt, est.min_samples
    bound = float(fx["tol_factor"].reshape(-1)[0]) * float(np.max(fx["tol_case"]))
    o_force, o_fresh = np.zeros((PERIODS, FB, 3)), np.zeros((PERIODS, FB), dtype=np.int32)
    worst = 0.0
    for b in range(FB):
        count, y_prev = -1, [0.0] * 9
        for k in range(PERIODS):
            f0 = h["f_hat"][k - 1, b] if k else [0.0] * 3
            _, y_prev, count, force, fresh, _, _ = EO.update(h["meas"][k, b], h["thrust"][k, b], f0, y_prev, count, dt, alpha, ms)
            o_force[k, b], o_fresh[k, b] = force, fresh
            assert count == 5 * (k + 1) - 1
    worst = float(np.max(np.abs(o_force - h["force"])))
    print("oracle against the device's force over %d periods: worst %.3e, bound %.3e (ratio %.3f)" % (PERIODS, worst, bound, worst / bound))
    assert worst <= bound and np.array_equal(o_fresh, h["fresh"]) and np.array_equal(_bits(h["force"]), _bits(h["f_hat"]))
    assert np.all(h["fresh"][:1] == 0) and np.all(h["fresh"][2:] == 1)                     # min_samples = 10: after two periods
    # when the planner first hears a loud force: the oracle's period, the analytic one, and a search in it
    nb = fsm.ext_noise_bound
    loud = lambda f: max(max(abs(f[0]), abs(f[1])), abs(f[2])) > nb
    for b, f in FORCED.items():
        assert h["fsm"][FORCE_AT - 1, b] == solver.FSM_EXEC_TRAJ and np.all(h["consider"][FORCE_AT:FORCE_AT + 4, b] == 1), b
        first = int(np.argmax(np.any(h["external_acc"][:, b] != 0.0, axis=1)))
        want = next(k for k in range(1, PERIODS) if o_fresh[k - 1, b] and loud(o_force[k - 1, b]))      # period k hears what k - 1 left
        n_samples = math.ceil(math.log(1.0 - nb / max(abs(v) for v in f)) / math.log(1.0 - alpha))
        analytic = FORCE_AT + n_samples / S                                       # in periods: the step acts from period FORCE_AT's samples on
        print("planner %d: external_acc first non-zero in period %d, the oracle's %d, analytic %d samples = period %.2f" % (b, first, want, n_samples, analytic))
        assert first == want and np.any(h["external_acc"][first, b] != 0.0) and abs(first - analytic) <= 1.0, (b, first, want, analytic)
        assert h["search"][first, b] == 1 and np.array_equal(_bits(h["external_acc"][first, b]), _bits(h["force"][first - 1, b]))
    free = np.array([b not in FORCED for b in range(FB)])
    assert np.all(h["external_acc"][:, free] == 0.0)
    err = np.max(np.abs(h["f_hat"][-1] - f_step), axis=1)
    print("|f_hat - f_true|_inf at the end:", ["%.3e" % v for v in err])
    assert np.all(err < nb)
