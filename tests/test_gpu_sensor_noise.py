"""GPU tests of the sensor noise (include/frp_nmpc.h section 16, csrc/frp_sensor_noise.hip, solver.SensorNoise): the three entry points
against the 50-digit fixture tests/golden/sensor_noise_mp.npz (states and scan points within 8 times the error of
tests/sensor_noise_oracle.py on the same case -- the project's rule for the gust draws: it covers the device's log and cos against libm's
--, depth images EQUAL in every pixel, which tests/test_sensor_noise_cpu.py licenses by showing that the cases hold no near-tie), one S = 5
call against five S = 1 calls and a fleet against its halves (device against device, to the bit), zero noise as the identity -- in the
calls and in a closed loop --, noise that reaches the estimator of a closed loop as the oracle chain says, a captured step + depth chain
replayed against eager launches, and the argument rules.  Shapes: 67 vehicles (a partial wave, a partial workgroup), 37 x 53 pixels (eight
workgroups per frame, the last partial), 131 points."""
import ctypes
import os
import types

import numpy as np
import pytest

from forces_resilient_planner_amd import capi, layout as L, solver, workloads

from . import estimator_oracle as EO
from . import sensor_noise_cases as NC
from . import sensor_noise_oracle as NO
from . import vehicle_cases as VC
from . import vehicle_oracle as VO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCALARS = dict(mass=VC.MASS, g=VC.G, dt_cmd=VC.DT_CMD, **VC.GAINS)
KW = dict(sigma_p=NC.SIGMA_P, sigma_v=NC.SIGMA_V, sigma_a=NC.SIGMA_A, sigma_bias=NC.SIGMA_BIAS, tau_bias=NC.TAU_BIAS, depth=NC.DEPTH, scan=NC.SCAN, seed=NC.SEED)
ZERO = dict(seed=NC.SEED)                      # SENSOR_NOISE_DEFAULTS: every sigma and p_drop zero
M64 = 1 << 64


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "sensor_noise_mp.npz"))


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _u16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(DEV).view(torch.uint16)


def _host16(t):
    import torch
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _err(got, pair):
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.abs((got - pair[..., 0]) - pair[..., 1])


def _vehicle(n, S_=NC.S, trace=False):
    import torch
    fleet = types.SimpleNamespace(torch=torch, B=n, solver=types.SimpleNamespace(device=torch.device(DEV)))
    return solver.Vehicle(fleet, trace=trace, S=S_, **SCALARS)


def _noise(n=NC.B, S_=NC.S, first=0, F=None, **kw):
    """A SensorNoise on n vehicles loaded with the state case's lanes first ... first + n - 1 (id0 shifted by `first`)."""
    x, bias0, tick0 = NC.states_case()
    k = dict(KW, id0=NC.ID0 + first)
    k.update(kw)
    noise = solver.SensorNoise(_vehicle(n, S_), F=F, **k)
    noise.bias.copy_(_dev(bias0[first:first + n], np.float64)); noise.tick.copy_(_dev(tick0[first:first + n], np.int64))
    return noise, _dev(x[first:first + n, :S_], np.float64)


@pytest.fixture(scope="module")
def measured(fx):
    """The state case measured once with S = 5, advancing: (meas, y, bias, tick) on the host, shared."""
    import torch
    noise, x = _noise()
    assert list(noise.bias_a) + list(noise.bias_c) == list(fx["scalars"])
    m = noise.states(x)
    torch.cuda.synchronize()
    assert m is noise.meas
    return m.cpu().numpy(), noise.y.cpu().numpy(), noise.bias.cpu().numpy(), noise.tick.cpu().numpy()


def test_a_states_against_the_50_digit_fixture(fx, measured):
    import torch
    m, y, bias, tick = measured
    x = fx["states_x"]
    factor = float(fx["tol_factor"].reshape(-1)[0])
    want = fx["states_meas"]
    fin = np.isfinite(want[..., 0])
    # per component: 8 x the oracle's own error on that vehicle, and never below one ulp of the true value (the components of sigma 0)
    bound = np.maximum(factor * fx["states_tol_case"][:, None, None], np.where(np.isfinite(x), np.spacing(np.abs(x)), 0.0))
    e = np.where(fin, _err(m, want), 0.0)
    worst = np.unravel_index(int(np.argmax(e / bound)), e.shape)
    print("states: worst error over bound %.3f at %s (%.3e against %.3e)" % (e[worst] / bound[worst], worst, e[worst], bound[worst]))
    assert np.all(e <= bound), (worst, e[worst], bound[worst])
    eb = _err(bias, fx["states_bias"])
    assert np.all(eb <= factor * fx["states_tol_case"][:, None]), eb.max()
    # what is not finite passes through to the bit; the pitch (sigma 0) and the negative zeros are the truth to the bit
    assert np.array_equal(_bits(m[~np.isfinite(x)]), _bits(x[~np.isfinite(x)])) and np.all(np.isfinite(m[np.isfinite(x)]))
    assert np.array_equal(_bits(m[:, :, 7]), _bits(x[:, :, 7])) and not np.array_equal(_bits(m[:, :, 6]), _bits(x[:, :, 6]))
    assert np.array_equal(_bits(y), _bits(m[:, -1])) and np.array_equal(tick.view(np.uint64), fx["states_tick"])
    assert len(np.unique(_bits(m[:, 0, 3]))) == NC.B                                     # every lane draws its own stream
    # in place equals out of place, to the bit; a pure query leaves bias and tick
    noise, xd = _noise()
    b0, t0 = noise.bias.clone(), noise.tick.clone()
    q = noise.states(xd, advance=False, out=torch.empty_like(xd))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(q.cpu().numpy()), _bits(m)) and torch.equal(noise.bias.view(torch.int64), b0.view(torch.int64)) and torch.equal(noise.tick, t0)
    noise.states(xd, out=xd)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(xd.cpu().numpy()), _bits(m)) and np.array_equal(_bits(noise.bias.cpu().numpy()), _bits(bias))


def test_b_split_and_shard_device_against_device(measured):
    import torch
    m, y, bias, tick = measured
    noise, x = _noise(S_=1)
    xs = _dev(NC.states_case()[0], np.float64)
    for s in range(NC.S):
        ms = noise.states(xs[:, s:s + 1].contiguous())
        torch.cuda.synchronize()
        assert np.array_equal(_bits(ms.cpu().numpy()[:, 0]), _bits(m[:, s])), s
    assert np.array_equal(_bits(noise.bias.cpu().numpy()), _bits(bias)) and np.array_equal(noise.tick.cpu().numpy(), tick) and np.array_equal(_bits(noise.y.cpu().numpy()), _bits(y))
    for first, n in ((0, 33), (33, 34)):
        half, xh = _noise(n=n, first=first)
        mh = half.states(xh)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(mh.cpu().numpy()), _bits(m[first:first + n])) and np.array_equal(_bits(half.bias.cpu().numpy()), _bits(bias[first:first + n])), first


def test_c_depth_images_equal_the_oracles_in_every_pixel(fx):
    import torch
    noise = solver.SensorNoise(_vehicle(1), F=NC.F, **dict(KW, id0=NC.ID0))
    img, active = _u16(fx["depth_in"]), _dev(NC.DEPTH_ACTIVE, np.int32)
    out = _u16(np.full((NC.F, NC.ROWS, NC.COLS), 7, dtype=np.uint16))
    assert noise.depth(img, active=active, out=out) is out
    torch.cuda.synchronize()
    got = _host16(out)
    assert np.array_equal(got[0], fx["depth_out"][0][0]) and np.array_equal(got[2], fx["depth_out"][0][2]) and np.all(got[1] == 7)   # the inactive frame is not written
    assert np.array_equal(_host16(img), fx["depth_in"]) and noise.depth_tick.cpu().tolist() == [1, 0, 1]
    # the second call, in place on the first one's images: other draws, the oracle's at tick 1; the inactive frame's image and tick stay
    buf = _u16(fx["depth_out"][0])
    noise.depth(buf, active=active, out=buf)
    torch.cuda.synchronize()
    got2 = _host16(buf)
    assert np.array_equal(got2, fx["depth_out"][1]) and not np.array_equal(got2[0], got[0]) and np.array_equal(got2[1], fx["depth_in"][1])
    assert noise.depth_tick.cpu().tolist() == [2, 0, 2]
    # the case reaches what it was built for: pixels of 0, 1 and 65535, and pixels the noise took off either end of the uint16
    src, first = fx["depth_in"], fx["depth_out"][0]
    assert np.all(first[src == 0] == 0) and np.any(first[src == 1] == 0) and np.any(first[src == 1] > 0) and np.any(first[src == 65535] == 0) and np.any(first[src == 65535] > 0)


def test_d_scan_points_against_the_50_digit_fixture(fx):
    import torch
    noise = solver.SensorNoise(_vehicle(1), F=NC.SCANS, **dict(KW, id0=NC.ID0))
    pts, origin, count = _dev(fx["scan_in"], np.float64), _dev(fx["scan_origin"], np.float64), _dev(fx["scan_count"], np.int32)
    out = noise.scan(pts, origin, count=count)
    torch.cuda.synchronize()
    got, want = out.cpu().numpy(), fx["scan_out"]
    factor = float(fx["tol_factor"].reshape(-1)[0])
    assert np.array_equal(np.isnan(got), np.isnan(want[..., 0])) and np.array_equal(np.isinf(got), np.isinf(want[..., 0]))      # the NaN pattern is exact
    fin = np.isfinite(want[..., 0])
    e = np.where(fin, _err(got, want), 0.0).reshape(NC.SCANS, -1).max(axis=1)
    print("scan: error over bound", e / (factor * fx["scan_tol_case"]))
    assert np.all(e <= factor * fx["scan_tol_case"])
    lost = np.isnan(got).all(axis=2) & ~np.isnan(fx["scan_in"]).any(axis=2)
    assert lost.sum() > 5 and noise.scan_tick.cpu().tolist() == [1, 1] and np.array_equal(_bits(pts.cpu().numpy()), _bits(fx["scan_in"]))
    for s in range(NC.SCANS):                                                            # storage beyond count is untouched; the point at the origin stays
        assert np.array_equal(_bits(got[s, NC.COUNT[s]:]), _bits(fx["scan_in"][s, NC.COUNT[s]:])), s
    assert np.array_equal(_bits(got[1, 3]), _bits(fx["scan_origin"][1]))
    # in place, with the out-of-count storage poisoned: the same points, the poison kept
    noise2 = solver.SensorNoise(_vehicle(1), F=NC.SCANS, **dict(KW, id0=NC.ID0))
    buf = pts.clone()
    buf[1, NC.COUNT[1]:] = 7.0
    noise2.scan(buf, origin, count=count, out=buf)
    torch.cuda.synchronize()
    g2 = buf.cpu().numpy()
    assert np.array_equal(_bits(g2[0]), _bits(got[0])) and np.array_equal(_bits(g2[1, :NC.COUNT[1]]), _bits(got[1, :NC.COUNT[1]])) and np.all(g2[1, NC.COUNT[1]:] == 7.0)


def test_e_zero_noise_is_the_identity_to_the_bit(fx):
    import torch
    noise, x = _noise(F=NC.F, **dict(sigma_p=0.0, sigma_v=0.0, sigma_a=0.0, sigma_bias=0.0, depth=None, scan=None))
    noise.bias.zero_()
    m = noise.states(x)
    img = _u16(fx["depth_in"])
    d = noise.depth(img)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(m.cpu().numpy()), _bits(fx["states_x"])) and np.array_equal(_bits(noise.y.cpu().numpy()), _bits(fx["states_x"][:, -1]))
    assert np.array_equal(_host16(d), fx["depth_in"]) and noise.depth_tick.cpu().tolist() == [1, 1, 1]
    n2 = solver.SensorNoise(_vehicle(1), F=NC.SCANS, **ZERO)
    pts = _dev(fx["scan_in"], np.float64)
    o = n2.scan(pts, _dev(fx["scan_origin"], np.float64), count=_dev(fx["scan_count"], np.int32))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(o.cpu().numpy()), _bits(fx["scan_in"]))


# ---- the closed loop: test_gpu_disturbance's fleet, six planners in lanes of their own, 20 periods ----
from .test_gpu_estimator import _layout                     # noqa: E402
from .test_gpu_disturbance import WEIGHTS                   # noqa: E402

FB, PERIODS = 6, 20
LOOP_SIGMA_V = 0.05


def _camera(x, y, z):
    """A camera at (x, y, z) that looks along world +x: T_wc [4,4]."""
    T = np.eye(4)
    T[0:3, 0:3] = [[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]
    T[0:3, 3] = (x, y, z)
    return T


def _loop(noise_kw):
    """PERIODS periods of FleetFSM.period(force=est.force, force_fresh=est.fresh, vehicle=veh), eagerly, with a SensorNoise of noise_kw attached
    (None: none); the rings are device tensors read back once after the loop."""
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
    noise = solver.SensorNoise(veh, **noise_kw) if noise_kw is not None else None
    start, goal = (a[:FB] for a in _layout())
    veh.reset(_dev(start, np.float64))
    veh.odometry(fsm)
    f64, i32 = dict(dtype=torch.float64, device=DEV), dict(dtype=torch.int32, device=DEV)
    d_goal, fresh_goal = _dev(goal, np.float64), torch.zeros((FB,), **i32)
    clock = torch.zeros((3,), **f64)
    post = dict(x=veh.x, state=veh.state, f_hat=est.f_hat, force=est.force, fresh=est.fresh, trace=est.meas, thrust=est.thrust, fsm=fsm.state)
    pre = dict(x0=veh.x, hold0=veh.hold)
    if noise is not None:
        post.update(meas=noise.meas, y=noise.y)
        pre.update(bias0=noise.bias, tick0=noise.tick)
    ring = {n: torch.zeros((PERIODS,) + tuple(t.shape), dtype=t.dtype, device=DEV) for n, t in list(post.items()) + list(pre.items())}
    ring["cmd"], ring["kind"] = torch.zeros((PERIODS, FB, 5, 16), **f64), torch.zeros((PERIODS, FB, 5), **i32)
    ones, zeros = torch.ones((FB,), **i32), torch.zeros((FB,), **i32)
    clocks = [_dev(solver.FleetFSM.clock_for(0.05 * k, 1), np.float64) for k in range(PERIODS)]
    torch.cuda.synchronize()
    for k in range(PERIODS):
        fresh_goal.copy_(ones if k == 0 else zeros)
        clock.copy_(clocks[k])
        for n, t in pre.items():
            ring[n][k].copy_(t)
        cmds = fsm.period(pl, dm, None, clock, cloud, goal=d_goal, goal_fresh=fresh_goal, force=est.force, force_fresh=est.fresh, fsm_steps=1, vehicle=veh)
        for n, t in post.items():
            ring[n][k].copy_(t)
        ring["cmd"][k].copy_(cmds.cmd); ring["kind"][k].copy_(cmds.kind)
    torch.cuda.synchronize()
    h = {n: t.cpu().numpy() for n, t in ring.items()}
    h["map"] = dm.occ.cpu().numpy()
    par = dict(alpha=est.alpha, dt=est.dt, min_samples=est.min_samples, n_sub=veh.n_sub, mass=veh.mass, g=veh.g, kp=veh.kp, kv=veh.kv, ka=veh.ka)
    if noise is not None:
        par["noise"] = dict(seed=noise.seed, id0=noise.id0, sigma_p=noise.sigma_p, sigma_v=noise.sigma_v, sigma_a=noise.sigma_a, bias_a=noise.bias_a, bias_c=noise.bias_c)
    return h, par


@pytest.fixture(scope="module")
def plain_loop():
    return _loop(None)


def test_f_a_closed_loop_with_zero_noise_attached_is_the_loop_without_one(plain_loop):
    h0, _ = plain_loop
    h1, _ = _loop(ZERO)
    for n in ("x", "state", "f_hat", "force", "fresh", "trace", "thrust", "fsm", "cmd", "kind", "map"):
        a, b = h0[n], h1[n]
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), n
    assert np.array_equal(_bits(h1["meas"]), _bits(h1["trace"])) and np.array_equal(_bits(h1["y"]), _bits(h1["x"])) and np.all(h1["tick0"] == 5 * np.arange(PERIODS)[:, None])
    assert np.any(h0["fsm"] == solver.FSM_EXEC_TRAJ) and np.abs(h0["x"][-1] - h0["x0"][0]).max() > 0.1          # the fleet flew


def test_g_noise_reaches_the_estimator_of_the_loop_as_the_oracle_chain_says(golden_dir):
    """sigma_v > 0, zero true force.  Per period and planner, from what the device held before the period: tests/vehicle_oracle.py flies the
    commands, tests/sensor_noise_oracle.py measures that trace, tests/estimator_oracle.py absorbs the measurements with the oracle's
    thrusts -- and the force it leaves is the device's within test_gpu_estimator's own bound, tol_factor x max tol_case of estimator_mp.npz."""
    h, par = _loop(dict(sigma_v=LOOP_SIGMA_V, seed=11, id0=5))
    assert np.any(h["state"] != h["x"]) and np.array_equal(_bits(h["y"]), _bits(h["meas"][:, :, -1])) and not np.array_equal(_bits(h["meas"]), _bits(h["trace"]))
    assert np.array_equal(_bits(h["meas"][..., 0:3]), _bits(h["trace"][..., 0:3]))          # (the position and the angles have no noise here)
    assert np.all(np.any(h["f_hat"][-1] != 0.0, axis=1)) and np.all(np.isfinite(h["f_hat"]))
    efx = np.load(os.path.join(golden_dir, "estimator_mp.npz"))
    bound = float(efx["tol_factor"].reshape(-1)[0]) * float(np.max(efx["tol_case"]))
    kw = dict(mass=par["mass"], g=par["g"], dt_cmd=par["dt"], n_sub=par["n_sub"], kp=par["kp"], kv=par["kv"], ka=par["ka"])
    ctl = {k: kw[k] for k in ("mass", "g", "kp", "kv", "ka")}
    worst = worst_m = 0.0
    for b in range(FB):
        count, y_prev = -1, [0.0] * 9
        for k in range(PERIODS):
            x0, hold0 = list(h["x0"][k, b]), list(h["hold0"][k, b])
            _, _, trace, _ = VO.step(x0, hold0, [0.0] * 3, h["cmd"][k, b], h["kind"][k, b], **kw)
            meas, _, _, tick = NO.states(trace, h["bias0"][k, b], int(h["tick0"][k, b]), b, par["noise"])
            assert tick == 5 * (k + 1)
            worst_m = max(worst_m, float(np.abs(np.array(meas) - h["meas"][k, b]).max()))
            thrust = EO.thrusts(x0, hold0, h["cmd"][k, b], h["kind"][k, b], trace, **ctl)
            f0 = h["f_hat"][k - 1, b] if k else [0.0] * 3
            _, y_prev, count, force, fresh, _, _ = EO.update(meas, thrust, f0, y_prev, count, par["dt"], par["alpha"], par["min_samples"])
            worst = max(worst, float(np.abs(np.array(force) - h["force"][k, b]).max()))
            assert fresh == h["fresh"][k, b]
            y_prev = list(h["meas"][k, b, -1])                                           # (the next call starts from the measurement the device kept)
    print("oracle chain over %d periods: measurement worst %.3e, chained force worst %.3e (bound %.3e); |f_hat| at the end up to %.3e" % (PERIODS, worst_m, worst, bound, np.abs(h["f_hat"][-1]).max()))
    assert worst <= bound, (worst, bound)


def test_h_step_with_noise_and_depth_replayed_from_a_hipgraph_equal_eager_launches(golden_dir):
    """Vehicle.step with a SensorNoise and a ForceEstimator attached, then SensorNoise.depth on a frame set rendered from a map: captured
    once, replayed three times.  The counters are device memory, so every replay draws anew -- what the eager sequence draws at the same ticks."""
    import torch
    vfx = np.load(os.path.join(golden_dir, "vehicle_mp.npz"))
    idx = np.nonzero(vfx["n_sub"] == 4)[0]
    c = idx[np.arange(NC.B) % len(idx)]
    dm = solver.OccupancyMap(workloads.astar_world(0, "empty", allocate_num=12000))
    dm.insert_cloud(np.array([(x, y, z) for x in np.arange(-0.25, 0.26, 0.1) for y in np.arange(-0.25, 0.26, 0.1) for z in np.arange(-0.95, 2.96, 0.1)], dtype=np.float32))
    T = np.stack([_camera(-2.0, 0.0, 1.2), _camera(-3.0, 0.3, 1.0), _camera(-1.5, -0.2, 1.5)])
    K = [[40.0, 0.0, NC.COLS / 2.0], [0.0, 40.0, NC.ROWS / 2.0], [0.0, 0.0, 1.0]]
    frames = dm.render_depth(T, K, NC.ROWS, NC.COLS, max_range=5.0)
    torch.cuda.synchronize()
    assert int((frames.view(torch.int16) != 0).sum()) > 100                               # the cameras see the pillar

    def make():
        veh = _vehicle(NC.B, trace=True)
        est = solver.ForceEstimator(veh)
        noise = solver.SensorNoise(veh, F=NC.F, **KW)
        veh.reset(_dev(vfx["x0"][c], np.float64)); veh.hold.copy_(_dev(vfx["hold0"][c], np.float64))
        cmds = solver.Commands(_dev(vfx["cmd"][c], np.float64), _dev(vfx["kind"][c], np.int32), None, None, None)
        return veh, est, noise, cmds, torch.zeros(tuple(frames.shape), dtype=torch.int16, device=DEV).view(torch.uint16)

    def chain(veh, est, noise, cmds, noisy, stream=None):
        veh.step(cmds, stream)
        noise.depth(frames, out=noisy, stream=stream)

    def snap(veh, est, noise, cmds, noisy):
        torch.cuda.synchronize()
        return [t.clone() for t in (veh.x, veh.trace, noise.meas, noise.y, noise.bias, noise.tick, noise.depth_tick, est.f_hat, noisy.view(torch.int16))]

    a = make()
    ref = []
    for _ in range(4):
        chain(*a)
        ref.append(snap(*a))
    assert ref[-1][5].tolist() == [20] * NC.B and ref[-1][6].tolist() == [4] * NC.F and not torch.equal(ref[0][8], ref[1][8])
    g_ = make()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        chain(*g_, side)                                                                 # (call 1, eagerly: the capture itself runs nothing)
    side.synchronize()
    got = [snap(*g_)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        chain(*g_, torch.cuda.current_stream())
    torch.cuda.synchronize()
    for _ in range(3):
        g.replay()
        got.append(snap(*g_))
    view = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t
    for r, (p, q) in enumerate(zip(got, ref)):
        for i, (u, v) in enumerate(zip(p, q)):
            assert torch.equal(view(u), view(v)), (r, i)


def test_i_every_refusal_through_the_c_abi_and_through_python_launches_nothing(fx):
    import torch
    from .test_sensor_noise_cpu import refusals
    l = solver.lib()
    noise, x = _noise(F=NC.F)
    keep = [t.clone() for t in (noise.bias, noise.tick, noise.depth_tick, noise.scan_tick, noise.y, noise.meas)]
    for what, call, _ in refusals():
        assert call(l) == capi.FRP_ERR_ARG, what
    # the same rules on device pointers: a struct this object made, with one field out of its range
    img = _u16(fx["depth_in"])
    out16, outx = _u16(np.full((NC.F, NC.ROWS, NC.COLS), 7, dtype=np.uint16)), torch.full_like(x, 7.0)
    pts = _dev(np.ones((NC.F, 8, 3)), np.float64)
    outp = torch.full_like(pts, 7.0)
    origin = torch.zeros((NC.F, 3), dtype=torch.float64, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for field, bad in (("sigma_v", -1.0), ("sigma_p", float("nan")), ("depth_p_drop", 1.5), ("scan_p_drop", -0.1), ("depth_sigma2", float("inf")), ("B", 0)):
        n = noise.struct()
        if field in ("sigma_v", "sigma_p"):
            getattr(n, field)[0] = bad
        else:
            setattr(n, field, bad)
        r = ctypes.byref(n)
        assert l.frp_nmpc_sensor_noise_states(r, NC.S, p(x), p(outx), p(noise.y), 1, s) == capi.FRP_ERR_ARG, field
        assert l.frp_nmpc_sensor_noise_reset(r, None, p(x[:, 0].contiguous()), p(noise.y), s) == capi.FRP_ERR_ARG, field
        assert l.frp_nmpc_sensor_noise_depth(r, NC.F, NC.ROWS, NC.COLS, p(img), p(out16), None, p(noise.depth_tick), s) == capi.FRP_ERR_ARG, field
        assert l.frp_nmpc_sensor_noise_scan(r, NC.F, 8, p(pts), p(outp), p(origin), None, None, p(noise.scan_tick), s) == capi.FRP_ERR_ARG, field
    n = noise.struct()
    r = ctypes.byref(n)
    assert l.frp_nmpc_sensor_noise_states(r, 0, p(x), p(outx), p(noise.y), 1, s) == capi.FRP_ERR_ARG
    assert l.frp_nmpc_sensor_noise_depth(r, 0, NC.ROWS, NC.COLS, p(img), p(out16), None, p(noise.depth_tick), s) == capi.FRP_ERR_ARG
    assert l.frp_nmpc_sensor_noise_scan(r, 0, 8, p(pts), p(outp), p(origin), None, None, p(noise.scan_tick), s) == capi.FRP_ERR_ARG
    # Python: a ValueError with a message, before anything is made
    veh = noise.vehicle
    for kw in (dict(sigma_p=-0.1), dict(sigma_v=(0.1, float("nan"), 0.1)), dict(sigma_a=float("inf")), dict(sigma_bias=-1.0), dict(tau_bias=0.0), dict(depth=dict(p_drop=1.5)),
               dict(depth=dict(sigma0=-1.0)), dict(depth=dict(sigma2=float("nan"))), dict(scan=dict(p_drop=-0.5)), dict(scan=dict(sigma1=float("inf"))), dict(scan=dict(sigma9=1.0)),
               dict(depth=dict(depth_scale=0.0)), dict(F=0), dict(F=capi.SENSOR_NOISE_MAX_FRAMES + 1), dict(seed=2 ** 63)):
        with pytest.raises(ValueError, match="SensorNoise"):
            solver.SensorNoise(veh, **kw)
    assert veh.noise is noise                                                            # a refused constructor attaches nothing
    with pytest.raises(ValueError, match="SensorNoise.depth"):
        noise.depth(img[:2].contiguous())
    with pytest.raises(ValueError, match="SensorNoise.scan"):
        noise.scan(pts[:, :, :2].contiguous(), origin)
    with pytest.raises(ValueError, match="S = 5"):
        veh.step(solver.Commands(torch.zeros((NC.B, 3, 16), dtype=torch.float64, device=DEV), torch.zeros((NC.B, 3), dtype=torch.int32, device=DEV), None, None, None))
    torch.cuda.synchronize()
    # nothing ran: every output holds its poison, every counter and state its value
    assert torch.all(outx == 7.0) and torch.all(outp == 7.0) and np.all(_host16(out16) == 7)
    for t0, t1 in zip(keep, (noise.bias, noise.tick, noise.depth_tick, noise.scan_tick, noise.y, noise.meas)):
        assert torch.equal(t0.view(torch.int64) if t0.dtype == torch.float64 else t0, t1.view(torch.int64) if t1.dtype == torch.float64 else t1)
