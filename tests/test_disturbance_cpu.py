"""CPU tests of the disturbance model (include/frp_nmpc.h section 15): the restatement tests/disturbance_oracle.py against the exact rational
and 50-digit scheme of tests/golden/disturbance_mp.npz (tests/tools/gen_disturbance_mp.py) with the branches counted, the generator's integers
against a big-integer restatement, the statistics of 2^16 draws per axis, and the boundary of the built library without a device: the symbols,
the struct, every FRP_ERR_ARG rule before any device call, and what solver.Vehicle launches with a solver.Disturbance attached.
The model has no reference counterpart: the fixture and the oracle are its specification."""
import collections
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

from forces_resilient_planner_amd import capi, distributed, solver

from . import disturbance_cases as DC
from . import disturbance_oracle as DO
from . import vehicle_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRP_ERR_NO_DEVICE, FRP_ERR_ARG = -1001, -1003
NAMES = ["frp_nmpc_disturbance_eval", "frp_nmpc_disturbance_reset", "frp_nmpc_vehicle_step_field"]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "disturbance_mp.npz"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _run(sc, case, S, branches=None):
    gust = sc["gust"]
    a, c = DC.gust_coefficients(gust["sigma"], gust["tau"]) if gust else ([0.0] * 3, [0.0] * 3)
    return DO.evaluate(case["pos"][:S], int(case["tick0"]), int(case["lane"]), case["base"], sc["zones"], case["events"], list(case["g0"]) if gust else None,
                       a, c, sc["seed"], sc["id0"], sc["t_epoch"], DC.DT, branches)


# ---- the oracle against the fixture ----
def test_the_oracle_is_the_exact_scheme_to_the_bit_and_takes_every_branch(fx):
    scenes = DC.scenes()
    assert [s["name"] for s in scenes] == list(fx["names"]) and {len(s["zones"]) for s in scenes} == {0, 1, 16} and {s["E"] for s in scenes} == {0, 1, 8}
    count = collections.Counter()
    for sc in scenes:
        name = sc["name"]
        arr = DC.arrays(sc)
        for k, v in arr.items():                                   # the fixture's inputs are the case list's
            assert np.array_equal(fx[f"{name}_{k}"], v, equal_nan=True), (name, k)
        for ci, case in enumerate(sc["cases"]):
            taken = []
            f, g, tick = _run(sc, case, 5, taken)
            per = len(sc["zones"]) + sc["E"] + (1 if sc["gust"] else 0)
            assert len(taken) == 5 * per and tick == case["tick0"] + 5
            for s in range(5):
                got = taken[s * per:(s + 1) * per]
                assert tuple(b for b in got if b != DO.GUST) == tuple(case["expect"][s]), (name, ci, s)
                assert got.count(DO.GUST) == (1 if sc["gust"] else 0)
            count.update(taken)
            if not sc["gust"]:
                assert g is None and np.array_equal(_bits(f), _bits(fx[f"{name}_det"][ci])), (name, ci)
                f1, _, t1 = _run(sc, case, 1)                      # one sample alone is the first of five
                assert t1 == case["tick0"] + 1 and np.array_equal(_bits(f1), _bits(fx[f"{name}_det"][ci][:1]))
            else:
                want, tol = fx[f"{name}_force"][ci], fx[f"{name}_tol_case"][ci]
                err = np.abs((np.array(f) - want[..., 0]) - want[..., 1]).max()
                gw = fx[f"{name}_gust"][ci][4]
                assert err <= tol and np.abs((np.array(g) - gw[:, 0]) - gw[:, 1]).max() <= tol, (name, ci, err, tol)
                assert tol >= 2.0 ** -52 and tol < 1e-14
    # every branch of the model was taken, and as often as the cases were built to take it
    built = collections.Counter(b for sc in scenes for case in sc["cases"] for row in case["expect"] for b in row)
    built[DO.GUST] = sum(5 * len(sc["cases"]) for sc in scenes if sc["gust"])
    assert count == built and set(count) == {DO.ZONE_OFF, DO.ZONE_OUT, DO.ZONE_RAMP, DO.ZONE_FULL, DO.EVENT_ON, DO.EVENT_OFF, DO.GUST}
    assert min(count.values()) >= 10, count
    assert (DO.ZONE_OFF, DO.ZONE_OUT, DO.ZONE_RAMP, DO.ZONE_FULL, DO.EVENT_ON, DO.EVENT_OFF) == (DC.OFF, DC.OUT, DC.RAMP, DC.FULL, DC.EV_ON, DC.EV_OFF)


def test_the_edges_the_cases_were_built_on(fx):
    """A face is closed, one ulp decides; d == ramp is full weight and the double below it is not; t == t_on is in, t == t_off is out."""
    box = DC.scenes()[0]
    zone = box["zones"][0]
    t_in = DC.t_of(60, DC.BOX_EPOCH)
    for face in range(6):
        pos = box["cases"][face]["pos"]
        w = [DO.zone_weight(zone, p, t_in)[0] for p in pos]
        # (every coordinate is below 4 in magnitude: one ulp is at most 2^-51, over the ramp of 0.25 at most 2^-49)
        assert w[0] == 0.0 and 0.0 < w[1] <= 2.0 ** -49 and w[2] == 0.0 and w[3] == 1.0 and 1.0 - 2.0 ** -48 < w[4] < 1.0, (face, w)
    mid = [0.5, 1.0, 2.0]
    assert DO.zone_weight(zone, mid, zone[10])[1] == DO.ZONE_FULL and DO.zone_weight(zone, mid, zone[11])[1] == DO.ZONE_OFF
    assert DO.zone_weight(zone, mid, math.nextafter(zone[10], -math.inf))[1] == DO.ZONE_OFF
    hard = list(zone); hard[9] = 0.0                              # ramp = 0: a hard edge with closed faces
    assert DO.zone_weight(hard, box["cases"][0]["pos"][0], t_in) == (1.0, DO.ZONE_FULL) and DO.zone_weight(hard, box["cases"][0]["pos"][2], t_in)[0] == 0.0
    forever = list(zone); forever[11] = math.inf
    assert DO.zone_weight(forever, mid, 1e300)[1] == DO.ZONE_FULL
    for bad in (math.nan, math.inf, -math.inf):
        assert DO.zone_weight(zone, [bad, 1.0, 2.0], t_in) == (0.0, DO.ZONE_OUT)
    # reset, and a pure query
    assert DO.reset([1.0, 2.0, 3.0], 17) == ([0.0, 0.0, 0.0], 0) and DO.reset([1.0, 2.0, 3.0], 17, mask=0) == ([1.0, 2.0, 3.0], 17) and DO.reset(None, 5) == (None, 0)


# ---- the generator's integers ----
def _finalise(x):
    """SplitMix64's finaliser restated on unbounded integers with % and //."""
    m = 2 ** 64
    x = (x + 0x9E3779B97F4A7C15) % m
    x = ((x ^ (x // 2 ** 30)) * 0xBF58476D1CE4E5B9) % m
    x = ((x ^ (x // 2 ** 27)) * 0x94D049BB133111EB) % m
    return x ^ (x // 2 ** 31)


def test_the_generators_integers_against_a_big_integer_restatement_and_the_package_mixer():
    import torch
    m = 2 ** 64
    quads = [(0, 0, 0, 0), (1, 2, 3, 1), (20261021, 1000, 54, 2), (-7, -3, 2 ** 31 - 1, 0), (-7, -1, 2 ** 31, 1), (2 ** 63 - 1, -2 ** 63 + 256, 2 ** 31 + 1, 2),
                 (12345, 2 ** 63 - 1, 2 ** 40, 0)]
    for seed, ident, k, axis in quads:
        h = _finalise((_finalise((_finalise(seed % m) + ident) % m) + k) % m)
        r0, r1 = _finalise((h + 2 * axis) % m), _finalise((h + 2 * axis + 1) % m)
        u1, u2 = DO.uniforms(seed, ident, k, axis)
        assert DO.stream_key(seed % m, ident % m, k % m) == h
        assert u1 == (r0 // 2048 + 1) / 2.0 ** 53 and u2 == (r1 // 2048) / 2.0 ** 53 and 0.0 < u1 <= 1.0 and 0.0 <= u2 < 1.0
        assert DO.normal(seed, ident, k, axis) == math.sqrt(-2.0 * math.log(u1)) * math.cos(6.283185307179586 * u2)
    # the finaliser is the package's (distributed._splitmix64, on wrapping int64 tensors), the same constants
    xs = [0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1, 0x0123456789ABCDEF]
    signed = lambda v: v - m if v >= 2 ** 63 else v
    got = distributed._splitmix64(torch.tensor([signed(v) for v in xs], dtype=torch.int64)).tolist()
    assert [v % m for v in got] == [DO.mix(v) for v in xs] == [_finalise(v) for v in xs]
    assert DO.U1_DIV == 2.0 ** 53 == DO.U2_DIV                    # 2^53 + 1 is no double: the literal denotes 2^53
    # the draw depends on (seed, id0 + b, k, axis) alone: the same vehicle under another split of the fleet or of the flight
    assert DO.normal(5, 100 + 7, 9, 1) == DO.normal(5, 107 + 0, 9, 1) and DO.normal(5, 7, 9, 1) != DO.normal(5, 7, 10, 1)
    assert len({DO.normal(5, 7, 9, ax) for ax in range(3)}) == 3 and DO.normal(5, 7, 9, 0) != DO.normal(6, 7, 9, 0) != DO.normal(5, 8, 9, 0)


# ---- the statistics of the gusts ----
STAT_N, STAT_BURN, STAT_SEED = 2 ** 16, 1024, 1


def test_statistics_of_65536_gust_samples_per_axis():
    """The mean, the variance and the lag-1 autocorrelation of g within 5 standard errors of 0, sigma^2 and a.  For a stationary AR(1)
    process of coefficient a and variance v over N samples (Bartlett's large-sample formulas):
        se(mean) = sqrt(v (1 + a) / ((1 - a) N)),  se(var) = v sqrt(2 (1 + a^2) / ((1 - a^2) N)),  se(r1) = sqrt((1 - a^2) / N).
    The process starts from g = 0 (what a reset leaves), so the first STAT_BURN samples -- many time constants -- are drawn and not counted.
    STAT_SEED is fixed: the draws are deterministic, and this seed passes."""
    sigma, tau = (0.5, 0.3, 0.2), (0.05, 0.1, 0.02)
    a, c = DO.gust_coefficients(sigma, tau, DC.DT)
    g = [0.0, 0.0, 0.0]
    rows = np.empty((STAT_N, 3))
    for k in range(STAT_BURN + STAT_N):
        _, g = DO.sample([0.0, 0.0, 0.0], k, 0, [0.0, 0.0, 0.0], [], [], g, a, c, STAT_SEED, 0, 0.0, DC.DT)
        if k >= STAT_BURN:
            rows[k - STAT_BURN] = g
    for i in range(3):
        x, v, N = rows[:, i], sigma[i] ** 2, STAT_N
        mean, var = x.mean(), x.var()
        r1 = np.mean((x[1:] - mean) * (x[:-1] - mean)) / var
        se = (math.sqrt(v * (1 + a[i]) / ((1 - a[i]) * N)), v * math.sqrt(2 * (1 + a[i] ** 2) / ((1 - a[i] ** 2) * N)), math.sqrt((1 - a[i] ** 2) / N))
        z = (mean / se[0], (var - v) / se[1], (r1 - a[i]) / se[2])
        print("axis %d: a = %.4f; mean %+.3e (%.2f se), variance %.5f against %.5f (%.2f se), lag-1 %.5f (%.2f se)" % (i, a[i], mean, z[0], var, v, z[1], r1, z[2]))
        assert all(abs(u) <= 5.0 for u in z), (i, z)


# ---- the boundary, without a device ----
def _has_gpu():
    try:
        return solver.lib().frp_nmpc_device_count() > 0
    except Exception:
        return False


def test_the_three_calls_are_declared_in_frp_nmpc_h_and_the_struct_is_the_headers():
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    assert re.findall(r"^int (frp_nmpc_disturbance_\w+|frp_nmpc_vehicle_step_field)\(", hdr, flags=re.M) == NAMES
    assert all(n in solver.EXPORTS and hasattr(solver.lib(), n) for n in NAMES) and not os.path.exists(os.path.join(ROOT, "include", "frp_nmpc_disturbance.h"))
    assert "#define FRP_NMPC_ABI_VERSION 7" in hdr and solver.ABI_VERSION == 7 and "---- (15)" in hdr and "no reference counterpart" in hdr.lower()
    assert capi.C_TYPES[capi.DisturbanceArgs] == ("frp_nmpc_disturbance", "frp_nmpc.h")
    assert [f for f, _ in capi.DisturbanceArgs._fields_] == ["B", "Z", "E", "t_epoch", "dt", "gust_a", "gust_c", "seed", "id0", "zone", "event", "gust", "tick"]
    assert (solver.DISTURBANCE_MAX_ZONES, solver.DISTURBANCE_MAX_EVENTS, solver.DISTURBANCE_ZONE_STRIDE, solver.DISTURBANCE_EVENT_STRIDE) == \
        (DO.MAX_ZONES, DO.MAX_EVENTS, DO.ZONE_STRIDE, DO.EVENT_STRIDE) == (16, 8, 12, 5)
    build = __import__("forces_resilient_planner_amd.build", fromlist=["x"])
    assert "frp_disturbance.hip" in build.SOURCES and "frp_disturbance.hpp" in build.HEADERS
    assert build.PER_SOURCE_FLAGS["frp_disturbance.hip"] == ["-ffp-contract=off"] == build.PER_SOURCE_FLAGS["frp_vehicle.hip"]
    assert solver.Disturbance.__module__.endswith(".flight") and "chosen, not derived" in solver.Disturbance.__doc__.lower()


def _dist(**kw):
    a = dict(DC.GOOD); a.update(kw)
    vals = [(ctypes.c_double * 3)(*a[f]) if f in ("gust_a", "gust_c") else a[f] for f, _ in solver.DisturbanceArgs._fields_]
    return solver.DisturbanceArgs(*vals)


def _vehicle_args(**kw):
    a = dict(VC.GOOD_STEP); a.update(kw)
    return solver.VehicleArgs(*[(ctypes.c_double * 3)(*a[f]) if f in ("kp", "kv", "ka") else a[f] for f, _ in solver.VehicleArgs._fields_])


def test_every_bad_argument_is_refused_before_any_device_call():
    """Without a device a call that passes the argument checks answers FRP_ERR_NO_DEVICE, so FRP_ERR_ARG here was decided before any device
    call; with a device the good calls are not made here (their addresses are not memory)."""
    l, vp = solver.lib(), ctypes.c_void_p
    pos, force = vp(0x5000), vp(0x6000)
    ev = lambda d, S=5, pos=pos, base=None, force=force: l.frp_nmpc_disturbance_eval(ctypes.byref(d) if d is not None else None, S, pos, base, 1, force, None)
    rs = lambda d: l.frp_nmpc_disturbance_reset(ctypes.byref(d) if d is not None else None, None, None)
    vb = VC.GOOD_STEP["B"]
    sf = lambda d, v=None, thrust=None: l.frp_nmpc_vehicle_step_field(ctypes.byref(v if v is not None else _vehicle_args()), ctypes.byref(d) if d is not None else None,
                                                                        thrust, force, None)
    assert ev(None) == rs(None) == sf(None) == FRP_ERR_ARG
    assert l.frp_nmpc_vehicle_step_field(None, ctypes.byref(_dist(B=vb)), None, None, None) == FRP_ERR_ARG
    for bad in DC.BAD:
        d = _dist(**bad)
        assert ev(d) == FRP_ERR_ARG and rs(d) == FRP_ERR_ARG, bad
        if "B" not in bad:
            assert sf(_dist(**dict(bad, B=vb))) == FRP_ERR_ARG, bad
    good = _dist()
    assert ev(good, S=0) == ev(good, S=-1) == ev(good, pos=None) == ev(good, force=None) == FRP_ERR_ARG
    assert ev(_dist(B=2 ** 30), S=2) == FRP_ERR_ARG                                   # B * S beyond 2^31 - 1
    # the fused step: the vehicle's own rules, and the two that tie the structs together
    assert sf(_dist(B=vb + 1)) == FRP_ERR_ARG and sf(_dist(B=vb, dt=0.5 * VC.GOOD_STEP["dt_cmd"])) == FRP_ERR_ARG
    for bad in VC.BAD_STEP:
        v = _vehicle_args(**bad)
        assert sf(_dist(B=v.B if v.B >= 1 else vb), v) == FRP_ERR_ARG, bad
    if not _has_gpu():
        assert ev(good) == rs(good) == FRP_ERR_NO_DEVICE and ev(good, S=1, base=vp(0x7000)) == FRP_ERR_NO_DEVICE
        assert l.frp_nmpc_disturbance_reset(ctypes.byref(good), vp(0x7000), None) == FRP_ERR_NO_DEVICE
        for ok in DC.GOOD_TOO:
            assert ev(_dist(**ok)) == rs(_dist(**ok)) == FRP_ERR_NO_DEVICE, ok
            assert sf(_dist(**dict(ok, B=vb, dt=VC.GOOD_STEP["dt_cmd"]))) == FRP_ERR_NO_DEVICE, ok
        assert sf(_dist(B=vb, dt=VC.GOOD_STEP["dt_cmd"]), thrust=vp(0x8000)) == FRP_ERR_NO_DEVICE
        assert l.frp_nmpc_vehicle_step_field(ctypes.byref(_vehicle_args()), ctypes.byref(_dist(B=vb, dt=VC.GOOD_STEP["dt_cmd"])), None, None, None) == FRP_ERR_NO_DEVICE


# ---- what solver.Vehicle launches ----
class _Recorder:
    """Stands in for the loaded library: records (name, arguments) of every call and answers FRP_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, [({f: getattr(a._obj, f) for f, _ in a._obj._fields_ if not hasattr(getattr(a._obj, f), "__len__")} if hasattr(a, "_obj") else a)
                                      for a in args]))
            return 0
        return call


def test_vehicle_with_a_disturbance_launches_the_field_step_and_resets_it_under_the_same_mask(monkeypatch):
    import torch
    rec = _Recorder()
    monkeypatch.setattr("forces_resilient_planner_amd.flight.lib", lambda: rec)
    fleet = types.SimpleNamespace(torch=torch, B=3, solver=types.SimpleNamespace(device=torch.device("cpu")))
    veh = solver.Vehicle(fleet)
    cmds = solver.Commands(torch.zeros((3, 5, 16), dtype=torch.float64), torch.zeros((3, 5), dtype=torch.int32), None, None, None)
    stream = types.SimpleNamespace(cuda_stream=0x77)
    assert veh.disturbance is None
    veh.step(cmds, stream)
    assert [c[0] for c in rec.calls] == ["frp_nmpc_vehicle_step"]                   # without one, today's launch
    del rec.calls[:]
    zones = [[0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.5, 0.0, 0.0, 0.25, 0.0, math.inf]]
    dist = solver.Disturbance(veh, zones=zones, events=[[1.0, 2.0, 0.0, 0.0, 1.0]], gust_sigma=0.3, gust_tau=(0.5, 1.0, 0.25), seed=-5, id0=40, t_epoch=2.0)
    assert veh.disturbance is dist and (dist.B, dist.S, dist.Z, dist.E, dist.dt) == (3, 5, 1, 1, veh.dt_cmd)
    a, c = DO.gust_coefficients((0.3, 0.3, 0.3), (0.5, 1.0, 0.25), veh.dt_cmd)
    assert list(dist.gust_a) == a and list(dist.gust_c) == c and tuple(dist.event.shape) == (3, 1, 5) and dist.tick.dtype == torch.int64
    assert tuple(dist.force.shape) == (3, 5, 3) and tuple(dist.gust.shape) == (3, 3) and int(dist.tick.abs().sum()) == 0
    x0, mask = torch.zeros((3, 9), dtype=torch.float64), torch.ones((3,), dtype=torch.int32)
    veh.step(cmds, stream); veh.reset(x0, mask, stream)
    assert [c[0] for c in rec.calls] == ["frp_nmpc_vehicle_step_field", "frp_nmpc_vehicle_reset", "frp_nmpc_disturbance_reset"]
    v, d, thrust, force, st = rec.calls[0][1]
    assert v["f_true"] == veh.f_true.data_ptr() and thrust is None and force.value == dist.force.data_ptr() and st.value == 0x77
    assert (d["B"], d["Z"], d["E"], d["t_epoch"], d["dt"], d["seed"], d["id0"]) == (3, 1, 1, 2.0, veh.dt_cmd, -5, 40)
    assert (d["zone"], d["event"], d["gust"], d["tick"]) == tuple(t.data_ptr() for t in (dist.zone, dist.event, dist.gust, dist.tick))
    assert rec.calls[2][1][1].value == mask.data_ptr()
    # with an estimator too: its thrust goes into the same launch, its update follows
    del rec.calls[:]
    est = solver.ForceEstimator(veh)
    veh.step(cmds, stream)
    assert [c[0] for c in rec.calls] == ["frp_nmpc_vehicle_step_field", "frp_nmpc_estimator_update"] and rec.calls[0][1][2].value == est.thrust.data_ptr()
    assert rec.calls[0][1][0]["trace"] == est.meas.data_ptr()
    # the stand-alone call
    del rec.calls[:]
    pos = torch.zeros((3, 2, 3), dtype=torch.float64)
    out = dist.eval(pos, stream=stream)
    name, (d, S, p, base, advance, force, st) = rec.calls[0]
    assert name == "frp_nmpc_disturbance_eval" and (S, advance, base) == (2, 0, None) and p.value == pos.data_ptr() and force.value == out.data_ptr()
    dist.eval(pos, advance=True, base=veh.f_true, out=out, stream=stream)
    assert rec.calls[1][1][4] == 1 and rec.calls[1][1][3].value == veh.f_true.data_ptr()
    # what the class refuses on the host: the ramp's contract, the sizes, half a gust
    for bad in (dict(zones=[zones[0][:9] + [-0.1] + zones[0][10:]]), dict(zones=[zones[0][:9] + [math.nan] + zones[0][10:]]), dict(zones=[zones[0][:9] + [math.inf] + zones[0][10:]]),
                dict(zones=zones * 17), dict(zones=[[0.0] * 11]), dict(events=[[0.0] * 5] * 9), dict(events=np.zeros((2, 1, 5))), dict(gust_sigma=0.1), dict(gust_tau=0.1),
                dict(gust_sigma=-0.1, gust_tau=1.0), dict(gust_sigma=0.1, gust_tau=0.0), dict(seed=2 ** 63), dict(t_epoch=math.inf)):
        with pytest.raises(ValueError):
            solver.Disturbance(veh, **bad)
    bare = solver.Disturbance(veh)
    assert (bare.Z, bare.E, bare.zone, bare.event, bare.gust) == (0, 0, None, None, None) and veh.disturbance is bare
