"""CPU tests of the force estimator (include/frp_nmpc_estimator.h): the restatement tests/estimator_oracle.py against the same discrete scheme in
50 digits (tests/golden/estimator_mp.npz, tests/tools/gen_estimator_mp.py), the filter's convexity bound and the residual's order on a plant
flown by tests/vehicle_oracle.py, deliberately broken schemes against the fixture, and the boundary of the built library without a device:
the symbols, the struct, every FRP_ERR_ARG rule before any device call, and what solver.Vehicle launches with and without an estimator.
The estimator has no reference counterpart: the fixture and the oracle are its specification."""
import ctypes
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest

from forces_resilient_planner_amd import solver

from . import estimator_cases as EC
from . import estimator_oracle as EO
from . import vehicle_cases as VC
from . import vehicle_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = dict(mass=VC.MASS, g=VC.G, **VC.GAINS)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "estimator_mp.npz"))


def _err(got, pair):
    """max |got - (hi + lo)|, the subtraction of hi made first (exact for a got next to hi)."""
    got = np.asarray(got, dtype=np.float64)
    return float(np.max(np.abs((got - pair[..., 0]) - pair[..., 1])))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _run(fx, c, broken=None):
    S = int(fx["S"][c])
    return EO.update(fx["meas"][c, :S], fx["thrust"][c, :S], fx["f_hat0"][c], fx["y_prev0"][c], int(fx["count0"][c]), float(fx["dt"].reshape(-1)[0]), float(fx["alpha"][c]),
                     int(fx["min_samples"][c]), broken=broken)


def _agrees(fx, c, out):
    """Whether an update's result is the fixture's for case c: the doubles within twice the stored oracle error, the rest exact."""
    S = int(fx["S"][c])
    fh, yp, count, force, fresh, res, stat = out
    tol = 2.0 * float(fx["tol_case"][c])
    if not all(np.all(np.isfinite(np.asarray(v, dtype=np.float64))) for v in (fh, force, res)):
        return False
    ok = _err(fh, fx["f_hat"][c]) <= tol and _err(force, fx["force"][c]) <= tol and _err(res, fx["residual"][c, :S]) <= tol
    return bool(ok and np.array_equal(_bits(yp), _bits(fx["y_prev"][c])) and count == int(fx["count"][c]) and fresh == int(fx["fresh"][c])
                and stat == fx["status"][c, :S].tolist())


# ---- the scheme in 50 digits ----
def test_fixture_is_the_generators_case_list_and_covers_every_branch(fx):
    cases, labels = EC.mp_cases()
    for k, v in cases.items():
        assert fx[k].dtype == v.dtype and np.array_equal(fx[k].view(np.uint8), v.view(np.uint8)), k          # (bytes: the cases hold NaNs)
    C = len(labels)
    assert C == 2 * EC.PER_ALPHA == 62 and int(fx["dps"].reshape(-1)[0]) == 50 and float(fx["tol_factor"].reshape(-1)[0]) == 8.0 and float(fx["dt"].reshape(-1)[0]) == EC.DT == 0.01
    # the census, from the stored results: every branch, both gains, both sample counts, fresh both ways, each on its label
    st, S = fx["status"], fx["S"]
    for a in EC.ALPHAS:
        m = fx["alpha"] == a
        assert m.sum() == EC.PER_ALPHA
        for code in (EC.SKIPPED, EC.FIRST, EC.ABSORBED):
            assert np.any(st[m] == code), (a, code)
        assert set(S[m].tolist()) == {1, 5} and set(fx["fresh"][m].tolist()) == {0, 1}
    assert EC.ALPHAS[0] == 1.0 and 0.0 < EC.ALPHAS[1] < 0.2
    for c, lb in enumerate(labels):
        s, count0, stat, count, fresh = EC.EXPECT[lb]
        assert (int(S[c]), int(fx["count0"][c])) == (s, count0) and tuple(st[c, :s].tolist()) == stat and np.all(st[c, s:] == -1), (c, lb)
        assert (int(fx["count"][c]), int(fx["fresh"][c])) == (count, fresh), (c, lb)
    assert set(labels) == set(EC.EXPECT)
    idx = lambda lb: [c for c, l in enumerate(labels) if l == lb]
    # a first call; the count crossing min_samples inside a call, stopping one short of it, and landing on it
    assert fx["count0"][idx("first_call")[0]] == -1 and fx["count0"][idx("crossing")[0]] < EC.MIN_SAMPLES < fx["count"][idx("crossing")[0]]
    assert fx["count"][idx("not_yet")[0]] == EC.MIN_SAMPLES - 1 and fx["count"][idx("exactly")[0]] == EC.MIN_SAMPLES
    assert fx["count"][idx("count_saturates")[0]] == EC.INT_MAX
    # a NaN or an infinity in each of the ten input positions, and all three kinds of them
    kinds = set()
    for k in range(10):
        c = idx("nan_pos_%d" % k)[0]
        row = np.r_[fx["meas"][c, 2], fx["thrust"][c, 2]]
        bad = np.nonzero(~np.isfinite(row))[0]
        assert bad.tolist() == [k] and np.all(np.isfinite(fx["meas"][c, [0, 1, 3, 4]])) and np.all(np.isfinite(fx["thrust"][c, [0, 1, 3, 4]]))
        kinds.add("nan" if np.isnan(row[k]) else "+inf" if row[k] > 0 else "-inf")
    assert kinds == {"nan", "+inf", "-inf"}
    # the thrust at both bounds, rolled and pitched attitudes, a residual that is zero up to the rounding of T / m - g
    assert np.all(fx["thrust"][idx("thrust_lo")[0]] == VO.THRUST_LO) and np.all(fx["thrust"][idx("thrust_hi")[0]] == VO.THRUST_HI)
    assert abs(fx["meas"][idx("rolled")[0], 0, 6]) > 0.4 and abs(fx["meas"][idx("pitched")[0], 0, 7]) > 0.4
    rp = fx["meas"][idx("rolled_pitched")[0], 0]
    assert abs(rp[6]) > 0.4 and abs(rp[7]) > 0.4
    z = idx("zero_residual")[0]
    assert np.max(np.abs(fx["residual"][z].sum(axis=-1))) < 1e-14 and np.max(np.abs(fx["f_hat0"][z])) > 0.1
    tol = fx["tol_case"]
    # a few units in the last place of accelerations below 32 m/s^2
    assert tol.shape == (C,) and np.all(tol >= 2.0 ** -52) and np.max(tol) < 4 * 32 * 2.0 ** -52


def test_oracle_agrees_with_the_scheme_in_50_digits(fx):
    worst = 0.0
    for c in range(len(fx["S"])):
        out = _run(fx, c)
        S = int(fx["S"][c])
        e = max(_err(out[0], fx["f_hat"][c]), _err(out[3], fx["force"][c]), _err(out[5], fx["residual"][c, :S]))
        worst = max(worst, e)
        # (the stored tolerance is this very measurement on the generating machine; another libm may differ in the last place)
        assert _agrees(fx, c, out), (c, e, float(fx["tol_case"][c]))
        assert out[0] == out[3]                                                    # force is f_hat
    print("oracle against the 50-digit scheme, worst absolute error over all cases: %.3e" % worst)
    assert worst <= 2.0 * float(np.max(fx["tol_case"]))


@pytest.mark.parametrize("broken", EO.BREAKS)
def test_a_deliberately_broken_scheme_fails_its_named_case(fx, broken):
    _, labels = EC.mp_cases()
    named = [c for c, lb in enumerate(labels) if lb == EC.BREAK_FAILS[broken]]
    assert named
    failed = [c for c in range(len(labels)) if not _agrees(fx, c, _run(fx, c, broken=broken))]
    print(broken, "fails cases", failed)
    assert set(named) & set(failed), (broken, failed)
    if broken == "gain_complement":                                                # both gains tell alpha from 1 - alpha
        assert {float(fx["alpha"][c]) for c in failed} == set(EC.ALPHAS)
    if broken == "fresh_strict":                                                   # and only the cases that end ON min_samples
        assert all(int(fx["count"][c]) == EC.MIN_SAMPLES for c in failed)


# ---- on a plant flown by the vehicle's oracle ----
def _flight(dt_cmd, n, f, n_sub=64):
    """n samples of dt_cmd flown by VO.step towards a hold half a metre away under the constant force f: (states [n + 1][9], thrust [n])."""
    x0 = [0.5, 0.25, 1.0, 0.6, -0.4, 0.2, 0.15, -0.1, 0.4]
    _, hold = VO.reset(x0)
    hold[0] += 0.4; hold[1] -= 0.3; hold[3] += 0.2
    cmd, kind = np.zeros((n, 16)), [VO.NONE] * n
    _, _, trace, _, thrust = EO.fly(x0, hold, f, cmd, kind, dt_cmd=dt_cmd, n_sub=n_sub, **SCALARS)
    return [x0] + trace, thrust


def test_estimate_obeys_the_filters_convexity_bound_on_a_flown_plant():
    """f_hat_n - f = (1 - alpha)^n (f_hat_0 - f) + sum_k alpha (1 - alpha)^(n - k) (r_k - f): with f_hat_0 = 0 and the weights summing to
    1 - (1 - alpha)^n <= 1, per axis |f_hat_n - f| <= (1 - alpha)^n |f| + max_k |r_k - f|, plus the rounding of n filter steps."""
    f = [0.9, -0.6, 0.4]
    for alpha in EC.ALPHAS + (0.3,):
        for n in (5, 40):
            states, thrust = _flight(0.01, n, f)
            out = EO.update(states[1:], thrust, [0.0] * 3, states[0], 0, 0.01, alpha, EC.MIN_SAMPLES)
            assert out[2] == n and out[6] == [EO.ABSORBED] * n and out[4] == int(n >= EC.MIN_SAMPLES)
            for i in range(3):
                dev = max(abs(r[i] - f[i]) for r in out[5])
                bound = (1.0 - alpha) ** n * abs(f[i]) + dev + 8 * n * 2.0 ** -52
                assert abs(out[0][i] - f[i]) <= bound, (alpha, n, i, out[0][i], bound)
            if alpha == 1.0:
                assert out[0] == out[5][-1]                                         # the whole residual: the estimate is the last one
    # and the residual is the force to the scheme's accuracy: far inside the planner's noise bound
    assert dev < 1e-2 < solver.FSM_EXT_NOISE_BOUND


def test_the_residual_is_second_order_in_the_sample_period():
    """The same 0.08 s of flight sampled at dt, dt / 2 and dt / 4 (the plant itself integrated far finer, n_sub = 64): max_s |r_s - f| falls
    by 4 per halving -- the trapezoidal mean of the model's acceleration misses the mean over the sample by O(dt^2).  The controller runs
    once per sample, so the three flights differ slightly and the ratio is not exactly 4: measured 3.992 and 3.996 (orders 1.997, 1.999),
    held to [3.5, 4.5], an observed order within 0.2 of 2."""
    f = [0.9, -0.6, 0.4]
    errs = []
    for dt, n in ((0.02, 4), (0.01, 8), (0.005, 16)):
        states, thrust = _flight(dt, n, f)
        out = EO.update(states[1:], thrust, [0.0] * 3, states[0], 0, dt, 1.0, 1)
        errs.append(max(abs(r[i] - f[i]) for r in out[5] for i in range(3)))
    ratios = [errs[0] / errs[1], errs[1] / errs[2]]
    print("max |r - f| at dt = 0.02, 0.01, 0.005:", ["%.3e" % e for e in errs], "ratios", ["%.3f" % r for r in ratios],
          "observed order", ["%.3f" % math.log2(r) for r in ratios])
    assert errs[2] > 1e-9                                                           # the scheme's error, not rounding
    assert all(3.5 <= r <= 4.5 for r in ratios), ratios


def test_thrusts_of_a_flight_are_the_controllers_and_the_reset_is_masked():
    states, thrust = _flight(0.01, 5, [0.0] * 3, n_sub=4)
    assert len(thrust) == 5 and all(VO.THRUST_LO <= t <= VO.THRUST_HI for t in thrust) and len(set(thrust)) == 5
    st = ([0.3, 0.2, 0.1], [1.0] * 9, 7, [0.3, 0.2, 0.1], 1)
    assert EO.reset(*st, mask=0) == ([0.3, 0.2, 0.1], [1.0] * 9, 7, [0.3, 0.2, 0.1], 1)
    assert EO.reset(*st) == ([0.0] * 3, [1.0] * 9, -1, [0.0] * 3, 0)


# ---- the boundary, without a device ----
FRP_ERR_NO_DEVICE, FRP_ERR_ARG = -1001, -1003
NAMES = ["frp_nmpc_vehicle_step_observed", "frp_nmpc_estimator_update", "frp_nmpc_estimator_reset"]


def _has_gpu():
    try:
        return solver.lib().frp_nmpc_device_count() > 0
    except Exception:
        return False


def test_the_three_calls_are_declared_and_exported_and_the_struct_is_the_headers(tmp_path):
    own = open(os.path.join(ROOT, "include", "frp_nmpc_estimator.h")).read()
    declared = re.findall(r"^int (frp_nmpc_\w+)\(", own, flags=re.M)
    assert declared == NAMES == solver.ESTIMATOR_EXPORTS
    lib = solver.lib()
    for n in NAMES:
        assert hasattr(lib, n), n
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    assert hdr.count('#include "frp_nmpc_estimator.h"') == 1 and "#define FRP_NMPC_ABI_VERSION 7" in hdr and solver.ABI_VERSION == 7
    assert "(13)" in hdr and "section (13)" in own and "no reference counterpart" in own.lower() and "structurally unpinned" in own.lower()
    lines = [f'_Static_assert(sizeof(frp_nmpc_estimator) == {ctypes.sizeof(solver.EstimatorArgs)}, "size");']
    for fld, _ in solver.EstimatorArgs._fields_:
        lines.append(f'_Static_assert(offsetof(frp_nmpc_estimator, {fld}) == {getattr(solver.EstimatorArgs, fld).offset}, "{fld}");')
    lines.append('_Static_assert(FRP_EST_SKIPPED == 0 && FRP_EST_FIRST == 1 && FRP_EST_ABSORBED == 2, "status");')
    assert (solver.EST_SKIPPED, solver.EST_FIRST, solver.EST_ABSORBED) == (EO.SKIPPED, EO.FIRST, EO.ABSORBED) == (EC.SKIPPED, EC.FIRST, EC.ABSORBED) == (0, 1, 2)
    for inc in ("frp_nmpc.h", "frp_nmpc_estimator.h"):   # through frp_nmpc.h, and on its own; strict C99 plus the C11 assertion
        src = tmp_path / ("layout_" + inc.replace(".", "_") + ".c")
        src.write_text('#include <stddef.h>\n#include "' + inc + '"\n' + "\n".join(lines) +
                       "\nint main(void) { frp_nmpc_vehicle v; (void)v; return 0; }\n")
        subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(src) + ".o"])
    # the defaults are the documented choice, and the gain is the host's
    d = solver.ESTIMATOR_DEFAULTS
    assert set(d) == {"tau", "min_samples"} and d["min_samples"] >= 1 and d["tau"] > 0
    assert -math.expm1(-solver.VEHICLE_DEFAULTS["dt_cmd"] / d["tau"]) == EC.ALPHAS[1]
    assert "chosen, not derived" in solver.ForceEstimator.__doc__.lower()


def _update(**kw):
    a = dict(EC.GOOD_UPDATE); a.update(kw)
    e = solver.EstimatorArgs(*[a[f] for f, _ in solver.EstimatorArgs._fields_])   # the addresses are never dereferenced on the host
    return solver.lib().frp_nmpc_estimator_update(ctypes.byref(e), None)


def _observed(thrust, **kw):
    a = dict(VC.GOOD_STEP); a.update(kw)
    vals = [(ctypes.c_double * 3)(*a[f]) if f in ("kp", "kv", "ka") else a[f] for f, _ in solver.VehicleArgs._fields_]
    return solver.lib().frp_nmpc_vehicle_step_observed(ctypes.byref(solver.VehicleArgs(*vals)), thrust, None)


def test_every_bad_argument_is_refused_before_any_device_call():
    """Without a device a call that passes the argument checks answers FRP_ERR_NO_DEVICE, so FRP_ERR_ARG here was decided before any device
    call; with a device the same order holds and the good calls are not made here (their addresses are not memory)."""
    l, vp = solver.lib(), ctypes.c_void_p
    assert l.frp_nmpc_estimator_update(None, None) == FRP_ERR_ARG
    for bad in EC.BAD_UPDATE:
        assert _update(**bad) == FRP_ERR_ARG, bad
    assert l.frp_nmpc_vehicle_step_observed(None, vp(0x8000), None) == FRP_ERR_ARG
    assert _observed(None) == FRP_ERR_ARG                                           # thrust NULL
    for bad in VC.BAD_STEP:                                                         # every other rule is the step's
        assert _observed(vp(0x8000), **bad) == FRP_ERR_ARG, bad
    a, b, c, d, e = vp(0x1000), vp(0x2000), vp(0x3000), vp(0x4000), vp(0x5000)
    for args in ((0, None, a, b, c, d, e), (-1, None, a, b, c, d, e), (4, None, None, b, c, d, e), (4, None, a, None, c, d, e), (4, None, a, b, None, d, e),
                 (4, None, a, b, c, None, e), (4, None, a, b, c, d, None)):
        assert l.frp_nmpc_estimator_reset(*args, None) == FRP_ERR_ARG, args
    if not _has_gpu():
        assert _update() == FRP_ERR_NO_DEVICE and _update(residual=None, status=None) == FRP_ERR_NO_DEVICE
        assert _update(alpha=1.0, min_samples=1, S=1, B=1) == FRP_ERR_NO_DEVICE and _update(alpha=5e-324, dt=5e-324) == FRP_ERR_NO_DEVICE
        assert _observed(vp(0x8000)) == FRP_ERR_NO_DEVICE and _observed(vp(0x8000), trace=None, sat=None) == FRP_ERR_NO_DEVICE
        assert l.frp_nmpc_estimator_reset(4, None, a, b, c, d, e, None) == FRP_ERR_NO_DEVICE
        assert l.frp_nmpc_estimator_reset(4, vp(0x6000), a, b, c, d, e, None) == FRP_ERR_NO_DEVICE


# ---- what solver.Vehicle launches ----
class _Recorder:
    """Stands in for the loaded library: records (name, arguments) of every call and answers FRP_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            first = args[0]
            if hasattr(first, "_obj"):                                              # a byref(struct): keep a copy of its fields
                first = {f: getattr(first._obj, f) for f, _ in first._obj._fields_ if f not in ("kp", "kv", "ka")}
            self.calls.append((name, first, args[1:]))
            return 0
        return call


def _host_vehicle(trace):
    import torch
    fleet = types.SimpleNamespace(torch=torch, B=3, solver=types.SimpleNamespace(device=torch.device("cpu")))
    veh = solver.Vehicle(fleet, trace=trace)
    cmds = solver.Commands(torch.zeros((3, 5, 16), dtype=torch.float64), torch.zeros((3, 5), dtype=torch.int32), None, None, None)
    return veh, cmds, types.SimpleNamespace(cuda_stream=0x77), torch


@pytest.mark.parametrize("trace", [False, True])
def test_vehicle_without_an_estimator_makes_the_calls_it_made_before_and_with_one_feeds_it(monkeypatch, trace):
    rec = _Recorder()
    monkeypatch.setattr("forces_resilient_planner_amd.flight.lib", lambda: rec)
    veh, cmds, stream, torch = _host_vehicle(trace)
    assert veh.estimator is None
    x0, mask = torch.zeros((3, 9), dtype=torch.float64), torch.ones((3,), dtype=torch.int32)
    veh.step(cmds, stream); veh.reset(x0, mask, stream); veh.reset(x0, None, stream)
    assert [c[0] for c in rec.calls] == ["frp_nmpc_vehicle_step", "frp_nmpc_vehicle_reset", "frp_nmpc_vehicle_reset"]
    v = rec.calls[0][1]
    assert (v["B"], v["S"], v["n_sub"]) == (3, 5, 4) and v["x"] == veh.x.data_ptr() and v["trace"] == (veh.trace.data_ptr() if trace else None)
    assert len(rec.calls[0][2]) == 1 and rec.calls[0][2][0].value == 0x77           # (struct, stream): no further argument
    # with an estimator: the observed step and the update, in that order, on the same stream; the reset under the same mask
    del rec.calls[:]
    est = solver.ForceEstimator(veh, residual=True)
    assert veh.estimator is est and (est.B, est.S, est.dt, est.min_samples) == (3, 5, veh.dt_cmd, solver.ESTIMATOR_DEFAULTS["min_samples"])
    assert est.alpha == -math.expm1(-veh.dt_cmd / solver.ESTIMATOR_DEFAULTS["tau"]) and int(est.count.min()) == int(est.count.max()) == -1
    veh.step(cmds, stream); veh.reset(x0, mask, stream); veh.reset(x0, None, stream)
    assert [c[0] for c in rec.calls] == ["frp_nmpc_vehicle_step_observed", "frp_nmpc_estimator_update", "frp_nmpc_vehicle_reset", "frp_nmpc_estimator_reset",
                                         "frp_nmpc_vehicle_reset", "frp_nmpc_estimator_reset"]
    v, rest = rec.calls[0][1], rec.calls[0][2]
    meas = veh.trace if trace else est.meas                                         # the vehicle's own trace, or else the estimator's meas
    assert v["trace"] == meas.data_ptr() and v["x"] == veh.x.data_ptr() and rest[0].value == est.thrust.data_ptr() and rest[1].value == 0x77
    e = rec.calls[1][1]
    assert (e["B"], e["S"], e["min_samples"], e["dt"], e["alpha"]) == (3, 5, est.min_samples, est.dt, est.alpha)
    assert (e["meas"], e["thrust"], e["f_hat"], e["y_prev"], e["count"], e["force"], e["fresh"], e["residual"], e["status"]) == \
        tuple(t.data_ptr() for t in (meas, est.thrust, est.f_hat, est.y_prev, est.count, est.force, est.fresh, est.residual, est.status))
    assert rec.calls[3][1] == 3 and rec.calls[3][2][0].value == mask.data_ptr() and rec.calls[5][2][0] is None
    assert [a.value for a in rec.calls[3][2][1:6]] == [t.data_ptr() for t in (est.f_hat, est.y_prev, est.count, est.force, est.fresh)]
    with pytest.raises(ValueError):
        solver.ForceEstimator(veh, tau=0.0)
    with pytest.raises(ValueError):
        solver.ForceEstimator(veh, min_samples=0)
