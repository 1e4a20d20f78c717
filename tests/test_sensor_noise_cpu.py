"""CPU tests of the sensor noise's specification (include/frp_nmpc.h section 16): tests/sensor_noise_oracle.py against the 50-digit fixture
tests/golden/sensor_noise_mp.npz, the separation of its draws from the gusts' and between its channels, the identity at zero noise, the
independence of how a flight is split into calls and a fleet into shards, the absence of near-ties that lets the GPU test demand equal
images -- and the BREAKS: named alterations of the oracle, each of which has to fail the check it is named against.  The argument rules of
the C-ABI are checked here too: FRP_ERR_ARG comes before the device is looked for."""
import ctypes
import math
import os

import numpy as np
import pytest

from forces_resilient_planner_amd import build, capi, solver

from . import disturbance_oracle as DO
from . import sensor_noise_cases as NC
from . import sensor_noise_oracle as NO

M64 = 1 << 64


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "sensor_noise_mp.npz"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _err(got, pair):
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid="ignore"):                 # (inf - inf where a value passed through: the callers mask those)
        return np.abs((got - pair[..., 0]) - pair[..., 1])


def _same_where_not_finite(got, pair):
    got, want = np.asarray(got, dtype=np.float64), pair[..., 0]
    odd = ~np.isfinite(want)
    return np.array_equal(~np.isfinite(got), odd) and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[odd & ~np.isnan(want)], want[odd & ~np.isnan(want)])


# ---- the checks: each takes the alteration set of the oracle it examines; () is the statement ----
def check_states_against_the_fixture(fx, brk=()):
    par = NC.params()
    x, bias0, tick0 = NC.states_case()
    assert np.array_equal(_bits(x), _bits(fx["states_x"])) and np.array_equal(tick0, fx["states_tick0"]) and np.array_equal(_bits(bias0), _bits(fx["states_bias0"]))
    assert list(par["bias_a"]) + list(par["bias_c"]) == list(fx["scalars"])
    for b in range(NC.B):
        m, y, bias, tick = NO.states(x[b], bias0[b], int(tick0[b]), b, par, brk)
        assert _same_where_not_finite(m, fx["states_meas"][b]), b
        fin = np.isfinite(fx["states_meas"][b][..., 0])
        e = max(float(_err(m, fx["states_meas"][b])[fin].max()), float(_err(bias, fx["states_bias"][b]).max()))
        assert e <= fx["states_tol_case"][b], (b, e, fx["states_tol_case"][b])      # the error the generator recorded is the oracle's error
        assert np.array_equal(_bits(y), _bits(m[-1])) and tick % M64 == int(fx["states_tick"][b]), b
        # what is not finite passed through to the bit, and the pitch (sigma 0) is the truth to the bit
        raw = ~np.isfinite(x[b])
        assert np.array_equal(_bits(np.array(m)[raw]), _bits(x[b][raw])) and np.array_equal(_bits(np.array(m)[:, 7]), _bits(x[b][:, 7])), b


def check_depth_against_the_fixture(fx, brk=()):
    par = NC.params()
    cur, ticks = NC.depth_case(), [0] * NC.F
    assert np.array_equal(cur, fx["depth_in"])
    for call in range(NC.DEPTH_CALLS):
        got = []
        for f in range(NC.F):
            o, ticks[f] = NO.depth(cur[f].tolist(), f, ticks[f], par, active=NC.DEPTH_ACTIVE[f], brk=brk)
            got.append(o)
        cur = np.array(got, dtype=np.uint16)
        assert np.array_equal(cur, fx["depth_out"][call]), call
    assert ticks == [NC.DEPTH_CALLS * a for a in NC.DEPTH_ACTIVE]
    assert not np.array_equal(fx["depth_out"][0], fx["depth_out"][1]) and np.array_equal(fx["depth_out"][1][1], fx["depth_in"][1])
    assert np.all(fx["depth_out"][0][fx["depth_in"] == 0] == 0)                    # no return stays no return


def check_scan_against_the_fixture(fx, brk=()):
    par = NC.params()
    pts, origin, count = NC.scan_case()
    assert np.array_equal(_bits(pts), _bits(fx["scan_in"])) and np.array_equal(count, fx["scan_count"])
    for s in range(NC.SCANS):
        o, tick = NO.scan(pts[s], origin[s], int(count[s]), s, 0, par, brk=brk)
        assert tick == 1 and _same_where_not_finite(o, fx["scan_out"][s]), s
        fin = np.isfinite(fx["scan_out"][s][..., 0])
        assert float(_err(o, fx["scan_out"][s])[fin].max()) <= fx["scan_tol_case"][s], s
        assert np.array_equal(_bits(np.array(o)[count[s]:]), _bits(pts[s][count[s]:])), s      # storage beyond count is untouched
    assert np.array_equal(_bits(fx["scan_out"][1][3][:, 0]), _bits(origin[1]))     # the point at the origin stays


def _words(brk=()):
    """Every 64-bit word the case set draws, per channel, and the gusts' words for the same (seed, id0 + b, k)."""
    par = NC.params()
    _, _, tick0 = NC.states_case()
    gust, st, dp, sc = set(), set(), set(), set()
    for b in range(NC.B):
        for s in range(NC.S):
            k = int(tick0[b]) + s
            hg = DO.stream_key(par["seed"], (par["id0"] + b) & DO.MASK, k & DO.MASK)
            gust |= {DO.mix((hg + j) & DO.MASK) for j in range(6)}
            h = NO.sample_key(par["seed"], par["id0"] + b, k, NO.TAG_STATE, brk)
            st |= {w for j in range(12) for w in NO.normal_words(h, j)}
    for f in range(NC.F):
        for k in range(NC.DEPTH_CALLS):
            hg = DO.stream_key(par["seed"], (par["id0"] + f) & DO.MASK, k)
            gust |= {DO.mix((hg + j) & DO.MASK) for j in range(6)}
            hd, hs = NO.sample_key(par["seed"], par["id0"] + f, k, NO.TAG_DEPTH, brk), NO.sample_key(par["seed"], par["id0"] + f, k, NO.TAG_SCAN, brk)
            for idx in range(NC.ROWS * NC.COLS):
                h = DO.mix((hd + idx) & DO.MASK)
                dp |= {DO.mix((h + j) & DO.MASK) for j in range(3)}
            for idx in range(NC.P):
                h = DO.mix((hs + idx) & DO.MASK)
                sc |= {DO.mix((h + j) & DO.MASK) for j in range(3)}
    return gust, st, dp, sc


def check_domain_separation(fx, brk=()):
    gust, st, dp, sc = _words(brk)
    assert len(st) == NC.B * NC.S * 24 and len(dp) == NC.F * NC.DEPTH_CALLS * NC.ROWS * NC.COLS * 3 and len(sc) == NC.F * NC.DEPTH_CALLS * NC.P * 3
    assert not (gust & st) and not (gust & dp) and not (gust & sc)
    assert not (st & dp) and not (st & sc) and not (dp & sc)


def check_split_and_shard(fx, brk=()):
    par = NC.params()
    x, bias0, tick0 = NC.states_case()
    for b in (0, 1, 7, 12, 66):
        whole = NO.states(x[b], bias0[b], int(tick0[b]), b, par, brk)
        bias, tick, rows = list(bias0[b]), int(tick0[b]), []
        for s in range(NC.S):
            m, y, bias, tick = NO.states(x[b][s:s + 1], bias, tick, b, par, brk)
            rows.append(m[0])
        assert np.array_equal(_bits(rows), _bits(whole[0])) and np.array_equal(_bits(bias), _bits(whole[2])) and tick == whole[3] == int(tick0[b]) + NC.S, b
        # the second half of the fleet: vehicle b - 33 of a fleet whose id0 is shifted by 33
        if b >= 33:
            half = NO.states(x[b], bias0[b], int(tick0[b]), b - 33, NC.params(id0=NC.ID0 + 33), brk)
            assert np.array_equal(_bits(half[0]), _bits(whole[0])) and np.array_equal(_bits(half[2]), _bits(whole[2]))
    img = NC.depth_case()
    one, t1 = NO.depth(img[0].tolist(), 0, 0, par, brk=brk)
    two, t2 = NO.depth(one, 0, t1, par, brk=brk)
    assert (t1, t2) == (1, 2) and one != two and two != NO.depth(one, 0, 0, par, brk=brk)[0]       # the second call draws anew
    assert NO.depth(img[2].tolist(), 2, 0, par, brk=brk) == NO.depth(img[2].tolist(), 0, 0, dict(par, id0=NC.ID0 + 2), brk=brk)
    pts, origin, count = NC.scan_case()
    a, b_ = NO.scan(pts[1], origin[1], int(count[1]), 1, 0, par, brk=brk), NO.scan(pts[1], origin[1], int(count[1]), 0, 0, dict(par, id0=NC.ID0 + 1), brk=brk)
    assert np.array_equal(_bits(a[0]), _bits(b_[0]))


def check_zero_pixels_and_count(fx, brk=()):
    par = NC.params()
    img = NC.depth_case()
    out, _ = NO.depth(img[0].tolist(), 0, 0, par, brk=brk)
    assert np.all(np.array(out)[img[0] == 0] == 0)
    pts, origin, count = NC.scan_case()
    o, _ = NO.scan(pts[1], origin[1], int(count[1]), 1, 0, par, brk=brk)
    assert np.array_equal(_bits(np.array(o)[count[1]:]), _bits(pts[1][count[1]:]))


def test_the_oracle_against_the_50_digit_fixture(fx):
    check_states_against_the_fixture(fx)
    check_depth_against_the_fixture(fx)
    check_scan_against_the_fixture(fx)
    assert int(fx["dps"].reshape(-1)[0]) == 50 and float(fx["tol_factor"].reshape(-1)[0]) == 8.0 and list(fx["ints"]) == [NC.SEED, NC.ID0]


def test_no_draw_is_shared_with_the_gusts_or_between_the_channels(fx):
    check_domain_separation(fx)
    assert len({NO.TAG_STATE, NO.TAG_DEPTH, NO.TAG_SCAN}) == 3
    assert (NO.TAG_STATE, NO.TAG_DEPTH, NO.TAG_SCAN) == (capi.SENSOR_NOISE_TAG_STATE, capi.SENSOR_NOISE_TAG_DEPTH, capi.SENSOR_NOISE_TAG_SCAN)


def test_zero_noise_is_the_identity_to_the_bit():
    par = NC.params(zero=True)
    x, bias0, tick0 = NC.states_case()
    for b in range(NC.B):
        m, y, bias, tick = NO.states(x[b], [0.0] * 3, int(tick0[b]), b, par)
        assert np.array_equal(_bits(m), _bits(x[b])) and np.array_equal(_bits(y), _bits(x[b][-1])) and tick == int(tick0[b]) + NC.S, b
    assert np.signbit(x[4, :, 6:9]).all()                                          # (the case holds negative zeros)
    img = NC.depth_case()
    for f in range(NC.F):
        assert NO.depth(img[f].tolist(), f, 0, par)[0] == img[f].tolist()
    pts, origin, count = NC.scan_case()
    for s in range(NC.SCANS):
        assert np.array_equal(_bits(NO.scan(pts[s], origin[s], int(count[s]), s, 0, par)[0]), _bits(pts[s]))


def test_a_call_of_five_samples_is_five_calls_and_a_fleet_is_its_halves(fx):
    check_split_and_shard(fx)


def test_the_depth_and_scan_cases_hold_no_near_tie(fx):
    """What lets tests/test_gpu_sensor_noise.py demand EQUAL images and an exact NaN pattern: the device's log and cos differ from libm's by
    an ulp or so of n, which moves v by at most 65535 * 2^-50 < 1e-10."""
    par = NC.params()
    cur, ticks = NC.depth_case(), [0] * NC.F
    kept = dropped = below = above = 0
    for call in range(NC.DEPTH_CALLS):
        got = []
        for f in range(NC.F):
            detail = []
            o, ticks[f] = NO.depth(cur[f].tolist(), f, ticks[f], par, active=NC.DEPTH_ACTIVE[f], detail=detail)
            got.append(o)
            for idx, u, vh in detail:
                assert abs(u - par["depth_p_drop"]) > 1e-12, (call, f, idx, u)
                if vh is None:
                    dropped += 1
                    continue
                kept += 1
                assert abs(vh - round(vh)) > 1e-6, (call, f, idx, vh)
                below += vh < 1.0
                above += vh >= 65536.0
        cur = np.array(got, dtype=np.uint16)
    assert kept > 5000 and dropped > 500 and below > 10 and above > 10, (kept, dropped, below, above)   # the noise drives pixels off both ends
    assert all(float(fx[n].reshape(-1)[0]) > m for n, m in (("depth_margin", 1e-6), ("depth_u_margin", 1e-12), ("scan_u_margin", 1e-12)))
    img = NC.depth_case()
    assert {0, 1, 65535} <= set(np.unique(img).tolist())
    pts, origin, count = NC.scan_case()
    for s in range(NC.SCANS):
        detail = []
        NO.scan(pts[s], origin[s], int(count[s]), s, 0, par, detail=detail)
        assert all(abs(u - par["scan_p_drop"]) > 1e-12 for _, u in detail) and any(u < par["scan_p_drop"] for _, u in detail), s


# ---- the breaks: (the alteration, the check it has to fail) ----
BREAKS = (("tag_dropped", check_domain_separation), ("tick_not_advanced", check_split_and_shard), ("bias_on_non_finite", check_states_against_the_fixture),
          ("floor_without_half", check_depth_against_the_fixture), ("zero_pixel_redrawn", check_zero_pixels_and_count), ("count_ignored", check_zero_pixels_and_count))


@pytest.mark.parametrize("name,check", BREAKS, ids=[b[0] for b in BREAKS])
def test_every_named_break_fails_its_named_check(fx, name, check):
    assert name in NO.BREAKS and {b[0] for b in BREAKS} == set(NO.BREAKS)
    check(fx)                                          # the statement passes ...
    with pytest.raises(AssertionError):
        check(fx, brk=(name,))                         # ... and the altered one does not


# ---- the C-ABI's argument rules: FRP_ERR_ARG before any device call ----
def good_struct():
    """A valid frp_nmpc_sensor_noise whose pointers are never followed (the refusals come first): (struct, keep-alive)."""
    a, c = NC.coefficients()
    v3 = lambda v: (ctypes.c_double * 3)(*v)
    bias, tick = (ctypes.c_double * 3)(), (ctypes.c_longlong * 1)()
    n = capi.SensorNoiseArgs(1, v3(NC.SIGMA_P), v3(NC.SIGMA_V), v3(NC.SIGMA_A), v3(a), v3(c), 1000.0, 0.002, 0.0005, 0.1, 0.01, 0.002, 0.1, NC.SEED, NC.ID0,
                             ctypes.addressof(bias), ctypes.addressof(tick))
    return n, (bias, tick)


def refusals():
    """(what, a function of the library that makes the refused call) for every rule of the header; each keeps its buffers alive."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    out = []

    def calls(n):
        r = ctypes.byref(n)
        return [lambda l: l.frp_nmpc_sensor_noise_states(r, 1, p, p, p, 1, None), lambda l: l.frp_nmpc_sensor_noise_reset(r, None, p, p, None),
                lambda l: l.frp_nmpc_sensor_noise_depth(r, 1, 2, 2, p, p, None, p, None), lambda l: l.frp_nmpc_sensor_noise_scan(r, 1, 2, p, p, p, None, None, p, None)]

    def bad(what, change):
        n, keep = good_struct()
        change(n)
        for i, c in enumerate(calls(n)):
            out.append((f"{what} [{i}]", c, (n, keep, buf)))

    def setv(field, i, v):
        def f(n):
            getattr(n, field)[i] = v
        return f
    for field in ("sigma_p", "sigma_v", "sigma_a", "bias_c"):
        for v in (-1e-9, float("nan"), float("inf")):
            bad(f"{field} = {v}", setv(field, 1, v))
    for v in (-0.5, 1.5, float("nan")):
        bad(f"bias_a = {v}", setv("bias_a", 2, v))
    for field in ("depth_sigma0", "depth_sigma2", "scan_sigma0", "scan_sigma1"):
        for v in (-1.0, float("nan"), float("inf")):
            bad(f"{field} = {v}", lambda n, field=field, v=v: setattr(n, field, v))
    for field in ("depth_p_drop", "scan_p_drop"):
        for v in (-1e-9, 1.0 + 1e-9, float("nan")):
            bad(f"{field} = {v}", lambda n, field=field, v=v: setattr(n, field, v))
    for v in (0.0, -1000.0, float("nan"), float("inf")):
        bad(f"depth_scale = {v}", lambda n, v=v: setattr(n, "depth_scale", v))
    for v in (0, -3):
        bad(f"B = {v}", lambda n, v=v: setattr(n, "B", v))
    n, keep = good_struct()
    r = ctypes.byref(n)
    own = [("states S = 0", lambda l: l.frp_nmpc_sensor_noise_states(r, 0, p, p, p, 1, None)), ("states x_true NULL", lambda l: l.frp_nmpc_sensor_noise_states(r, 1, None, p, p, 1, None)),
           ("states x_meas NULL", lambda l: l.frp_nmpc_sensor_noise_states(r, 1, p, None, p, 1, None)), ("states n NULL", lambda l: l.frp_nmpc_sensor_noise_states(None, 1, p, p, p, 1, None)),
           ("reset x without y", lambda l: l.frp_nmpc_sensor_noise_reset(r, None, p, None, None)), ("reset y without x", lambda l: l.frp_nmpc_sensor_noise_reset(r, None, None, p, None)),
           ("depth F = 0", lambda l: l.frp_nmpc_sensor_noise_depth(r, 0, 2, 2, p, p, None, p, None)), ("depth F = 65536", lambda l: l.frp_nmpc_sensor_noise_depth(r, 65536, 2, 2, p, p, None, p, None)),
           ("depth rows = 0", lambda l: l.frp_nmpc_sensor_noise_depth(r, 1, 0, 2, p, p, None, p, None)), ("depth cols = -1", lambda l: l.frp_nmpc_sensor_noise_depth(r, 1, 2, -1, p, p, None, p, None)),
           ("depth 2^16 x 2^15 pixels", lambda l: l.frp_nmpc_sensor_noise_depth(r, 1, 65536, 32768, p, p, None, p, None)),
           ("depth in NULL", lambda l: l.frp_nmpc_sensor_noise_depth(r, 1, 2, 2, None, p, None, p, None)), ("depth out NULL", lambda l: l.frp_nmpc_sensor_noise_depth(r, 1, 2, 2, p, None, None, p, None)),
           ("depth tick NULL", lambda l: l.frp_nmpc_sensor_noise_depth(r, 1, 2, 2, p, p, None, None, None)),
           ("scan S = 0", lambda l: l.frp_nmpc_sensor_noise_scan(r, 0, 2, p, p, p, None, None, p, None)), ("scan P = 0", lambda l: l.frp_nmpc_sensor_noise_scan(r, 1, 0, p, p, p, None, None, p, None)),
           ("scan origin NULL", lambda l: l.frp_nmpc_sensor_noise_scan(r, 1, 2, p, p, None, None, None, p, None)), ("scan tick NULL", lambda l: l.frp_nmpc_sensor_noise_scan(r, 1, 2, p, p, p, None, None, None, None))]
    out += [(w, c, (n, keep, buf)) for w, c in own]
    for field in ("bias", "tick"):
        m, keep2 = good_struct()
        setattr(m, field, None)
        rr = ctypes.byref(m)
        out.append((f"states {field} NULL", lambda l, rr=rr: l.frp_nmpc_sensor_noise_states(rr, 1, p, p, p, 1, None), (m, keep2, buf)))
        out.append((f"reset {field} NULL", lambda l, rr=rr: l.frp_nmpc_sensor_noise_reset(rr, None, p, p, None), (m, keep2, buf)))
    return out


def test_the_c_abi_refuses_every_bad_argument_before_it_looks_for_a_device():
    l = solver.lib()
    table = refusals()
    assert len(table) > 150
    for what, call, _ in table:
        assert call(l) == capi.FRP_ERR_ARG, what


def test_the_unit_is_built_like_its_neighbours_and_the_vehicle_has_the_attachment_point():
    import inspect
    assert "frp_sensor_noise.hip" in build.SOURCES and build.PER_SOURCE_FLAGS["frp_sensor_noise.hip"] == ["-ffp-contract=off"]
    src = "\n".join(ln for ln in open(os.path.join(build.CSRC, "frp_sensor_noise.hip")).read().splitlines() if not ln.lstrip().startswith("//"))
    assert '#include "frp_disturbance.hpp"' in src and "__shared__" not in src and "atomic" not in src and "asm" not in src and "__syncthreads" not in src
    names = ["frp_nmpc_sensor_noise_states", "frp_nmpc_sensor_noise_reset", "frp_nmpc_sensor_noise_depth", "frp_nmpc_sensor_noise_scan"]
    i = solver.EXPORTS.index(names[0])
    assert solver.EXPORTS[i:i + 4] == names and all(hasattr(solver.lib(), n) for n in names)
    assert solver.SensorNoise.__module__.endswith(".flight") and capi.C_TYPES[capi.SensorNoiseArgs] == ("frp_nmpc_sensor_noise", "frp_nmpc.h")
    assert "self.noise = None" in inspect.getsource(solver.Vehicle.__init__)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(build.ROOT, doc)).read()
        assert "SensorNoise" in text and "Gauss-Markov" in text and "rolling shutter" in text, doc
