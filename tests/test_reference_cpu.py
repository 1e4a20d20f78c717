"""CPU tests of the stage-reference and mode-switch oracle (oracle/reference_oracle.py) against tests/golden/reference_mp.npz (50 digits,
tests/tools/gen_reference_mp.py), against the oracle as it was before the conversion was stated, against a hand-worked table, and
against two closed forms.  The case table is tests/reference_cases.py; its census is asserted here."""
import math
import sys
from fractions import Fraction as F

import numpy as np
import pytest

from . import oracle_lib as OL
from . import reference_cases as RC
from . import reference_fixture as RF

sys.path.insert(0, OL.ROOT)
from oracle import reference_oracle as R     # noqa: E402


def old_references_one(kino_path, kino_size, time_offset, mpc_output, N, Ts=0.05):
    """references_one as it stood before the conversion was stated: `int(q) & 0xFFFFFFFF`."""
    ref_pos = np.zeros((N, 3)); ref_yaw = np.zeros(N)
    last_yaw = float(mpc_output[1, 16])
    replan = False
    for index in range(N):
        index_time = index * Ts + time_offset
        kino_index = int(index_time / Ts) & 0xFFFFFFFF
        if kino_index + 1 < kino_size:
            pos = kino_path[kino_index] + math.fmod(index_time, Ts) / Ts * (kino_path[kino_index + 1] - kino_path[kino_index])
        else:
            pos = kino_path[kino_size - 1]
        fwd = kino_path[kino_index + 5] if kino_index + 5 < kino_size else kino_path[kino_size - 1]
        d = fwd - pos
        yaw_temp = math.atan2(d[1], d[0]) if np.linalg.norm(d) > 0.1 else last_yaw
        if abs(yaw_temp - last_yaw) > R.PI:
            yaw = yaw_temp - 2 * R.PI if yaw_temp > 0 else yaw_temp + 2 * R.PI
        else:
            yaw = yaw_temp
        yaw = 0.2 * last_yaw + 0.8 * yaw
        last_yaw = yaw
        ref_pos[index] = pos; ref_yaw[index] = yaw
        if index == 0 and np.linalg.norm(pos - mpc_output[1, 8:11]) > 1.0:
            replan = True
    return ref_pos, ref_yaw, replan


@pytest.fixture(scope="module")
def oracle_results():
    out = {}
    for c in RC.cases():
        trace = []
        pos, yaw, replan = R.references_one(c.path, c.eff_size, c.off, c.plan(), c.N, c.Ts, trace=trace)
        out[c.index] = (pos, yaw, replan, trace)
    return out


def test_fixture_belongs_to_this_case_table():
    fx = RF.load()
    fx.inputs_match(RC.cases())
    g = fx.g
    assert int(g["dps"].reshape(-1)[0]) == 50 and float(g["margin"].reshape(-1)[0]) == 1e-9
    refuse = 1e-9 * (1 - 1e-6)
    exact = np.concatenate([np.full(c.N, c.family == "direction_exact") for c in RC.cases()])
    assert np.all(g["margins"][exact][:, 0] == 0) and exact.sum() == 2                     # ON the threshold, by construction
    m = np.where(exact[:, None] & (np.arange(2) == 0), 1.0, g["margins"])
    assert m.min() >= refuse * (1 - 2.0 ** -23) and g["case_replan_margin"].min() >= refuse * (1 - 2.0 ** -23)   # stored as float32
    assert len(g["ki"]) == sum(c.N for c in RC.cases())


def test_paths_of_the_sample_cases_have_distinct_samples():
    """A wrong ki or ki + 5 moves ref_yaw by more than 1e-3 on the paths of the on-grid and end-of-path cases."""
    for pid in ("grid", "grid_cw", "k30", "k30_cw", "k40", "k80"):
        ok, move = RC.direction_distinct(RC.PATHS[pid])
        assert ok, (pid, move)


def test_census_every_branch_is_taken():
    n = RC.census(R)
    print("\ncensus of tests/reference_cases.py (%d cases, %d launches):" % (len(RC.cases()), len(RC.launches())))
    for k in sorted(n):
        print("  %-28s %6d" % (k, n[k]))
    empty = [k for k, v in n.items() if v == 0]
    assert not empty, empty
    for Ts in RC.TS_ALL:
        assert n["grid_below_%g" % Ts] >= 50 and n["grid_equal_%g" % Ts] >= 50, (Ts, n["grid_below_%g" % Ts], n["grid_equal_%g" % Ts])
    assert all(L.B <= 64 for L in RC.launches())
    fam = {c.family for c in RC.cases()}
    assert fam >= {"grid", "grid_ulp", "negative", "hostile", "end", "size", "size_shared", "k1", "horizon", "direction", "hold", "unwrap", "unwrap_held",
                   "seed", "replan", "replan_stage0", "coord", "straight", "direction_exact"}


def test_oracle_takes_the_fixtures_decisions(oracle_results):
    """Branch per stage and the replan flag: the oracle's doubles decide as exact arithmetic on the same inputs does."""
    fx = RF.load()
    for c in RC.cases():
        pos, yaw, replan, trace = oracle_results[c.index]
        ki, bits, w = fx.field(c, "ki"), fx.field(c, "branch"), fx.field(c, "w")
        assert replan == fx.replan(c), c.name
        it, q = RC.stage_quotients(c)
        for i, (k, interp, ahead, far, unwrap) in enumerate(trace):
            b = int(bits[i])
            hostile = bool(b & RF.B_HOSTILE)
            assert hostile == (not RC.in_range(q[i])), (c.name, i)
            if not hostile:
                assert k == int(ki[i]), (c.name, i, k, int(ki[i]))
                if interp:
                    assert math.fmod(it[i], c.Ts) / c.Ts == w[i], (c.name, i)
            want = (bool(b & RF.B_INTERP), bool(b & RF.B_AHEAD), bool(b & RF.B_FAR), -1 if b & RF.B_MINUS else 1 if b & RF.B_PLUS else 0)
            assert (interp, ahead, far, unwrap) == want, (c.name, i, (interp, ahead, far, unwrap), want)


def test_oracle_positions_and_yaw_against_50_digits(oracle_results):
    """ref_pos = a + w (b - a) with w the fixture's own double: fl(b - a), one multiply, one add, so
        |err| <= u |r| + 2 u |w (b - a)| (1 + u)^2,  u = 2^-53,
    which is within 2 ulp of the result wherever the step w (b - a) does not cancel a (|w (b - a)| <= |r|); where it does (a coordinate
    that crosses zero) only the absolute bound can hold.  Both are asserted.  ref_yaw: the error is measured per Ts, printed, and held
    to the table of tests/reference_fixture.py, the base of the kernel's tolerance."""
    fx = RF.load()
    u = 2.0 ** -53
    worst = {k: 0.0 for k in RF.ORACLE_ERR}
    cancel = total = 0
    for c in RC.cases():
        pos, yaw, _, trace = oracle_results[c.index]
        hi, lo = fx.field(c, "pos_hi"), fx.field(c, "pos_lo").astype(np.float64)
        w = fx.field(c, "w")
        err = np.abs((pos - hi) - lo)
        for i, t in enumerate(trace):
            step = np.abs(w[i] * (c.path[t[0] + 1] - c.path[t[0]])) if t[1] else np.zeros(3)
            bound = (u * np.abs(hi[i]) + 2 * u * step) * (1 + 1e-9)
            assert np.all(err[i] <= bound), (c.name, i, err[i], bound)
            plain = step <= np.abs(hi[i])
            assert np.all(err[i][plain] <= 2 * np.spacing(np.abs(hi[i][plain]))), (c.name, i)
            cancel += int(np.sum(~plain)); total += 3
        e = RF.yaw_err(yaw, fx.field(c, "yaw_hi"), fx.field(c, "yaw_lo"))
        worst[RF.err_key(c)] = max(worst[RF.err_key(c)], float(e.max()))
    print("\nref_pos: %d of %d components where the step cancels the sample (absolute bound only)" % (cancel, total))
    assert 100 * cancel <= total, (cancel, total)                          # the plain 2 ulp must stay the rule: at most 1 % left to the absolute bound
    print("ref_yaw, oracle against 50 digits, max |err| / max(1, |yaw|) per Ts (and over the 'coord' family):")
    for k in worst:
        print("  %-6s %.3g   (table %.3g)" % (k, worst[k], RF.ORACLE_ERR[k]))
    for k in worst:
        assert worst[k] <= RF.ORACLE_ERR[k], (k, worst[k])                  # the table is this measurement, rounded up


def test_old_oracle_against_new_oracle():
    """Bit-equal wherever every stage's quotient is in (-1, 2**31); different at (2**32 + 3) Ts; no exception for nan / inf."""
    same = 0
    for c in RC.cases():
        _, q = RC.stage_quotients(c)
        if all(x == x and -1.0 < x < 2.0 ** 31 for x in q):
            new = RC.oracle_case(R, c)
            old = old_references_one(c.path, c.eff_size, c.off, c.plan(), c.N, c.Ts)
            assert np.array_equal(new[0], old[0]) and np.array_equal(new[1], old[1]) and new[2] == old[2], c.name
            same += 1
    assert same > 800
    path, plan = RC.PATHS["k40"], np.zeros((21, 17))
    off = (2 ** 32 + 3) * 0.05
    new = R.references_one(path, 40, off, plan, 20)
    old = old_references_one(path, 40, off, plan, 20)
    assert np.array_equal(new[0], np.tile(path[-1], (20, 1))) and not np.array_equal(new[0], old[0])
    assert np.linalg.norm(old[0][0] - path[3]) < 1e-6                   # the old mask wrapped 2**32 + 3 to sample 3
    for off in (math.nan, math.inf, -math.inf):
        with pytest.raises((ValueError, OverflowError)):
            old_references_one(path, 40, off, plan, 20)
        pos, yaw, replan = R.references_one(path, 40, off, plan, 20)
        assert np.array_equal(pos, np.tile(path[-1], (20, 1))) and np.all(yaw == 0.0)


def test_conversions_as_stated():
    assert R.cvttsd2si(3.99) == 3 and R.cvttsd2si(-0.99) == 0 and R.cvttsd2si(-1.0) == 0xFFFFFFFF and R.cvttsd2si(-3.7) == 0xFFFFFFFD
    assert R.cvttsd2si(2.0 ** 31 - 0.5) == 2 ** 31 - 1 and R.cvttsd2si(-2.0 ** 31 - 0.5) == 0x80000000
    for q in (2.0 ** 31, -2.0 ** 31 - 1.0, 2.0 ** 32 + 3, 1e300, -1e300, math.inf, -math.inf, math.nan):
        assert R.cvttsd2si(q) == 0x80000000, q
    assert [R.cvt_i32_f64(q) for q in (3.99, -3.99, 2.0 ** 31 - 0.5, 2.0 ** 31, 1e300, math.inf, -2.0 ** 31 - 0.5, -1e300, -math.inf, math.nan)] == \
        [3, -3, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, -2 ** 31, -2 ** 31, 0]


def test_mode_one_against_the_hand_worked_table():
    for N, Ts, radius, off, size, last, end, want, why in RC.MODE_TABLE:
        plan = np.zeros((N + 1, 17)); plan[N - 1, 8:11] = last
        plan[N, 8:11] = end; plan[0, 8:11] = end                        # the rows the rule must NOT read sit on the goal
        assert R.mode_one(plan, off, size, np.array(end, dtype=float), N, Ts, radius) == want, why
    # the starred rows, with exact fractions: each IEEE operation rounded once
    fl = lambda x: x.numerator / x.denominator
    q = fl(F(fl(F(fl(F(20) * F(0.05))) + F(0.05))) / F(0.05))
    assert q == 21.0
    q = fl(F(fl(F(fl(F(20) * F(0.05))) + F(-2.0))) / F(0.05))
    assert q == -20.0
    assert {r[7] for r in RC.MODE_TABLE} == {True, False} and len(RC.MODE_TABLE) >= 20


def test_mode_groups_cover_both_outcomes_by_both_disjuncts():
    n = dict(index=0, radius=0, neither=0, sticky=0, nonfinite=0)
    for g in RC.mode_groups():
        want = g.expect(R)
        assert g.B in RC.MODE_B or g.B == 64
        for b in range(g.B):
            size = int(g.sizes[b if g.size_per else 0])
            mi = R.cvt_i32_f64((g.N * g.Ts + g.off[b]) / g.Ts)
            e = g.end_pt[b] if g.end_per else g.end_pt
            near = np.linalg.norm(g.plans[b, g.N - 1, 8:11] - e) < g.radius
            n["index"] += mi >= size and not near; n["radius"] += bool(near) and mi < size; n["neither"] += not near and mi < size
            n["sticky"] += g.mode_in[b] == RC.MODE_FINAL and not near and mi < size and want[b] == RC.MODE_FINAL
            n["nonfinite"] += not math.isfinite(g.off[b])
    assert all(v > 0 for v in n.values()), n


def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath


@pytest.mark.parametrize("Ts", RC.TS_ALL)
def test_closed_form_on_a_straight_path(Ts):
    """yaw_k = theta (1 - 0.2^(k+1)) + 0.2^(k+1) yaw0, theta the 50-digit atan2 of the path's step."""
    mp = _mp()
    c = next(c for c in RC.cases() if c.name == "straight_%g" % Ts)
    pos, yaw, _ = RC.oracle_case(R, c)
    step = c.path[1] - c.path[0]
    theta = mp.atan2(mp.mpf(float(step[1])), mp.mpf(float(step[0])))
    for k in range(c.N):
        g = mp.mpf(2) ** (k + 1) / mp.mpf(10) ** (k + 1)
        want = theta * (1 - g) + g * mp.mpf(c.yaw0)
        assert abs(mp.mpf(float(yaw[k])) - want) < mp.mpf(10) ** -14, (k, float(yaw[k]), want)   # step rounded to 1 ulp of 0.1: 1e-16 rad; filter constants 6e-17
    assert np.allclose(pos[:, 0] * 0.08, pos[:, 1] * 0.06, rtol=0, atol=1e-15)                  # on the line


@pytest.mark.parametrize("sign", [1, -1], ids=["ccw", "cw"])
def test_closed_form_on_a_circle_through_the_seam(sign):
    """Samples on a circle, a constant angle `a` apart, weight 1/2: the look-ahead direction is phi_k = phi_0 + k a, and the first-order
    filter y_k = y_{k-1} / 5 + 4 phi_k / 5 has the closed form
        y_k = phi_0 + k a - a / 4 + (yaw0 - phi_0 + 5 a / 4) / 5^(k+1)           (steady-state lag a / 4)
    until phi_k leaves (-pi, pi]: from that stage k_s on atan2 wraps by -+2 pi and the unwrap puts back +-2 PI with PI = 3.1415926, a
    step of -+(2 pi - 2 PI) in the filter's input: y_k -= +-(2 pi - 2 PI) (1 - 1 / 5^(k - k_s + 1))."""
    mp = _mp()
    K, N, Ts, a = 60, 40, 0.05, mp.mpf(8) / 100
    start = mp.mpf(1) / 2
    path = np.array([[float(2 * mp.cos(start + sign * a * k)), float(2 * mp.sin(start + sign * a * k)), 1.0] for k in range(K)])
    plan = np.zeros((N + 1, 17))
    P = [[mp.mpf(v) for v in row] for row in path]
    mid = [(P[3][j] + P[4][j]) / 2 for j in range(3)]
    phi0 = mp.atan2(P[8][1] - mid[1], P[8][0] - mid[0])
    yaw0 = float(phi0) - 0.3 * sign
    plan[1, 16] = yaw0
    trace = []
    pos, yaw, _ = R.references_one(path, K, 3.5 * Ts, plan, N, Ts, trace=trace)
    assert [t[0] for t in trace] == list(range(3, 3 + N))
    ks = next(k for k in range(N) if abs(phi0 + sign * a * k) > mp.pi)
    assert 5 < ks < N - 5 and [t[4] for t in trace] == [0] * ks + [sign] * (N - ks)
    s = 2 * mp.pi - 2 * mp.mpf(R.PI)
    for k in range(N):
        # the continuous angle is kept: past the seam the filtered yaw runs beyond +-pi instead of wrapping
        want = phi0 + sign * a * k - sign * a / 4 + (mp.mpf(yaw0) - phi0 + sign * 5 * a / 4) / mp.mpf(5) ** (k + 1)
        if k >= ks:
            want -= sign * s * (1 - 1 / mp.mpf(5) ** (k - ks + 1))
        assert abs(mp.mpf(float(yaw[k])) - want) < mp.mpf(10) ** -12, (k, float(yaw[k]), want)
