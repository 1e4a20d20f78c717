"""The closed forms of the kinodynamic A* against the mathematics, on the CPU.

tests/golden/astar_mp.npz (tests/tools/gen_astar_mp.py: mpmath at 60 digits, written from the two-point boundary value problem of the
double integrator, not from the code) holds, for 246 state pairs and three (w_time, max_vel) settings, the constrained minimum over
T >= t_bar of the minimum-energy cost J(T) and its minimiser.  oracle/astar_oracle.c and csrc/frp_astar.hip were written one from
the other and are compared to the bit elsewhere (tests/test_gpu_astar*.py); a mistake they share -- a sign in c2, a coefficient of the
quartic -- shows only here.  stateTransit is checked against exact rational arithmetic by tests/astar_referee.py's rule."""
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

from . import astar_lib as AL
from . import astar_referee as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "astar_mp.npz")
TIE = 1.0 + 1.0 / 10000  # kinodynamic_astar.h:139


@pytest.fixture(scope="module")
def fx():
    z = np.load(PATH)
    keys = [str(k) for k in z["result_keys"]]
    out = {k: z[k] for k in ("kind", "x1", "x2", "w_time", "max_vel")}
    out.update({k: z["result"][:, i] for i, k in enumerate(keys)})
    out["tol_measured"] = float(z["tol_measured"].reshape(-1)[0]); out["tol_factor"] = float(z["tol_factor"].reshape(-1)[0]); out["dps"] = int(z["dps"].reshape(-1)[0])
    return out


def _gen():
    pytest.importorskip("mpmath", reason="mpmath is needed to re-evaluate the multiprecision reference")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import gen_astar_mp
    return gen_astar_mp


def test_fixture_covers_what_it_must(fx):
    kinds = fx["kind"].tolist()
    assert 200 <= len(kinds) <= 999 and os.path.getsize(PATH) < 256 * 1024 and fx["dps"] >= 50
    for k in ("generic", "far", "rest", "aligned", "disc"):
        assert kinds.count(k) >= 20, k
    assert len(set(zip(fx["w_time"].tolist(), fx["max_vel"].tolist()))) == 3 and (10.0, 2.0) in set(zip(fx["w_time"].tolist(), fx["max_vel"].tolist()))
    assert (fx["at_t_bar"] == 1).sum() >= 30 and (fx["at_t_bar"] == 0).sum() >= 30     # t_bar active / an interior minimum
    assert (fx["sign_D"] > 0).sum() >= 10 and (fx["sign_D"] < 0).sum() >= 10           # both branches of a closed-form cubic
    disc = np.array([k == "disc" for k in kinds])
    assert (fx["sign_D"][disc] > 0).any() and (fx["sign_D"][disc] < 0).any()
    assert np.any(np.abs(fx["x2"][:, 3:]).max(axis=1) > 0.1) and np.any(np.abs(fx["x2"][:, 3:]).max(axis=1) == 0.0)  # end_v != 0 and == 0
    assert np.all(fx["T_hi"] >= fx["t_bar"]) and np.all(fx["J_hi"] > 0)


def test_generator_meets_the_equation_it_claims_to_solve(fx):
    """For a spread of the committed cases (every kind, every setting): regenerating gives the committed bits; the boundary-value
    evaluation of J equals the closed form; T_min is a root of T^4 J' to 1e-40 of its largest term, or t_bar with J' >= 0 there; and
    no T >= t_bar on a 4000-point grid has a lower J (gen_astar_mp.verify)."""
    G = _gen()
    cases = G.case_list()
    assert len(cases) == len(fx["kind"]) and [c[0] for c in cases] == fx["kind"].tolist()
    picks = sorted({int(np.nonzero(fx["kind"] == k)[0][j]) for k in set(fx["kind"].tolist()) for j in (0, -1)} | {5, 90, 170})
    for i in picks:
        kind, x1, x2, w, vm = cases[i]
        assert np.array_equal(x1, fx["x1"][i]) and np.array_equal(x2, fx["x2"][i]) and w == fx["w_time"][i] and vm == fx["max_vel"][i]
        tb, T, J = G.solve(x1, x2, w, vm)
        assert G.split_double(J) == (fx["J_hi"][i], fx["J_lo"][i]) and G.split_double(T) == (fx["T_hi"][i], fx["T_lo"][i]) and float(tb) == fx["t_bar"][i]
        G.verify(x1, x2, w, vm, T, J)


def _float64_solve(x1, x2, w, max_vel):
    """An independent float64 solve: numpy.roots on T^4 J'(T), J in float64 at the real parts >= t_bar and at t_bar."""
    dp = x2[:3] - x1[:3]; v0, v1 = x1[3:], x2[3:]
    d, s, c = float(dp @ dp), float((v0 + v1) @ dp), float(v0 @ v0 + v0 @ v1 + v1 @ v1)
    tb = float(np.max(np.abs(dp))) / max_vel
    cand = [tb] + [float(r.real) for r in np.roots([w, 0.0, -4.0 * c, 24.0 * s, -36.0 * d]) if r.real >= tb]
    return min(w * T + 12.0 * d / T ** 3 - 12.0 * s / T ** 2 + 4.0 * c / T for T in cand if T > 0.0)


def _rel(value, i, fx):
    J = Fr(float(fx["J_hi"][i])) + Fr(float(fx["J_lo"][i]))
    return float((Fr(value) - J) / J)


def test_heuristic_is_the_constrained_minimum_of_the_energy_cost(fx):
    """estimateHeuristic of the oracle on every case, with cost = (1 + tie_breaker) J(t) as the reference scales it:
      * nothing beats the minimum:  cost >= (1 + tie_breaker) J_min (1 - 2^-40);
      * it IS the minimum:          cost <= (1 + tie_breaker) J_min (1 + tol);
      * the returned time is feasible (>= t_bar).
    tol is not taken from the oracle: the worst relative cost error of an independent float64 solve (numpy.roots on T^4 J', J in
    float64 at the candidates) against the fixture is 1.62e-15 (measured when the fixture was generated, stored in it as tol_measured;
    re-measured here and required to stay within twice that, LAPACK builds differing in the last bits); the oracle gets 8 x the stored
    value = 1.29e-14, Ferrari's closed formulas being less stable than companion-matrix roots.  The oracle's own worst, for the
    record: 1.05e-15 (a `disc` case), lowest -8.5e-16."""
    n = len(fx["kind"])
    measured = max(abs(_rel(_float64_solve(fx["x1"][i], fx["x2"][i], float(fx["w_time"][i]), float(fx["max_vel"][i])), i, fx)) for i in range(n))
    print("float64 solve, worst relative cost error: %.3e (stored %.3e)" % (measured, fx["tol_measured"]))
    assert 0.0 < fx["tol_measured"] < 1e-13 and measured <= 2.0 * fx["tol_measured"] and fx["tol_factor"] == 8.0
    tol = fx["tol_factor"] * fx["tol_measured"]
    worst_hi, worst_lo = -1.0, 1.0
    for i in range(n):
        cost, t = AL.heuristic(fx["x1"][i], fx["x2"][i], float(fx["w_time"][i]), float(fx["max_vel"][i]), TIE)
        rel = _rel(cost / (1.0 + TIE), i, fx)   # (the division's rounding, 1.1e-16, is far inside both bounds)
        worst_hi, worst_lo = max(worst_hi, rel), min(worst_lo, rel)
        assert t >= fx["t_bar"][i], (i, t, fx["t_bar"][i])
        assert rel >= -2.0 ** -40, (i, fx["kind"][i], rel)
        assert rel <= tol, (i, fx["kind"][i], rel, tol)
    print("oracle, relative cost error: %.3e .. %.3e (tol %.3e)" % (worst_lo, worst_hi, tol))


def test_heuristic_time_is_t_bar_or_a_root_the_quartic_reports(fx):
    """The time estimateHeuristic returns is t_bar or one of the (at most four) roots orc_astar_quartic reports for T^4 J', formed
    here from the case the way the mathematics writes it; and where the fixture's minimiser is interior and well separated from
    t_bar, the returned time is that minimiser to 1e-6 relative (J is flat to second order there: a cost error of 1e-14 allows 1e-7)."""
    for i in range(len(fx["kind"])):
        x1, x2, w, vm = fx["x1"][i], fx["x2"][i], float(fx["w_time"][i]), float(fx["max_vel"][i])
        dp = x2[:3] - x1[:3]; v0, v1 = x1[3:], x2[3:]
        d, s, c = float(dp @ dp), float((v0 + v1) @ dp), float(v0 @ v0 + v0 @ v1 + v1 @ v1)
        roots = AL.quartic(w, 0.0, -4.0 * c, 24.0 * s, -36.0 * d)
        cost, t = AL.heuristic(x1, x2, w, vm, TIE)
        assert len(roots) <= 4
        assert t == fx["t_bar"][i] or any(abs(t - r) <= 1e-12 * abs(r) for r in roots), (i, t, roots)
        if fx["at_t_bar"][i] == 0 and fx["kind"][i] != "disc" and fx["T_hi"][i] > 1.05 * fx["t_bar"][i]:
            assert abs(t - fx["T_hi"][i]) <= 1e-6 * fx["T_hi"][i], (i, t, fx["T_hi"][i])


def test_state_transit_against_exact_rational_arithmetic():
    """orc_astar_transit on random states, inputs, external accelerations and durations: every component within 4 ulp of the largest
    term of its exact value (tests/astar_referee.py derives the count: six roundings, < 4 ulp)."""
    rng = np.random.default_rng(17)
    for _ in range(400):
        s0 = np.r_[rng.uniform(-10, 10, 3), rng.uniform(-2, 2, 3)]
        um = rng.choice([-3.0, -1.5, 0.0, 1.5, 3.0], 3) if rng.random() < 0.5 else rng.uniform(-3, 3, 3)
        ext = rng.uniform(-1.5, 1.5, 3) * (rng.random() < 0.8)
        tau = float(rng.choice([0.0625, 0.25, 0.5, 0.8, rng.uniform(0.0, 1.0)]))
        s1 = AL.transit(ext, s0, um, tau)
        p, v, Lp, Lv = R._transit(s0, um, ext, tau)
        for k in range(3):
            assert abs(Fr(float(s1[k])) - p[k]) <= 4 * Fr(R._ulp(Lp[k])) and abs(Fr(float(s1[3 + k])) - v[k]) <= 4 * Fr(R._ulp(Lv[k]))
