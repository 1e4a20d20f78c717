"""Tube propagation against a 50-digit evaluation, on the CPU.

tests/golden/tube_mp.npz (tests/tools/gen_tube_mp.py, mpmath at 80 working digits, a third method) says what the mathematics
of NMPCSolver::setFORCESParams gives for 43 plans / constants / horizons; this file checks, without a GPU,
  * the generator against the equation it claims to solve (needs mpmath; skipped with that reason without it),
  * oracle/tube_oracle.py against the fixture: its measured error per Ts group is in tests/tube_fixture.py, asserted x 10,
  * the kernel's own arithmetic (csrc/frp_tube_math.hpp, compiled for the host into tests/cpp/tube_harness) against the fixture:
    per-stage Qd, rows of exp(Phi Ts), E -- the guard that fails when a quadrature weight, a Taylor order or a Jacobi sweep drifts.

Measured maxima of the harness (x86-64, no FMA contraction), for the comments beside the bounds below:
    E  by Ts group 0.02 .. 0.3:  1.8e-14  1.1e-13  5.5e-14  1.1e-14  2.9e-14  2.8e-14  3.9e-14   (tolerances 3e-13 .. 4e-11)
    Qd 5.8e-14, rows of exp 3.2e-16 of the largest entry of the stage's matrix.
One panel forced on every stage, same harness: Qd 6e-14 for nu = ||Phi||_1 Ts < 6,
4.7e-12 .. 7.7e-12 in [6, 8), 6.7e-10 in [10, 14), 1.9e-7 in [25, 30); E 1.0e-11 at Ts = 0.2 and 3.8e-8 at Ts = 0.3.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from forces_resilient_planner_amd import layout as L
from forces_resilient_planner_amd import solver

from . import tube_fixture as TF

ROOT = TF.ROOT
sys.path.insert(0, ROOT)
CASES = TF.load()


def _gen():
    pytest.importorskip("mpmath", reason="mpmath is needed to re-evaluate the multiprecision reference")
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import gen_tube_mp
    return gen_tube_mp


# ---- the fixture itself -----------------------------------------------------------------------------------------------------------
def test_fixture_covers_what_it_must():
    by = {c.name: c for c in CASES}
    lb, ub = L.bounds()
    assert 20 <= len(CASES) <= 99 and os.path.getsize(TF.PATH) < 512 * 1024
    assert sorted({c.N for c in CASES if c.name.startswith("horizon")}) == [1, 20, 21, 22, 42, 43, 63, 64]
    assert sorted({c.Ts for c in CASES}) == [0.02, 0.05, 0.08, 0.1, 0.15, 0.2, 0.3]
    for Ts in (0.02, 0.05, 0.08, 0.1, 0.15, 0.2, 0.3):
        e, t3 = by[f"Ts{Ts:g}_edge"], by[f"Ts{Ts:g}_t3"]
        assert np.all(np.abs(e.plan[:, 14:16]) == 0.4 * np.pi) and np.all(e.plan[:, 3] == ub[3]) and np.all(t3.plan[:, 3] == 3 * ub[3])
    assert np.all(by["tmin20"].plan[:, 3] == lb[3])
    assert by["noise_aniso"].consts["noise"] == (1e-3, 1.0, 1.0) and by["eps_small"].consts["epsilon"] == 1e-4 and by["eps_one"].consts["epsilon"] == 1.0
    assert by["ego_flat"].consts["ego_h"] * 100 < by["ego_flat"].consts["ego_r"] and by["mass_drag"].consts["mass"] != 0.74
    rnd = np.concatenate([c.plan for c in CASES if c.name.startswith("horizon")])
    assert np.abs(rnd[:, 16]).max() > 3.0 and np.abs(rnd[:, 11:14]).max() > 5.5
    assert min(c.lam_min.min() for c in CASES) >= 1e-3      # the generator refuses below: the Sylvester equation would be singular
    for c in CASES:
        assert np.isfinite(c.E).all() and np.linalg.eigvalsh(c.E).min() > 0 and np.max(np.abs(c.E - np.swapaxes(c.E, -1, -2))) < 1e-15


def test_generator_satisfies_the_sylvester_equation_and_the_root():
    """The Gramian integral solves  Phi X + X Phi' = N - e^{-Phi t} N e^{-Phi' t}  and E E is the Minkowski sum, both to 1e-40
    (relative to the largest entry of the right-hand side), at Ts = 0.05 and at the far end (Ts = 0.3, three times the thrust bound)."""
    G = _gen()
    mp = G._mp()
    by = {c.name: c for c in CASES}
    for name, stages in (("Ts0.05_rand", (0, 3)), ("Ts0.3_t3", (1,)), ("Ts0.15_edge", (2,))):
        cs = by[name]
        t = mp.mpf(cs.consts["Ts"])
        for k in stages:
            Phi, R, Xs, Qd, Ep = G.stage_mp(cs.plan[k], cs.consts)
            Em = G.expm_mp(-Phi * t)
            assert G.norm1(Em * Ep - mp.eye(9)) < mp.mpf(10) ** -40
            for i, X in enumerate(Xs):
                Nm = mp.zeros(9, 9); Nm[3 + i, 3 + i] = t * mp.mpf(cs.consts["noise"][i]) ** 2
                W = Nm - Em * Nm * Em.T
                res = Phi * X + X * Phi.T - W
                assert G.norm1(res) < mp.mpf(10) ** -40 * max(1, G.norm1(W)), (name, k, i, mp.nstr(G.norm1(res), 5))
    cs = by["Ts0.05_rand"]
    E, Qd, Gm, nu1, lam, det = G.tube_one_mp(cs.plan, cs.consts, details=True)
    for Q, Em in det:
        assert G.norm1(Em * Em - Q) < mp.mpf(10) ** -40 * G.norm1(Q)
        assert G.norm1(Em - Em.T) < mp.mpf(10) ** -60
    assert np.array_equal(E, cs.E) and np.array_equal(Qd, cs.Qd) and np.array_equal(Gm, cs.G)


def test_regenerating_a_case_reproduces_the_committed_bits():
    G = _gen()
    cases = G.case_list()
    assert [c[0] for c in cases] == [c.name for c in CASES]
    for idx in [i for i, c in enumerate(CASES) if c.name in ("horizon1", "Ts0.3_warm")]:   # inputs (plans, constants) and outputs
        case, cs = cases[idx], CASES[idx]
        z, E, Qd, Gm, nu1, lam = G.run_case(case)
        assert np.array_equal(z, cs.plan) and np.array_equal(G.consts_row(case[4]), cs.consts_row)
        assert np.array_equal(E, cs.E) and np.array_equal(Qd, cs.Qd) and np.array_equal(Gm, cs.G) and np.array_equal(nu1, cs.nu1)
        assert np.allclose(lam, cs.lam_min, rtol=1e-12)


# ---- the FP64 oracle against the fixture --------------------------------------------------------------------------------------
def test_oracle_error_against_the_multiprecision_reference():
    """oracle/tube_oracle.py on every case; per Ts group the largest |E - E_mp| / (1e-3 + |E_mp|) is the ORACLE'S MEASURED
    ERROR (tests/tube_fixture.py: 2.1e-14 .. 3.4e-12), asserted at ten times that, rounded up to one digit."""
    from oracle import tube_oracle as T
    worst = {}
    for c in CASES:
        worst[c.Ts] = max(worst.get(c.Ts, 0.0), TF.rel_E(T.tube_one(c.plan, c.consts), c.E))
    print("oracle vs 50 digits, by Ts:", {k: f"{v:.2e}" for k, v in sorted(worst.items())})
    for Ts, w in worst.items():
        assert w < TF.TOL[Ts], (Ts, w)


def test_oracle_closed_forms_are_the_generators():
    """Phi and R of the oracle (float64) and of the generator (80 digits) are the same closed forms: they differ by rounding."""
    G = _gen()
    from oracle import tube_oracle as T
    for c in (CASES[1], CASES[-2]):
        for k in (0, c.N - 1):
            Phi, R = T.update_matrix(c.plan[k, 14:17], c.plan[k, 11:14], c.plan[k, 3], c.consts)
            Pm, Rm = G.update_matrix_mp(c.plan[k], c.consts)
            Pm = np.array([[float(Pm[i, j]) for j in range(9)] for i in range(9)]); Rm = np.array([[float(Rm[i, j]) for j in range(3)] for i in range(3)])
            assert np.max(np.abs(Phi - Pm)) < 1e-13 * np.abs(Pm).max() and np.max(np.abs(R - Rm)) < 1e-15
            assert abs(np.linalg.norm(Phi, 1) * c.Ts - c.nu1[k]) < 1e-13 * c.nu1[k]


# ---- the kernel's arithmetic, compiled for the CPU ------------------------------------------------------------------------------
def _harness():
    exe = os.path.join(ROOT, "tests", "cpp", "tube_harness")
    src = exe + ".cpp"
    deps = [src, os.path.join(ROOT, "include", "frp_nmpc.h"), os.path.join(ROOT, "forces_resilient_planner_amd", "csrc", "frp_tube_math.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", src, "-o", exe])
    return exe


def _run_harness(tmp_path, cases, force_panels=0):
    fin, fout = str(tmp_path / "tube_in.bin"), str(tmp_path / "tube_out.bin")
    with open(fin, "wb") as f:
        np.array([len(cases)], dtype=np.int32).tofile(f)
        for c in cases:
            np.array([c.N, force_panels], dtype=np.int32).tofile(f)
            np.ascontiguousarray(c.consts_row, dtype=np.float64).tofile(f)
            np.ascontiguousarray(c.plan, dtype=np.float64).tofile(f)
    subprocess.check_call([_harness(), fin, fout])
    o = np.fromfile(fout).reshape(-1, 83)
    out, s = [], 0
    for c in cases:
        r = o[s:s + c.N]; s += c.N
        out.append(dict(E=r[:, :9].reshape(-1, 3, 3), Qd=r[:, 9:54], G=r[:, 54:81].reshape(-1, 3, 9), nu=r[:, 81], panels=r[:, 82]))
    return out


def _norm_err(a, b):
    """per stage: largest entry of the difference over the largest entry of the stage's matrix"""
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    return np.max(np.abs(a - b), axis=1) / np.max(np.abs(b), axis=1)


def test_kernel_arithmetic_on_the_cpu_meets_the_fixture(tmp_path):
    """E to the kernel's tolerance (the oracle's measured error of the Ts group, times ten).  Per stage, Qd to 3e-13 of its
    largest entry -- the tightest E tolerance: Qd enters E at its own relative size, so a Qd that is further off cannot be
    relied on to meet it -- and the rows of exp(Phi Ts) to 1e-13: at most 2 x 16 Taylor steps of ||h Phi||_1 <= 2.5, each of which
    can lose exp(2.5) ~ 12 roundings to cancellation, 32 x 12 x 2.2e-16.  Every stage of the fixture is inside the domain."""
    res = _run_harness(tmp_path, CASES)
    worstE, worstQ, worstG = {}, 0.0, 0.0
    for c, r in zip(CASES, res):
        assert np.all(r["panels"] >= 1) and np.all(r["panels"] == np.maximum(1, np.ceil(r["nu"] / 5.0)))
        assert np.max(np.abs(r["nu"] - c.nu1)) < 1e-12 * c.nu1.max()            # the device's norm bound is ||Phi||_1 Ts itself
        worstE[c.Ts] = max(worstE.get(c.Ts, 0.0), TF.rel_E(r["E"], c.E))
        worstQ = max(worstQ, _norm_err(r["Qd"], c.Qd).max()); worstG = max(worstG, _norm_err(r["G"], c.G).max())
    print("kernel arithmetic (CPU) vs 50 digits: E by Ts", {k: f"{v:.2e}" for k, v in sorted(worstE.items())}, f"Qd {worstQ:.2e} exp rows {worstG:.2e}")
    for Ts, w in worstE.items():
        assert w < TF.TOL[Ts], (Ts, w)
    assert worstQ < 3e-13 and worstG < 1e-13


def test_one_panel_is_not_enough_beyond_its_domain(tmp_path):
    """What the panels are for: with ONE panel forced the Ts >= 0.2 cases with three times the
    thrust bound miss the tolerance by decades (measured: E 1.0e-11 at Ts = 0.2, 3.8e-8 at 0.3) -- silently."""
    far = [c for c in CASES if c.name in ("Ts0.2_t3", "Ts0.3_t3")]
    res = _run_harness(tmp_path, far, force_panels=1)
    for c, r in zip(far, res):
        assert c.nu1.max() > 20 and TF.rel_E(r["E"], c.E) > 10 * c.tol, (c.name, TF.rel_E(r["E"], c.E))


def test_in_bounds_plans_stay_under_the_launchers_norm_bound_and_keep_one_panel():
    """include/frp_nmpc.h derives phi1 >= ||Phi||_1 for plans inside the stage bounds; check it on random in-bounds plans (corners
    included), and that such plans have a single panel (nu <= 5) up to Ts = 0.1 -- the range whose arithmetic must not change."""
    from oracle import tube_oracle as T
    lb, ub = L.bounds()
    rng = np.random.default_rng(7)
    r3 = np.sqrt(3.0)
    for mass, drag in ((0.74, 0.33), (1.3, 0.1), (0.4, 0.6)):
        phi1 = max(9.0, 8 * r3 / mass, 7 + r3 * drag, 1 + r3 * (drag + 6 / mass), 8 + r3 * (14.62315878 / mass + 2 * drag * 2 * r3))
        worst = 0.0
        for i in range(400):
            z = lb + (ub - lb) * (rng.random(17) if i % 2 else rng.integers(0, 2, 17))
            Phi, _ = T.update_matrix(z[14:17], z[11:14], z[3], dict(mass=mass, drag=drag))
            worst = max(worst, np.linalg.norm(Phi, 1))
        assert worst <= phi1, (mass, drag, worst, phi1)
        if mass == 0.74:
            assert abs(phi1 - 46.2) < 0.05 and worst * 0.1 <= 5.0


def test_launcher_refuses_a_sampling_time_outside_the_domain():
    """Ts * phi1 > 16 panels x 5: FRP_ERR_ARG on the host, before anything is launched (the limit is 1.73 at the defaults)."""
    l = solver.lib()
    tb = solver.Tube(4, 20, 8, 0.74, 0.33, 0.27, 0.0425, (ctypes.c_double * 3)(0.5, 0.5, 0.5), 0.06, 1.75, 8)
    assert l.frp_nmpc_tube_batch(ctypes.byref(tb), None) == -1003
    tb.Ts = float("nan")
    assert l.frp_nmpc_tube_batch(ctypes.byref(tb), None) == -1003
    tb.Ts = 0.2; tb.mass = 0.05   # the same thrust bound on a light vehicle: 8 + sqrt(3) (292 + ...) = 519 per second
    assert l.frp_nmpc_tube_batch(ctypes.byref(tb), None) == -1003
