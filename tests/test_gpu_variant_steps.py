"""Every instantiation of the LDS-resident solver kernel against the oracle, iterate by iterate.

The end-of-solve parity tests compare converged points, which a wrong step direction (a wrong second derivative, a wrong
theta weight) still reaches.  Here each kernel instantiation -- asserted by name through frp_nmpc_solver_variant, the
launch's own selection -- runs with maxit = k for k in K and is compared with the oracle after as many iterations: flags,
iteration counts, the Gauss-Newton redo counter (info[7] against nfallback), the iterate z and the step diagnostics
mu / mu_aff / sigma / step_aff.  CASES lists, per instantiation, the launch that selects it; B is picked relative to the
device's CU count.  tests/test_capi_cpu.py checks that CASES names every instantiation the built library holds."""
import numpy as np
import pytest

from forces_resilient_planner_amd import solver, workloads

from . import oracle_lib as OL

pytestmark = pytest.mark.gpu

K = (1, 2, 3, 5, 8)

# name -> (workload, N, M, model, B as a function of the CU count C, twisted, frp_nmpc_set_q4_min_batch value)
# B <= 2 C: the small-launch builds (lr2); B > 2 C: the three-per-CU builds (lr); q4 min 0: the high-residency builds (lrq, lrs).
# "hard": workloads.config_hard (N = 20, at most 6 live rows, some exact-Hessian factorisations fail: the theta path).
CASES = {
    "frp::lr::nmpc_ipm_lds_kernel<20, 2, true, 3, false>": ("c3", 20, 6, 0, lambda C: 2 * C + 8, False, -1),
    "frp::lr::nmpc_ipm_lds_kernel<20, 5, true, 3, false>": ("c3", 20, 15, 1, lambda C: 2 * C + 8, False, -1),
    "frp::lr::nmpc_ipm_lds_kernel<20, 2, true, 3, true>": ("c3", 20, 6, 0, lambda C: 2 * C + 8, True, -1),
    "frp::lr::nmpc_ipm_lds_kernel<20, 5, true, 3, true>": ("c3", 5, 15, 1, lambda C: 2 * C + 8, True, -1),
    "frp::lr::nmpc_ipm_lds_kernel<20, 10, false, 3, false>": ("c3", 20, 30, 0, lambda C: 2 * C + 8, False, -1),
    "frp::lr::nmpc_ipm_lds_kernel<20, 10, false, 3, true>": ("c3", 20, 30, 1, lambda C: 2 * C + 8, True, -1),
    "frp::lr::nmpc_ipm_lds_kernel<32, 3, true, 2, false>": ("c3", 21, 6, 0, lambda C: 64, False, -1),
    "frp::lr::nmpc_ipm_lds_kernel<32, 8, true, 2, false>": ("c3", 32, 16, 0, lambda C: 64, False, -1),
    "frp::lr::nmpc_ipm_lds_kernel<32, 15, false, 2, false>": ("c3", 21, 30, 1, lambda C: 48, False, -1),
    "frp::lr::nmpc_ipm_lds_kernel<64, 8, true, 1, false>": ("c3", 33, 8, 0, lambda C: 24, False, -1),
    "frp::lr::nmpc_ipm_lds_kernel<64, 30, false, 1, false>": ("c3", 64, 30, 1, lambda C: 24, False, -1),
    "frp::lrq::nmpc_ipm_lds_kernel<20, 2, true, 3, false>": ("c3", 2, 6, 1, lambda C: 64, False, 0),
    "frp::lrs::nmpc_ipm_lds_kernel<30, 8, true, 3, false>": ("c3", 30, 16, 0, lambda C: 64, False, 0),
    "frp::lr2::nmpc_ipm_lds_kernel<20, 2, true, 2, false>": ("hard", 20, 30, 0, lambda C: 128, False, -1),
    "frp::lr2::nmpc_ipm_lds_kernel<20, 5, true, 2, false>": ("c3", 20, 15, 0, lambda C: 64, False, -1),
    "frp::lr2::nmpc_ipm_lds_kernel<20, 10, true, 2, false>": ("c3", 20, 30, 1, lambda C: 64, False, -1),
    "frp::lr2::nmpc_ipm_lds_kernel<20, 2, true, 2, true>": ("c3", 6, 6, 1, lambda C: 64, True, -1),
    "frp::lr2::nmpc_ipm_lds_kernel<20, 5, true, 2, true>": ("c3", 20, 15, 0, lambda C: 64, True, -1),
    "frp::lr2::nmpc_ipm_lds_kernel<20, 10, true, 2, true>": ("c3", 20, 30, 1, lambda C: 64, True, -1),
}

# Tolerances: ten times the maxima measured on the MI355X, rounded up to one digit.  Per case: the |dz| tolerance at each k
# of K (absolute, over the batch), then one relative tolerance for mu / mu_aff / sigma / step_aff over all those k.  The
# comment under each case holds the measured maxima (|dz| per k, the diagnostics), the k = 3 distance between the kernel's
# iterate and the oracle's Gauss-Newton iterate, and that distance in units of the k = 3 tolerance.
# lr<20, 5, true, 3, false> at k = 8: 5.0e-9 is one problem (of 520) that diverges -- stationarity residual 2e6, mu 21 at
# k = 8, the rounding amplified by its large multipliers; the next problem is at 3.5e-11, the median 1.2e-14.
# The twisted instances (..., true>) carry the rounding of the 1e12 penalty that pins x_0 in their direction and drift from
# the oracle's twisted solve as they iterate.  For k <= 3 every flag, iteration count and redo counter is exact and the
# tolerances below apply; at k = 5 and 8 only the agreement of flags / iteration counts / redo counters is checked (at least
# 98 % of the problems; measured 99.2 % on lr<20, 2, true, 3, true>, 100 % elsewhere) and iterates are not compared.  Their
# Gauss-Newton distance is 1e2 .. 2e5 times their k = 3 tolerance, below the 1e3 the plain instances must show, so the
# guard is not applied to them: these cases are a weaker check.  The Hessian code they run is the plain instances'.
TOL = {
    "frp::lr::nmpc_ipm_lds_kernel<20, 2, true, 3, false>": ((6e-13, 2e-12, 2e-12, 2e-12, 2e-12), 8e-08),
        # |dz| 5.4e-14 1.3e-13 1.5e-13 1.7e-13 1.7e-13; diagnostics 7.0e-09; GN 2.7e-01 = 1e+11 x the k = 3 tolerance; agree 1.0000
    "frp::lr::nmpc_ipm_lds_kernel<20, 5, true, 3, false>": ((3e-13, 2e-12, 2e-12, 6e-12, 5e-08), 8e-08),
        # |dz| 2.8e-14 1.6e-13 1.1e-13 5.7e-13 5.0e-09; diagnostics 7.0e-09; GN 2.6e+00 = 1e+12 x the k = 3 tolerance; agree 1.0000
    "frp::lr::nmpc_ipm_lds_kernel<20, 2, true, 3, true>": ((7e-05, 2e-03, 9e-04), 1e-01),
        # |dz| 6.1e-06 1.7e-04 8.2e-05; diagnostics 9.8e-03; GN 2.7e-01 = 3e+02 x the k = 3 tolerance; agree 0.9923
    "frp::lr::nmpc_ipm_lds_kernel<20, 5, true, 3, true>": ((4e-06, 3e-06, 2e-06), 5e-04),
        # |dz| 3.8e-07 2.5e-07 1.1e-07; diagnostics 4.9e-05; GN 2.8e-01 = 1e+05 x the k = 3 tolerance; agree 1.0000
    "frp::lr::nmpc_ipm_lds_kernel<20, 10, false, 3, false>": ((6e-13, 3e-12, 8e-12, 2e-10, 2e-09), 1e-07),
        # |dz| 5.9e-14 2.1e-13 7.8e-13 1.7e-11 1.9e-10; diagnostics 9.4e-09; GN 7.8e-01 = 1e+11 x the k = 3 tolerance; agree 1.0000
    "frp::lr::nmpc_ipm_lds_kernel<20, 10, false, 3, true>": ((2e-05, 3e-03, 3e-03), 2e-01),
        # |dz| 1.8e-06 2.3e-04 2.4e-04; diagnostics 1.6e-02; GN 2.6e+00 = 9e+02 x the k = 3 tolerance; agree 1.0000
    "frp::lr::nmpc_ipm_lds_kernel<32, 3, true, 2, false>": ((3e-13, 2e-12, 2e-12, 2e-12, 2e-12), 8e-08),
        # |dz| 2.5e-14 1.1e-13 1.5e-13 1.1e-13 1.1e-13; diagnostics 7.6e-09; GN 2.2e-01 = 1e+11 x the k = 3 tolerance; agree 1.0000
    "frp::lr::nmpc_ipm_lds_kernel<32, 8, true, 2, false>": ((4e-13, 2e-12, 2e-12, 3e-11, 3e-10), 8e-09),
        # |dz| 3.2e-14 1.2e-13 1.2e-13 2.1e-12 2.1e-11; diagnostics 7.1e-10; GN 3.2e-01 = 2e+11 x the k = 3 tolerance; agree 1.0000
    "frp::lr::nmpc_ipm_lds_kernel<32, 15, false, 2, false>": ((3e-13, 3e-13, 5e-13, 3e-12, 4e-11), 2e-08),
        # |dz| 2.6e-14 2.9e-14 4.3e-14 2.4e-13 3.3e-12; diagnostics 2.0e-09; GN 3.1e-01 = 6e+11 x the k = 3 tolerance; agree 1.0000
    "frp::lr::nmpc_ipm_lds_kernel<64, 8, true, 1, false>": ((2e-13, 7e-13, 4e-12, 6e-12, 6e-11), 3e-08),
        # |dz| 1.1e-14 6.8e-14 3.1e-13 5.8e-13 5.3e-12; diagnostics 2.0e-09; GN 5.0e-01 = 1e+11 x the k = 3 tolerance; agree 1.0000
    "frp::lr::nmpc_ipm_lds_kernel<64, 30, false, 1, false>": ((2e-13, 3e-13, 4e-13, 3e-12, 3e-10), 2e-08),
        # |dz| 1.2e-14 2.4e-14 3.1e-14 2.7e-13 2.0e-11; diagnostics 1.9e-09; GN 5.9e-02 = 1e+11 x the k = 3 tolerance; agree 1.0000
    "frp::lrq::nmpc_ipm_lds_kernel<20, 2, true, 3, false>": ((2e-12, 3e-12, 4e-12, 4e-12, 4e-12), 9e-07),
        # |dz| 1.7e-13 2.1e-13 3.2e-13 3.2e-13 3.2e-13; diagnostics 8.2e-08; GN 5.2e-03 = 1e+09 x the k = 3 tolerance; agree 1.0000
    "frp::lrs::nmpc_ipm_lds_kernel<30, 8, true, 3, false>": ((2e-13, 9e-13, 2e-12, 2e-11, 3e-10), 2e-08),
        # |dz| 1.9e-14 8.3e-14 1.5e-13 1.6e-12 2.3e-11; diagnostics 1.1e-09; GN 2.4e-01 = 1e+11 x the k = 3 tolerance; agree 1.0000
    "frp::lr2::nmpc_ipm_lds_kernel<20, 2, true, 2, false>": ((7e-13, 2e-12, 3e-11, 4e-11, 2e-09), 1e-07),
        # |dz| 6.8e-14 1.7e-13 2.9e-12 3.0e-12 1.2e-10; diagnostics 9.0e-09; GN 8.6e-01 = 3e+10 x the k = 3 tolerance; agree 1.0000
    "frp::lr2::nmpc_ipm_lds_kernel<20, 5, true, 2, false>": ((4e-13, 2e-12, 2e-12, 9e-12, 2e-10), 2e-08),
        # |dz| 3.2e-14 1.2e-13 1.8e-13 8.8e-13 1.7e-11; diagnostics 1.9e-09; GN 5.6e-01 = 3e+11 x the k = 3 tolerance; agree 1.0000
    "frp::lr2::nmpc_ipm_lds_kernel<20, 10, true, 2, false>": ((9e-14, 8e-13, 2e-12, 8e-12, 4e-10), 4e-08),
        # |dz| 8.9e-15 7.8e-14 1.2e-13 7.2e-13 3.2e-11; diagnostics 3.7e-09; GN 2.2e-01 = 1e+11 x the k = 3 tolerance; agree 1.0000
    "frp::lr2::nmpc_ipm_lds_kernel<20, 2, true, 2, true>": ((2e-06, 3e-06, 5e-07), 3e-04),
        # |dz| 1.1e-07 2.0e-07 4.8e-08; diagnostics 2.1e-05; GN 1.1e-01 = 2e+05 x the k = 3 tolerance; agree 1.0000
    "frp::lr2::nmpc_ipm_lds_kernel<20, 5, true, 2, true>": ((6e-05, 2e-03, 5e-03), 4e-02),
        # |dz| 5.6e-06 1.8e-04 4.7e-04; diagnostics 3.4e-03; GN 5.6e-01 = 1e+02 x the k = 3 tolerance; agree 1.0000
    "frp::lr2::nmpc_ipm_lds_kernel<20, 10, true, 2, true>": ((2e-05, 9e-04, 7e-04), 2e-02),
        # |dz| 1.5e-06 8.9e-05 6.5e-05; diagnostics 2.0e-03; GN 2.2e-01 = 3e+02 x the k = 3 tolerance; agree 1.0000
}
GN_FACTOR = 1e3  # plain instances: at k = 3 the kernel's iterate is this many tolerances away from the Gauss-Newton iterate


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _workload(kind, N, M, model, B):
    if kind == "hard":
        w = workloads.config_hard(B, model=model)
        return w, w, int(w["nfaces"].max())
    w = workloads.config3(B, N=N, M=M, model=model)
    wn = dict(w); wn["nfaces"] = None  # (padding detection on the device; MF = M selects the variant)
    return w, wn, M


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-12)))


def measure(name, case=None):
    """Runs one case (CASES[name], or `case`: another launch that selects the instantiation).  Returns (selected kernel name, {k: maxima}, GN distance at k = 3, oracle fallbacks, {k: agreement}):
    agreement = the fraction of problems whose flag, iteration count and redo counter equal the oracle's; the maxima are
    taken over those problems."""
    kind, N, M, model, bfun, tw, q4 = CASES[name] if case is None else case
    B = bfun(_cus())
    w, wn, MF = _workload(kind, N, M, model, B)
    m = 9 * N // 20 if B <= 1024 else 3 * N // 10  # (the kernel's rule for twist = -1, frp_ipm_lds.hip: twist_stages)
    prev = solver.lib().frp_nmpc_set_q4_min_batch(q4)
    try:
        sel = solver.solver_variant(B, w["N"], w["M"], MF, model, solver.default_options(twist=-1 if tw else 0))
        out, exact, fallbacks = {}, {}, 0
        for k in K:
            z, fl, it, info = solver.solve_batch_host(wn, solver.default_options(maxit=k, twist=-1 if tw else 0), MF=MF)
            zo, flo, io = OL.solve_batch(w, OL.default_options(maxit=k, twist=m if tw else 0))
            ito = np.array([i.it for i in io]); nfb = np.array([i.nfallback for i in io])
            fallbacks = max(fallbacks, int((nfb > 0).sum()))
            same = (fl == flo) & (it == ito) & (info[:, 7].astype(int) == nfb)
            exact[k] = float(same.mean())
            s = same  # (the plain instances must agree everywhere; the twisted ones are compared where they do)
            out[k] = dict(z=float(np.max(np.abs(z[s] - zo[s]))),
                          mu=_rel(info[s, 5], np.array([i.mu for i in io])[s]),
                          mu_aff=_rel(info[s, 8], np.array([i.mu_aff for i in io])[s]),
                          sigma=_rel(info[s, 9], np.array([i.sigma for i in io])[s]),
                          step_aff=_rel(info[s, 10], np.array([i.step_aff for i in io])[s]))
            if k == 3:
                zg, _, _ = OL.solve_batch(w, OL.default_options(maxit=k, twist=m if tw else 0, hessian=0))
                gn = float(np.max(np.abs(z - zg)))
    finally:
        solver.lib().frp_nmpc_set_q4_min_batch(prev)
    return sel, out, gn, fallbacks, exact


_FALLBACKS = {}


@pytest.mark.parametrize("name", list(CASES))
def test_every_instantiation_steps_like_the_oracle(name):
    sel, out, gn, fallbacks, agree = measure(name)
    assert sel == name
    tw = CASES[name][5]
    tol_z, tol_rel = TOL[name]
    for i, k in enumerate(K):
        if tw and k > 3:
            assert agree[k] >= 0.98, (k, agree[k])
            continue
        assert agree[k] == 1.0, (k, agree[k])  # flags, iteration counts, info[7] == nfallback: every problem
        assert out[k]["z"] <= tol_z[i], (k, out[k])
        for q in ("mu", "mu_aff", "sigma", "step_aff"):
            assert out[k][q] <= tol_rel, (k, q, out[k])
    if not tw:  # the comparison sees the dynamics Hessian: the Gauss-Newton iterate is far outside the tolerance
        assert gn > GN_FACTOR * tol_z[K.index(3)], gn
    _FALLBACKS[name] = fallbacks


def test_the_theta_path_runs_in_the_step_comparison():
    """At least one case has exact-Hessian factorisations redone with Gauss-Newton within k <= 8, so info[7] against
    nfallback and the reduced theta weight are compared."""
    name = "frp::lr2::nmpc_ipm_lds_kernel<20, 2, true, 2, false>"
    if name not in _FALLBACKS:
        _FALLBACKS[name] = measure(name)[3]
    assert _FALLBACKS[name] > 0
