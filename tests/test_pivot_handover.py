"""The hand-over of the 4 x 4 pivot block of a Riccati stage to the lanes (frp_device.hpp: ldl4_rows -- D^-1 and the pivot test per
16-lane row; the uniform form stays on the plain-layout factor sweep): the solves still step like the oracle on every stage-loop
shape of sweep_factor, a failed pivot still poisons the sweep and is discarded the way the oracle discards it, and the arrival
sweep of the twisted solve agrees with the oracle's twisted solve.

Tolerances are those tests/test_gpu_parity.py uses for the same comparisons: iterates of problems with the oracle's iteration
count within 1e-6 (test_batch_matches_oracle), on the hard family within 1e-5
(test_hip_path_converges_on_the_hard_family_at_default_options)."""
import os

import numpy as np
import pytest

from forces_resilient_planner_amd import layout as L
from forces_resilient_planner_amd import solver, workloads

from . import oracle_lib as OL

pytestmark = pytest.mark.gpu

Q4_KERNEL = "frp::lrq::nmpc_ipm_lds_kernel<20, 2, true, 3, false>"


def _cut(w, N):
    """The first N stages of a workload (both implementations get the same shortened problem)."""
    return dict(w, N=N, x0=w["x0"][:, :N].copy(), params=w["params"][:, :N].copy(), nfaces=w["nfaces"][:, :N].copy())


class _q4:
    """Every launch inside takes the high-residency (four-per-CU) build when its shape has one, whatever the batch size."""

    def __enter__(self):
        self.prev = solver.lib().frp_nmpc_set_q4_min_batch(0)

    def __exit__(self, *a):
        solver.lib().frp_nmpc_set_q4_min_batch(self.prev)


def _compare(w, tol, opt=None, oopt=None, iterates=True):
    z, fl, it, info = solver.solve_batch_host(w, opt)
    zo, flo, io = OL.solve_batch(w) if oopt is None else OL.solve_batch(w, oopt)
    ito = np.array([i.it for i in io])
    nfb = np.array([i.nfallback for i in io])
    ok = (fl == 1) & (flo == 1) & (it == ito)
    err = float(np.max(np.abs(z[ok] - zo[ok]))) if ok.any() else 0.0
    print(f"N={w['N']} flags {fl.tolist()} / {flo.tolist()}  iterations {it.tolist()} / {ito.tolist()}  "
          f"redo {info[:, 7].astype(int).tolist()} / {nfb.tolist()}  max|z - z_oracle| = {err:.3e} (bound {tol:g})")
    assert np.array_equal(fl, flo), (fl, flo)
    assert np.array_equal(it, ito), (it, ito)
    if iterates:
        assert err < tol, err
    return fl, info, flo, nfb


# N = 4: one pass of three stages + stage 0 (the kk == 3 branch); 5: one four-stage pass; 7: a pass + the remainder loop; 20: the headline
@pytest.mark.parametrize("N", [4, 5, 7, 20])
def test_config2_steps_like_the_oracle_on_every_stage_loop_shape(N):
    w = _cut(workloads.config2(8), N)
    with _q4():
        assert solver.solver_variant(8, N, w["M"], 6, w["model"], solver.default_options()) == Q4_KERNEL
        _compare(w, 1e-6)


@pytest.mark.parametrize("N", [4, 5, 7, 20])
def test_hard_family_steps_like_the_oracle_on_every_stage_loop_shape(N):
    w = _cut(workloads.config_hard(8), N)
    with _q4():
        _compare(w, 1e-5)


def test_failed_pivot_poisons_the_sweep_and_is_discarded(golden_dir):
    """Instances of the hard fixture family whose exact-Hessian pivot block is not positive definite at some stage: the oracle
    (checked here, on the CPU) redoes that factorisation with the Gauss-Newton Hessian (nfallback > 0) or leaves with -7.  The
    device must take the same exits with the same redo count: a pivot test that swallowed a NaN or a sign would change either."""
    g = np.load(os.path.join(golden_dir, "solutions_hard.npz"), allow_pickle=False)
    sel = np.array([2, 30, 62, 134, 0, 1, 3, 4])  # the four -7 exits of the normal model + four that converge
    assert np.all(g["model"][sel] == g["model"][sel][0])
    w = dict(xinit=g["xinit"][sel], x0=g["x0"][sel], params=g["params"][sel], nfaces=g["nfaces"][sel],
             N=int(g["N"]), M=int(g["M"]), model=int(g["model"][sel][0]))
    with _q4():
        fl, info, flo, nfb = _compare(w, 1e-5, iterates=False)
    assert (nfb > 0).any() and (flo == -7).sum() >= 4, (nfb, flo)   # the chosen instances do take those paths in the oracle
    assert np.array_equal(info[:, 7].astype(int), nfb), (info[:, 7], nfb)


def test_indefinite_pivot_on_the_four_per_cu_kernel_is_a_factorisation_error():
    """The row form's pivot test on the kernel that has it in its factor sweep: a negative input-rate weight makes every pivot
    block indefinite under both Hessians (tests/test_gpu_parity.py: test_indefinite_cost_reports_factorization_error)."""
    w = workloads.config2(8)
    p = w["params"].copy()
    p[:, :, 8] = -50.0
    w["params"] = p
    with _q4():
        assert solver.solver_variant(8, w["N"], w["M"], 6, w["model"], solver.default_options()) == Q4_KERNEL
        z, fl, it, info = solver.solve_batch_host(w)
    zo, flo, io = OL.solve_batch(w)
    assert np.all(fl == L.FACTORIZATION_ERROR) and np.array_equal(fl, flo)
    assert np.all(it == 0) and np.all(np.isfinite(z))
    assert np.array_equal(info[:, 7].astype(int), np.array([i.nfallback for i in io]))


def test_twisted_solve_arrival_pivot_matches_the_oracles_twisted_solve():
    w = workloads.config2(8)
    z, fl, it, info = solver.solve_batch_host(w, solver.default_options(twist=9))
    zo, flo, io = OL.solve_batch(w, OL.default_options(twist=9))
    ito = np.array([i.it for i in io])
    print(f"twist 9: flags {fl.tolist()} / {flo.tolist()}  iterations {it.tolist()} / {ito.tolist()}")
    assert np.array_equal(fl, flo) and np.array_equal(it, ito)
