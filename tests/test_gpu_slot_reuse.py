"""A solve's bits do not depend on what its slot ran before.

The solver kernel runs persistent workgroups ("slots") that pull problem after problem from a device queue, and a lot of
state outlives a problem in a slot: the Ctl block, the X_RED partial results, the stage records, the packed-P block of the
L2 workspace, the registers the roles keep resident, and per CU the marks of the isolation protocol.  The other tests run
with at most as many problems as resident slots (every problem in a fresh workgroup), or reuse slots on benign inputs.

Part A squeezes every kernel instantiation (tests/test_gpu_variant_steps.py: CASES, the same launches, asserted by name)
onto a handful of slots with FRP_RESIDENT_SLOTS -- read at every call: it caps the grid and sizes the workspace, and does
not enter the variant selection -- so that every slot runs a chain of problems, and plants hostile predecessors: exits
-5, -7, BADFUNCEVAL, PARAM_VALUE, and (maxit = 3) MAXIT with a half-iterated record.  The squeezed runs must equal the
fresh run of the same launch bit for bit, for every problem, the poisoned ones included.  Part B runs the headline variant
with its isolation protocol at full residency, Part C pins that variant to the oracle on the hard family.
tests/test_capi_cpu.py checks that LAUNCHES names every instantiation the built library holds."""
import re

import numpy as np
import pytest

from forces_resilient_planner_amd import layout as L
from forces_resilient_planner_amd import solver, workloads

from . import test_gpu_variant_steps as VS

pytestmark = pytest.mark.gpu

KNOB = "FRP_RESIDENT_SLOTS"
LRQ = "frp::lrq::nmpc_ipm_lds_kernel<20, 2, true, 3, false>"

# The four-per-CU variant on the hard family (N = 20, long solves, exits -7, Gauss-Newton redos): Part C's launch, and in Part A the one
# whose solves reach iteration 12 (iso_it), where a solve marks its CU -- CASES[LRQ] (config3 at N = 2) stops after at most 6 iterations
HARD_ON_LRQ = ("hard", 20, 30, 0, lambda C: 128, False, 0)
# (id, instantiation, launch): every launch of the step-parity table, so every instantiation that ships, and the hard family on lrq
LAUNCHES = [(name, name, case) for name, case in VS.CASES.items()] + [("lrq on the hard family", LRQ, HARD_ON_LRQ)]

KINDS = ("indefinite", "infeasible", "nan", "count")  # the planted predecessors, see poisoned()
SENTINEL = 12345.0  # what the output buffers hold before every run: a field the kernel does not write (info of a PARAM_VALUE exit) stays equal


def small_slots(B):
    """The squeezed slot count of a case: chains of at least 8 problems per slot, and below 16 slots (iso_cap = slots / 16 = 0:
    the isolation protocol is off)."""
    return min(B // 8, 15)


ISO_SLOTS = 32  # iso_cap = 32 / 16 = 2: the four-per-CU variant's solves that reach iteration 12 mark their CU (the other builds have no such protocol)


def slot_counts(B):
    """The squeezed slot counts of a launch of B problems.  32 slots only from B = 128 on: the planted block must hold two problems
    per slot (64) and leave as many untouched ones to succeed them, which a launch of 24 .. 64 problems cannot; those launches
    belong to builds without the isolation protocol and run on small_slots(B) alone."""
    return (small_slots(B),) + ((ISO_SLOTS,) if B >= 4 * ISO_SLOTS else ())


def poisoned(case, C):
    """The launch `case` (a row of VS.CASES) on a device of C CUs with the block [0, P) overwritten by hostile predecessors, P >= twice the
    largest squeezed slot count of the launch (every slot's first claim is a poisoned problem when the block is queued first), kind i % nk:
      indefinite  input-rate weight -50: FACTORIZATION_ERROR at iteration 0 (test_indefinite_cost_reports_factorization_error);
      infeasible  faces 0 and 1 of stage N // 2 exclude each other: NOPROGRESS (test_infeasible_corridor_reports_failure_not_nan);
      nan         a NaN in x0: BADFUNCEVAL (test_launch_order_is_a_permutation_for_hostile_keys);
      count       where the launch passes face counts, one count above MF: PARAM_VALUE.
    Returns (workload as launched, MF, whether face counts are passed, kind per problem (-1 = untouched), options keywords)."""
    kind, N, M, model, bfun, tw, q4 = case
    B = bfun(C)
    w, wn, MF = VS._workload(kind, N, M, model, B)
    counts = wn.get("nfaces") is not None
    nk = 4 if counts else 3
    per = -(-2 * max(slot_counts(B)) // nk)
    P = per * nk
    assert P <= B // 2
    w = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}
    kinds = np.full(B, -1)
    kinds[:P] = np.arange(P) % nk
    s = N // 2
    w["params"][kinds == 0, :, 8] = -50.0
    bad = kinds == 1
    w["params"][bad, s, L.NPRE + 3 * M + 0] = -w["params"][bad, s, L.NPRE + 3 * M + 1] - 5.0
    w["x0"][kinds == 2, min(3, N - 1), 9] = np.nan
    if counts:
        w["nfaces"][kinds == 3, s] = MF + 1
    # an explicit m for the twisted cases (the kernel's rule for twist = -1 at B <= 1024), so that no run's m depends on its batch size
    opt = dict(twist=9 * N // 20) if tw else {}
    return w, MF, counts, kinds, opt


def _launch(w, MF, counts, opt, hint=None):
    """One launch through a DeviceSolver of its own (the workspace is sized under the knob's current value).  Returns the outputs
    and the queue workspace's first words."""
    import torch
    B = int(w["xinit"].shape[0])
    ds = solver.DeviceSolver(B, w["N"], w["M"], MF, w["model"])
    ds.use_nfaces = counts
    ds.opt = solver.default_options(**opt)
    ds.upload(w)
    ds.z.fill_(SENTINEL); ds.info.fill_(SENTINEL); ds.exitflag.fill_(-99); ds.iters.zero_()
    if hint is not None:
        ds.order_by_last_iters = True  # (the hint aliases iters: read before the solve writes it)
        ds.iters.copy_(torch.from_numpy(np.asarray(hint, dtype=np.int32)))
    ds.solve(); torch.cuda.synchronize()
    head = ds.ws[:32 + 1024].cpu().numpy().view(np.int32).copy()
    return dict(z=ds.z.cpu().numpy(), exitflag=ds.exitflag.cpu().numpy(), iters=ds.iters.cpu().numpy(),
                info=np.ascontiguousarray(ds.info.cpu().numpy()[:, 0:12])), head


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_bitwise(ref, run, tag, kinds):
    """z, exitflag, iters and info[:, 0:12] of `run` equal `ref` bit for bit; the message names the problems, their kind, and the fields."""
    for f in ("exitflag", "iters", "z", "info"):
        same = _bits(ref[f]) == _bits(run[f])
        if not same.all():
            per = same.reshape(same.shape[0], -1).all(axis=1)
            bad = np.nonzero(~per)[0]
            with np.errstate(invalid="ignore"):
                d = np.nanmax(np.abs(ref[f].astype(np.float64) - run[f].astype(np.float64)))
            names = [KINDS[k] if k >= 0 else "untouched" for k in kinds[bad[:16]]]
            cols = sorted(set(np.nonzero(~same.reshape(same.shape[0], -1))[1].tolist())) if f == "info" else None
            raise AssertionError(f"{tag}: {f} differs from the fresh run in {len(bad)} problems {bad[:16].tolist()} (kinds {names}, "
                                 f"flags {ref['exitflag'][bad[:16]].tolist()} / {run['exitflag'][bad[:16]].tolist()}, iterations {ref['iters'][bad[:16]].tolist()} / "
                                 f"{run['iters'][bad[:16]].tolist()}), max |difference| {d:.3e}" + (f", info columns {cols}" if cols else ""))


def _resident(name, C):
    """Resident workgroups of an instantiation: four per CU for lrq, else its waves-per-SIMD template argument."""
    return C * (4 if "::lrq::" in name else int(re.search(r"<\d+, \d+, \w+, (\d+), \w+>", name).group(1)))


@pytest.mark.parametrize("maxit", [None, 3], ids=["to_the_end", "maxit3"])
@pytest.mark.parametrize("name,case", [l[1:] for l in LAUNCHES], ids=[l[0] for l in LAUNCHES])
def test_slot_reuse_gives_the_bits_of_a_fresh_slot(name, case, maxit, monkeypatch):
    C = VS._cus()
    w, MF, counts, kinds, opt = poisoned(case, C)
    if maxit is not None:
        opt = dict(opt, maxit=maxit)
    B = int(w["xinit"].shape[0])
    q4 = case[6]
    variant = lambda: solver.solver_variant(B, w["N"], w["M"], MF, w["model"], solver.default_options(**opt))
    prev = solver.lib().frp_nmpc_set_q4_min_batch(q4)
    try:
        # ---- fresh: every problem in a workgroup of its own
        monkeypatch.delenv(KNOB, raising=False)
        assert B <= _resident(name, C)
        assert variant() == name
        fresh, head = _launch(w, MF, counts, opt)
        assert head[0] == 2 * B  # the queue head: B claims and the last, empty claim of each of the B workgroups
        fl, it = fresh["exitflag"], fresh["iters"]
        assert np.all(fl != -99)
        clean = kinds < 0
        assert np.all(fl[kinds == 0] == L.FACTORIZATION_ERROR) and np.all(it[kinds == 0] == 0)
        assert np.all(fl[kinds == 2] == L.BADFUNCEVAL)
        if counts:
            assert (kinds == 3).any() and np.all(fl[kinds == 3] == L.PARAM_VALUE_ERROR)
        if maxit is None:
            assert np.all(fl[kinds == 1] == L.NOPROGRESS), fl[kinds == 1]
            assert (fl[clean] == L.OPTIMAL).mean() >= 0.8, (fl[clean] == L.OPTIMAL).mean()
            if case is HARD_ON_LRQ:  # solves that mark their CU at 32 slots: planted predecessors and untouched problems alike
                assert (it[kinds == 1] >= 12).any() and (it[clean] >= 12).any(), (it[kinds == 1], it[clean].max())
        else:  # every other predecessor leaves through MAXIT, its record half iterated (oracle: 78 .. 100 % of the untouched ones too, the rest converged)
            assert np.all(fl[kinds == 1] == L.MAXIT) and np.all(it[kinds == 1] == maxit)
            assert (fl[clean] == L.MAXIT).mean() >= 0.5 and np.all(it[clean] <= maxit)
        # ---- squeezed: chains of problems per slot, the poisoned block first / last in the queue
        first = np.where(kinds >= 0, 1000, 1)  # (keys a factor 1000 apart never share a bin of the launch order)
        for S in slot_counts(B):
            monkeypatch.setenv(KNOB, str(S))
            assert variant() == name  # the knob does not enter the selection
            assert (kinds >= 0).sum() >= 2 * S and (kinds < 0).sum() >= 2 * S
            if S < 16:
                assert B // S >= 8
            for tag, hint in (("poisoned first", first), ("poisoned last", 1001 - first)):
                run, head = _launch(w, MF, counts, opt, hint)
                assert_bitwise(fresh, run, f"{S} slots, {tag}", kinds)
                assert head[0] == B + S  # the launch really ran on S workgroups: B claims and one empty claim each
                assert head[1] == 0 and np.all(head[64:] < 256)  # no CU mark outlives the launch
    finally:
        solver.lib().frp_nmpc_set_q4_min_batch(prev)


# ------------------------------------------------------------------ Part B
def test_slot_reuse_headline_variant_with_cu_isolation_at_full_residency():
    """The four-per-CU variant on three rounds of its resident slots of the hard family, no knob: long solves mark their CU and
    the other workgroups of the CU wait between two solves.  Bit for bit the plans of the same problems in index-order pieces
    of 600 (fresh slots, no queue order).  The preconditions make it a test of the protocol: enough long solves, exits -7,
    workgroups that shared a CU, and every mark given back."""
    C = VS._cus()
    B = 3 * 4 * C
    w = workloads.config_hard(B)
    prev = solver.lib().frp_nmpc_set_q4_min_batch(0)
    try:
        assert solver.solver_variant(B, w["N"], w["M"], 6, w["model"]) == LRQ
        kinds = np.full(B, -1)
        big, head = _launch(w, 6, True, {})
        pieces = []
        for lo in range(0, B, 600):
            sub = {k: (v[lo:lo + 600] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in w.items()}
            assert solver.solver_variant(int(sub["xinit"].shape[0]), w["N"], w["M"], 6, w["model"]) == LRQ
            pieces.append(_launch(sub, 6, True, {})[0])
        ref = {f: np.concatenate([p[f] for p in pieces]) for f in big}
        long_share = float((big["iters"] >= 12).mean())  # (iso_it's default)
        counter, cu = head[:8], head[64:]
        shared = int(sum(bin(int(v) & 15).count("1") > 1 for v in cu))
        print(f"solves of >= 12 iterations: {long_share:.4f}; exits -7: {int((big['exitflag'] == L.NOPROGRESS).sum())}; "
              f"CU words with more than one SIMD bit: {shared} of {int((cu != 0).sum())} in use")
        # observed on the MI355X (256 CUs, B = 3072): 10.03 % of the solves ran 12 or more iterations, 88 exits -7, and 256 of the 256 CU words
        # in use had more than one SIMD bit -- the dispatcher co-locates the workgroups at this size
        assert long_share >= 0.05, long_share
        assert (big["exitflag"] == L.NOPROGRESS).any()
        assert shared >= 1
        assert np.all(cu < 256) and counter[1] == 0
        assert_bitwise(ref, big, "three rounds against pieces of 600", kinds)
    finally:
        solver.lib().frp_nmpc_set_q4_min_batch(prev)


# ------------------------------------------------------------------ Part C
# VS.TOL's rule: ten times the maxima measured on the MI355X against the oracle, rounded up to one digit
HARD_TOL = ((7e-13, 2e-12, 2e-11, 2e-10, 5e-09), 5e-08)
    # |dz| 6.8e-14 1.7e-13 2.0e-12 1.4e-11 4.5e-10; diagnostics 4.8e-09; GN 8.6e-01 = 4e+10 x the k = 3 tolerance; agree 1.0000; redos 2


def test_slot_reuse_hard_family_steps_like_the_oracle_on_the_headline_variant():
    """The four-per-CU variant against the oracle iterate by iterate on the hard family (long solves, exits -7, Gauss-Newton
    redos): flags, iteration counts and redo counters exact, iterates and step diagnostics within HARD_TOL, the Gauss-Newton
    iterate far outside it, and at least one redo within k <= 8.  With Part A bit-equal, this comparison covers the squeezed runs too."""
    sel, out, gn, fallbacks, agree = VS.measure(LRQ, case=HARD_ON_LRQ)
    assert sel == LRQ
    print("measured:", " ".join(f"{out[k]['z']:.1e}" for k in VS.K), "; diagnostics",
          f"{max(out[k][q] for k in VS.K for q in ('mu', 'mu_aff', 'sigma', 'step_aff')):.1e}; GN {gn:.1e}; redos {fallbacks}")
    tol_z, tol_rel = HARD_TOL
    for i, k in enumerate(VS.K):
        assert agree[k] == 1.0, (k, agree[k])
        assert out[k]["z"] <= tol_z[i], (k, out[k])
        for q in ("mu", "mu_aff", "sigma", "step_aff"):
            assert out[k][q] <= tol_rel, (k, q, out[k])
    assert gn > VS.GN_FACTOR * tol_z[VS.K.index(3)], gn
    assert fallbacks > 0
