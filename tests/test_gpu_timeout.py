"""The wall-clock budget frp_nmpc_options.timeout on the MI355X (include/frp_nmpc.h, INTEGRATION.md "timeout").

The property every test leans on: a problem that stops with FRP_EXIT_TIMEOUT (2) after k iterations returns exactly what the same
launch returns with maxit = k -- z, iters and info bit for bit, only the flag differs (0 there).  The budget changes which iteration a
solve stops at, never an iterate."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from forces_resilient_planner_amd import layout as L
from forces_resilient_planner_amd import solver, workloads

from .test_gpu_variant_steps import CASES, _cus, _workload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT, MAXIT, OPTIMAL, INVALID = 2, 0, 1, -12
TINY = 1e-7  # 0.1 us: ten ticks of the 100 MHz wall clock, far below one prologue -- every problem stops at iteration 0


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _with_q4(name, fn):
    prev = solver.lib().frp_nmpc_set_q4_min_batch(CASES[name][6])
    try:
        return fn()
    finally:
        solver.lib().frp_nmpc_set_q4_min_batch(prev)


def _check_tiny_budget(name):
    def body():
        kind, N, M, model, bfun, tw, q4 = CASES[name]
        w, wn, MF = _workload(kind, N, M, model, bfun(_cus()))
        o = lambda **k: solver.default_options(twist=-1 if tw else 0, **k)
        assert solver.solver_variant(len(w["xinit"]), w["N"], w["M"], MF, model, o(timeout=TINY)) == name
        z, fl, it, info = solver.solve_batch_host(wn, o(timeout=TINY), MF=MF)
        z0, fl0, it0, info0 = solver.solve_batch_host(wn, o(maxit=0), MF=MF)
        assert (it == 0).all(), name
        assert set(np.unique(fl)) <= {TIMEOUT, OPTIMAL}, (name, np.unique(fl))
        assert (fl == TIMEOUT).any(), name
        assert np.array_equal(fl == TIMEOUT, fl0 == MAXIT) and np.array_equal(fl[fl != TIMEOUT], fl0[fl != TIMEOUT]), name
        assert _same(z, z0) and _same(it, it0) and _same(info, info0), name
    _with_q4(name, body)


def _check_generous_budget(name):
    def body():
        kind, N, M, model, bfun, tw, q4 = CASES[name]
        w, wn, MF = _workload(kind, N, M, model, bfun(_cus()))
        o = lambda **k: solver.default_options(twist=-1 if tw else 0, **k)
        a = solver.solve_batch_host(wn, o(timeout=10.0), MF=MF)
        b = solver.solve_batch_host(wn, o(), MF=MF)
        c = solver.solve_batch_host(wn, o(timeout=float("inf")), MF=MF)
        for x, y, q in zip(a, b, c):
            assert _same(x, y) and _same(q, y), name
        assert TIMEOUT not in set(a[1].tolist())
    _with_q4(name, body)


@pytest.mark.parametrize("name", list(CASES))
def test_a_budget_below_one_prologue_stops_every_problem_at_iteration_zero(name):
    """Every instantiation: flag 2 (or 1 for a problem optimal at its start), iters 0, and z / info / iters of a maxit = 0 launch."""
    _check_tiny_budget(name)


@pytest.mark.parametrize("name", list(CASES))
def test_a_generous_budget_changes_nothing(name):
    """Every instantiation: timeout = 10 s and +inf give the outputs of timeout = 0 bit for bit."""
    _check_generous_budget(name)


def _device_solver(w, MF):
    B, N, M = len(w["xinit"]), int(w["N"]), int(w["M"])
    ds = solver.DeviceSolver(B, N, M, MF, int(w["model"]), "cuda:0")
    ds.upload(w)
    return ds


def _outputs(ds):
    import torch
    torch.cuda.synchronize()
    return ds.z.cpu().numpy().copy(), ds.exitflag.cpu().numpy().copy(), ds.iters.cpu().numpy().copy(), ds.info.cpu().numpy().copy()


def _event_ms(ds, reps=1):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ds.solve()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _mixed_regime(w, MF, variant_tail):
    import torch
    ds = _device_solver(w, MF)
    B, N, M = len(w["xinit"]), int(w["N"]), int(w["M"])
    assert solver.solver_variant(B, N, M, MF, int(w["model"]), ds.opt).endswith(variant_tail)
    ds.solve(); torch.cuda.synchronize()  # (warm-up)
    t_full = float(np.median([_event_ms(ds) for _ in range(5)]))
    budget_ms = t_full / 3
    ds.opt.timeout = budget_ms * 1e-3
    t_b = _event_ms(ds)
    z, fl, it, info = _outputs(ds)
    assert (fl == OPTIMAL).any() and (fl == TIMEOUT).any(), np.unique(fl, return_counts=True)
    assert t_b <= budget_ms + 0.5 * t_full, (t_b, budget_ms, t_full)
    ds.opt.timeout = 0.0
    for k in np.unique(it[fl == TIMEOUT]):
        ds.opt.maxit = int(k)
        ds.solve()
        zk, flk, itk, infok = _outputs(ds)
        s = (fl == TIMEOUT) & (it == k)
        assert (flk[s] == MAXIT).all(), k
        assert _same(z[s], zk[s]) and _same(it[s], itk[s]) and _same(info[s], infok[s]), k
    return t_full, t_b


def test_mixed_regime_on_configs2_headline_variant():
    """configs[2] (B = 4096, N = 20) on the headline variant with a budget of a third of the unbounded launch: some problems converge,
    some time out, and every timed-out problem equals a maxit = k launch; the launch ends near the budget."""
    w = workloads.config2(4096)
    _mixed_regime(w, 6, "lrq::nmpc_ipm_lds_kernel<20, 2, true, 3, false>")


def test_mixed_regime_on_the_ticks_thirty_row_variant():
    """The same on the (20, 10, false) variant: 30 corridor rows per stage, B = 4096."""
    w = workloads.config3(4096, N=20, M=30)
    _mixed_regime(w, 30, "lr::nmpc_ipm_lds_kernel<20, 10, false, 3, false>")


@pytest.mark.parametrize("bad", [-1.0, float("nan"), 1e-9])
def test_an_invalid_budget_solves_nothing(bad):
    """Negative, NaN, shorter than one tick: every problem -12 with iters 0 and z = x0 bit for bit; the call itself succeeds."""
    w = workloads.config2(64)
    ds = _device_solver(w, 6)
    ds.exitflag.fill_(77); ds.iters.fill_(77); ds.z.fill_(float("nan"))
    ds.opt.timeout = bad
    ds.solve()
    z, fl, it, info = _outputs(ds)
    assert (fl == INVALID).all() and (it == 0).all()
    assert _same(z, ds.x0.cpu().numpy())
    zh, flh, ith, _ = solver.solve_batch_host(w, solver.default_options(timeout=bad))
    assert (flh == INVALID).all() and (ith == 0).all() and _same(zh, np.ascontiguousarray(w["x0"]))


_DROPIN = r"""
import ctypes, sys
sys.path.insert(0, {root!r})
from forces_resilient_planner_amd import solver, workloads
w0 = workloads.config0()
p = solver.ForcesParams(); o = solver.ForcesOutput(); info = solver.ForcesInfo()
p.xinit[:] = w0["xinit"][0]; p.x0[:] = w0["x0"][0].ravel(); p.all_parameters[:] = w0["params"][0].ravel()
p.num_of_threads = 1
flag = solver.lib().FORCESNLPsolver_normal_solve(ctypes.byref(p), ctypes.byref(o), ctypes.byref(info), None, None)
same = all(o.x[i][j] == p.x0[17 * i + j] for i in range(20) for j in range(17))
print("RESULT", flag, info.it, int(same))
"""


@pytest.mark.parametrize("env,want", [("-1", INVALID), ("1e-7", TIMEOUT), ("10", OPTIMAL)])
def test_dropin_reads_its_budget_from_the_environment(env, want):
    """FRP_NMPC_TIMEOUT (seconds) is the drop-in call's budget: -1 returns -12 with the initial guess, a budget below one prologue
    returns 2 after 0 iterations, a generous one changes nothing."""
    r = subprocess.run([sys.executable, "-c", _DROPIN.format(root=ROOT)], env=dict(os.environ, FRP_NMPC_TIMEOUT=env),
                       capture_output=True, text=True, timeout=300)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")]
    assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-2000:]
    _, flag, it, same = line[0].split()
    assert int(flag) == want, line
    if want in (INVALID, TIMEOUT):
        assert int(it) == 0, line
    if want == INVALID:
        assert int(same) == 1, line


def test_one_budget_for_a_whole_host_call():
    """frp_nmpc_solve_batch_host cuts B = 16384 pageable problems into chunks; they share ONE origin, so with a 0.2 ms budget the
    problems of the last chunk (staged milliseconds later) all stop at iteration 0.  Timed-out problems equal a maxit = k call."""
    w = workloads.config2(16384)
    z, fl, it, info = solver.solve_batch_host(w, solver.default_options(timeout=2e-4))
    assert (it[-3000:] == 0).all(), np.unique(it[-3000:], return_counts=True)
    assert (fl == TIMEOUT).any()
    ks = [k for k in np.unique(it[fl == TIMEOUT])][:4]
    for k in ks:
        zk, flk, itk, infok = solver.solve_batch_host(w, solver.default_options(maxit=int(k)))
        s = (fl == TIMEOUT) & (it == k)
        assert (flk[s] == MAXIT).all() and _same(z[s], zk[s]) and _same(info[s], infok[s]) and _same(it[s], itk[s]), k


def test_pipelined_host_batch_has_one_budget_per_ticket():
    """_host_begin / _wait on registered memory: the same maxit = k identity for the problems a budget stops."""
    B = 3000
    w = workloads.config2(B, seed=31)
    w = {k: (np.ascontiguousarray(v, dtype=(np.int32 if k == "nfaces" else np.float64)) if isinstance(v, np.ndarray) else v) for k, v in w.items()}
    ref = solver.solve_batch_host(w)
    out = tuple(np.full_like(a, -7) for a in ref)
    reg = [w["xinit"], w["x0"], w["params"], w["nfaces"]] + list(out)
    import torch
    ds = _device_solver(w, 6)
    t_full = float(np.median([_event_ms(ds) for _ in range(3)]))
    solver.host_register(*reg)
    try:
        tk = solver.solve_batch_host_begin(w, out, solver.default_options(timeout=t_full * 1e-3 / 3))
        solver.solve_batch_host_wait(tk)
        z, fl, it, info = (a.copy() for a in out)
    finally:
        solver.host_unregister(*reg)
    assert (fl == TIMEOUT).any() and (fl == OPTIMAL).any(), np.unique(fl, return_counts=True)
    for k in [k for k in np.unique(it[fl == TIMEOUT])][:4]:
        zk, flk, itk, infok = solver.solve_batch_host(w, solver.default_options(maxit=int(k)))
        s = (fl == TIMEOUT) & (it == k)
        assert (flk[s] == MAXIT).all() and _same(z[s], zk[s]) and _same(info[s], infok[s]), k


def test_graph_replays_stamp_a_fresh_origin():
    """A captured hipGraph of DeviceSolver.solve: the origin is stamped on the device at every replay (a stale one would stop every
    problem at iteration 0 from the second replay on), and with a 10 s budget replays equal eager launches bit for bit."""
    import torch
    w = workloads.config2(4096)
    ds = _device_solver(w, 6)
    ds.solve(); torch.cuda.synchronize()
    t_full = float(np.median([_event_ms(ds) for _ in range(3)]))
    for timeout, check in ((t_full * 1e-3 / 2, "fresh"), (10.0, "equal")):
        ds.opt.timeout = timeout
        ds.solve()
        eager = _outputs(ds)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ds.solve(side)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ds.solve(torch.cuda.current_stream())
        for rep in range(3):
            ds.iters.fill_(-1); ds.exitflag.fill_(-99)
            g.replay()
            z, fl, it, info = _outputs(ds)
            if check == "fresh":
                assert (it > 0).sum() > 0, rep
                assert (fl == TIMEOUT).any() or (fl == OPTIMAL).all(), rep
            else:
                for a, b in zip((z, fl, it, info), eager):
                    assert _same(a, b), rep
            time.sleep(0.01)
        del g


def test_fleet_keeps_the_plans_of_timed_out_planners_and_cold_starts_them():
    """DeviceFleet.full_tick with a budget: a planner that timed out keeps its previous plan (update_kernel writes on 1 only) and the
    next tick's cold start restarts it -- what any flag other than 1 does."""
    import torch
    from forces_resilient_planner_amd.adapter import init_mpc_output
    B, N, M, F, K = 256, 20, 30, 64, 200
    rng = np.random.default_rng(8)
    s = np.arange(K) * 0.05 * 0.4
    path = np.c_[s, 0.4 * np.sin(0.8 * s), 1.0 + 0.1 * np.cos(s)]
    cloud = np.c_[rng.uniform(-3, 12, 3000), rng.uniform(-4, 4, 3000), rng.uniform(-0.5, 3, 3000)]
    cx = np.interp(cloud[:, 0], path[:, 0], path[:, 1]); cz = np.interp(cloud[:, 0], path[:, 0], path[:, 2])
    cloud = cloud[np.hypot(cloud[:, 1] - cx, cloud[:, 2] - cz) > 0.9]
    plan = np.zeros((B, N + 1, 17)); plan[..., 3] = 7.3; plan[..., 7] = 7.3
    plan[..., 8:11] = path[0] + rng.normal(0, 0.02, (B, 1, 3)); plan[..., 16] = 0.2
    fleet = solver.DeviceFleet(B, N, M, F, L.MODEL_NORMAL, (15.0, 3.0, 80.0, 15.0, 0.0))
    fleet.poly_index = torch.zeros((B, N), dtype=torch.int32, device="cuda:0")
    d_path, d_cloud, d_f = fleet.to_device(path), fleet.to_device(cloud), fleet.to_device(rng.normal(0, 0.5, (B, 3)))
    rp = torch.zeros((B, N, 3), dtype=torch.float64, device="cuda:0"); ry = torch.zeros((B, N), dtype=torch.float64, device="cuda:0")
    fleet.mpc_output.copy_(fleet.to_device(plan))
    fleet.full_tick(d_f, d_path, fleet.to_device(np.zeros(B)), d_cloud, rp, ry)
    torch.cuda.synchronize()
    before = fleet.mpc_output.cpu().numpy().copy()
    fleet.solver.opt.timeout = TINY
    fleet.full_tick(d_f, d_path, fleet.to_device(np.full(B, 0.05)), d_cloud, rp, ry, coldstart=False)
    torch.cuda.synchronize()
    fl = fleet.solver.exitflag.cpu().numpy()
    after = fleet.mpc_output.cpu().numpy().copy()
    t = fl == TIMEOUT
    assert t.any()
    assert _same(after[t], before[t])
    fleet.coldstart(None)  # (the first step of the next full_tick)
    torch.cuda.synchronize()
    cold = fleet.mpc_output.cpu().numpy()
    assert np.array_equal(cold[t], init_mpc_output(after[t][:, 1, 8:17], N))
    assert _same(cold[fl == OPTIMAL], after[fl == OPTIMAL])


def test_default_code_generation_build_honours_the_budget():
    """The library built with the compiler's default code generation (lib_defaultflags.so) passes the per-instantiation budget tests."""
    from forces_resilient_planner_amd import build
    assert os.path.exists(build.DEFAULT_FLAGS_LIB), "run __graft_entry__.build()"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "below_one_prologue or generous_budget"], env=dict(os.environ, FRP_LIB=build.DEFAULT_FLAGS_LIB),
                       capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
