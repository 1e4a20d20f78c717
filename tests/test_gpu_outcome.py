"""GPU tests of the tick outcome (include/frp_nmpc_outcome.h, csrc/frp_outcome.hip) against tests/outcome_oracle.py: the scripted
sequence of tests/outcome_cases.py through frp_nmpc_tick_begin / frp_nmpc_tick_end (both shapes of the shared inputs, one planner, a
tail workgroup, both horizon limits), the mode against frp_nmpc_mode_batch run after the update, DeviceFleet.full_tick(tick=...)
against the same fleet ticked with the oracle's masks fed by hand, and that tick replayed from a hipGraph.
The rule is structurally unpinned (the reference holds no test vectors for it): the oracle is a restatement."""
import ctypes

import numpy as np
import pytest

from forces_resilient_planner_amd import layout as L, solver

from . import outcome_cases as OC
from . import outcome_oracle as OO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WEIGHTS = (15.0, 3.0, 80.0, 15.0, 0.0)
INTS = OO.STATE + OO.OUT


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _fleet(B, N=20, M=30, F=6, **kw):
    return solver.DeviceFleet(B, N, M, F, L.MODEL_NORMAL, WEIGHTS, **kw)


def _load(ts, initial):
    for k in OO.STATE:
        getattr(ts, k).copy_(_dev(initial[k], np.int32))
    ts.cmd_end_pt.copy_(_dev(initial["cmd_end_pt"], np.float64))


def _arrays(ts, mode, reset):
    out = {k: getattr(ts, k).cpu().numpy() for k in INTS}
    out["cmd_end_pt"] = ts.cmd_end_pt.cpu().numpy()
    out["mode"] = mode.cpu().numpy()
    out["reset_output"] = reset.cpu().numpy()
    return out


def run_device(B, N, K, per_planner, check_mode_batch=False):
    """The scripted sequence through the two entry points, outputs poisoned before every tick.  Returns the arrays after every tick."""
    import torch
    static, initial, steps = OC.sequence(B, N, K, per_planner=per_planner)
    ts = solver.TickState(_fleet(B, N))
    _load(ts, initial)
    mode = _dev(initial["mode"], np.int32)
    end_pt, path, size = _dev(static["end_pt"], np.float64), _dev(static["kino_path"], np.float64), _dev(static["kino_size"], np.int32)
    got = []
    for s in steps:
        for name, idx, value in s["host"]:
            getattr(ts, name)[torch.from_numpy(idx).to(DEV)] = int(value)
        for k in OO.OUT:
            getattr(ts, k).fill_(-99)
        reset = _dev(s["reset_output"], np.int32)
        z, mo, toff = _dev(s["z"], np.float64), _dev(s["mpc_output"], np.float64), _dev(s["time_offset"], np.float64)
        mode_before = mode.clone()
        ts.begin(reset)
        ts.end(z, _dev(s["exitflag"], np.int32), mo, _dev(s["state"], np.float64), end_pt, path, size, toff, _dev(s["ref_replan"], np.int32),
               Ts=OC.TS, mode=mode)
        if check_mode_batch:
            # frp_nmpc_mode_batch on the plan frp_nmpc_update_batch leaves for ts.accept, for the planners that ran
            vp = ctypes.c_void_p
            solver._check(solver.lib().frp_nmpc_update_batch(B, N, vp(z.data_ptr()), vp(ts.accept.data_ptr()), vp(mo.data_ptr()), None), "update")
            m2 = mode_before.clone()
            solver._check(solver.lib().frp_nmpc_mode_batch(B, N, vp(mo.data_ptr()), vp(toff.data_ptr()), vp(size.data_ptr()), int(per_planner), vp(end_pt.data_ptr()),
                                                           int(per_planner), OC.TS, 1.0, vp(m2.data_ptr()), None), "mode")
            want = torch.where(ts.gate == solver.TICK_RUN, m2, mode_before)
            assert torch.equal(mode, want)
        torch.cuda.synchronize()
        got.append(_arrays(ts, mode, reset))
    return got, OC.run_oracle(static, initial, steps)[0]


def compare(got, want):
    for t, (g, w) in enumerate(zip(got, want)):
        for k in INTS + ("mode", "reset_output"):
            assert np.array_equal(g[k], w[k]), (t, k, np.nonzero(g[k] != w[k])[0][:8], g[k][g[k] != w[k]][:8], w[k][g[k] != w[k]][:8])
        assert np.array_equal(g["cmd_end_pt"].view(np.uint64), w["cmd_end_pt"].view(np.uint64)), (t, "cmd_end_pt")


@pytest.mark.parametrize("per_planner", [True, False], ids=["per_planner", "shared"])
def test_a_eight_tick_sequence_equals_the_oracle(per_planner):
    got, want = run_device(OC.B, OC.N, OC.K, per_planner)
    assert len(got) == 8
    compare(got, want)
    assert {int(v) for g in got for v in np.unique(g["result"])} >= ({1, 0, -1, -2, -3, -4} if per_planner else {1, 0, -2, -3, -4})


def test_b_mode_is_what_mode_batch_leaves_after_the_update():
    got, want = run_device(OC.B, OC.N, OC.K, True, check_mode_batch=True)
    compare(got, want)
    assert np.any(got[-1]["mode"] == 1) and np.any(got[-1]["mode"] == 0)
    got, want = run_device(48, OC.N, OC.K, False, check_mode_batch=True)
    compare(got, want)


@pytest.mark.parametrize("B", [1, 257])
def test_c_one_planner_and_a_tail_workgroup(B):
    compare(*run_device(B, OC.N, OC.K, True))


@pytest.mark.parametrize("N", [2, 64])
def test_d_both_horizon_limits(N):
    compare(*run_device(80, N, OC.K, True))
    compare(*run_device(80, N, 1, False))       # and a path of one sample


def _scene(B, N, K, seed):
    rng = np.random.default_rng(seed)
    s = np.arange(K) * 0.05 * 0.4
    path = np.c_[s, 0.4 * np.sin(0.8 * s), 1.0 + 0.1 * np.cos(s)]
    cloud = np.c_[rng.uniform(-3, 12, 3000), rng.uniform(-4, 4, 3000), rng.uniform(-0.5, 3, 3000)]
    cx = np.interp(cloud[:, 0], path[:, 0], path[:, 1]); cz = np.interp(cloud[:, 0], path[:, 0], path[:, 2])
    cloud = cloud[np.hypot(cloud[:, 1] - cx, cloud[:, 2] - cz) > 0.9]
    plan = np.zeros((B, N + 1, 17)); plan[..., 3] = 7.3; plan[..., 7] = 7.3
    plan[..., 8:11] = path[0] + rng.normal(0, 0.02, (B, 1, 3)); plan[..., 16] = 0.2
    return path, cloud, plan, rng.normal(0, 0.5, (B, 3))


def _bits(x):
    import torch
    return x.view(torch.int64) if x.dtype == torch.float64 else x


def test_e_full_tick_with_a_tick_state_equals_the_oracles_masks_fed_by_hand():
    import torch
    B, N, M, F, K, T = 8, 20, 30, 64, 200, 3
    path, cloud, plan, force = _scene(B, N, K, 8)
    state = plan[:, 1, 8:17].copy()
    end = path[-1].copy()
    fleets = [_fleet(B, N, M, F, weights_final=WEIGHTS) for _ in range(2)]
    for f in fleets:
        f.poly_index = torch.zeros((B, N), dtype=torch.int32, device=DEV)
        f.mpc_output.copy_(f.to_device(plan))
    d_path, d_cloud, d_f, d_state, d_end = (fleets[0].to_device(a) for a in (path, cloud, force, state, end))
    rp = [torch.zeros((B, N, 3), dtype=torch.float64, device=DEV) for _ in range(2)]
    ry = [torch.zeros((B, N), dtype=torch.float64, device=DEV) for _ in range(2)]
    toff = [torch.zeros((B,), dtype=torch.float64, device=DEV) for _ in range(2)]
    dev_fleet, host_fleet = fleets
    ts = solver.TickState(dev_fleet)
    ts.cmd_status.fill_(solver.CMD_PUB_TRAJ); ts.cmd_status[3] = solver.CMD_WAIT           # planner 3 waits: gated from the first tick on
    oracle = OO.Fleet(B)
    for p in oracle.p:
        p.cmd_status = OO.PUB_TRAJ
    oracle.p[3].cmd_status = OO.WAIT
    host_fleet.snapshot_commands(accept=torch.zeros((B,), dtype=torch.int32, device=DEV))    # first use allocates pre_plan / have_traj; nobody is accepted
    ref_replan = torch.zeros((B,), dtype=torch.int32, device=DEV)
    failed = cold = 0
    for t in range(T):
        for f in fleets:
            f.solver.opt.maxit = 1 if t == 1 else solver.default_options().maxit            # tick 1: every solve that runs ends at MAXIT
        # --- the device's tick ---
        dev_fleet.full_tick(d_f, d_path, toff[0], d_cloud, rp[0], ry[0], state=d_state, tick=ts, end_pt=d_end)
        # --- the same fleet without `tick`: the oracle on the host between the stages, its masks fed by hand ---
        oracle.tick_begin()
        keep = np.array([p.keep for p in oracle.p])
        host_fleet.coldstart(d_state, True, keep=_dev(keep, np.int32))
        host_fleet.references(d_path, toff[1], rp[1], ry[1], ref_replan)
        host_fleet.tube(); host_fleet.corridor(d_cloud, rp[1], ry[1]); host_fleet.pack(d_f, rp[1], ry[1]); host_fleet.solver.solve()
        torch.cuda.synchronize()
        hs = host_fleet.solver
        want = oracle.tick_end(hs.z.cpu().numpy(), hs.exitflag.cpu().numpy(), host_fleet.mpc_output.cpu().numpy(), state, end, path, [K],
                               toff[1].cpu().numpy(), ref_replan.cpu().numpy())
        accept = _dev(want["accept"], np.int32)
        host_fleet.update(accept=accept); host_fleet.snapshot_commands(accept=accept); host_fleet.mode.copy_(_dev(want["mode"], np.int32))
        torch.cuda.synchronize()
        # --- everything, to the bit ---
        for name in ("mpc_output", "pre_plan", "have_traj", "mode"):
            assert torch.equal(_bits(getattr(dev_fleet, name)), _bits(getattr(host_fleet, name))), (t, name)
        for k in INTS:
            assert np.array_equal(getattr(ts, k).cpu().numpy(), want[k]), (t, k, getattr(ts, k).cpu().numpy(), want[k])
        assert np.array_equal(ts.cmd_end_pt.cpu().numpy().view(np.uint64), want["cmd_end_pt"].view(np.uint64))
        assert torch.equal(ts.ref_replan, ref_replan)
        run = want["gate"] == OO.RUN
        failed += int(np.sum(run & (want["accept"] == 0))); cold += int(np.sum(run & (keep == 0))) if t > 0 else 0
        if t == 0:
            assert np.sum(run) == B - 1 and np.all(keep[run] == 0) and want["gate"][3] == OO.AT_END and want["result"][3] == 0
        for x in toff:
            x.add_(0.05)
    assert failed >= 1 and cold >= 1, (failed, cold)                                      # a forced failure, and the cold start it causes
    # the gated planner: its plan is the one it started with, it never got a trajectory, its state never moved
    assert np.array_equal(dev_fleet.mpc_output[3].cpu().numpy(), plan[3]) and int(dev_fleet.have_traj[3]) == 0 and bool((dev_fleet.pre_plan[3] == 0).all())
    assert want["gate"][3] == OO.IDLE and want["exec_mpc"][3] == 0 and want["exit_code"][3] == 0 and want["initialized"][3] == 0
    assert int(dev_fleet.have_traj.sum()) >= 1


def test_f_tick_replayed_from_a_hipgraph_equals_eager_launches():
    """full_tick(tick=...) captured once on one stream (a linear chain) and replayed; state reset and outputs poisoned before every run."""
    import torch
    B, N, M, F, K, T = 16, 20, 30, 64, 200, 3
    path, cloud, plan, force = _scene(B, N, K, 9)
    state = plan[:, 1, 8:17].copy(); state[5, 0] += 4.0                                   # planner 5: odometry far from the plan -> -3
    fleet = _fleet(B, N, M, F, weights_final=WEIGHTS)
    fleet.poly_index = torch.zeros((B, N), dtype=torch.int32, device=DEV)
    d_plan, d_path, d_cloud, d_f, d_state, d_end = (fleet.to_device(a) for a in (plan, path, cloud, force, state, path[-1].copy()))
    rp = torch.zeros((B, N, 3), dtype=torch.float64, device=DEV); ry = torch.zeros((B, N), dtype=torch.float64, device=DEV)
    toff = torch.zeros((B,), dtype=torch.float64, device=DEV)
    ts = solver.TickState(fleet)                                                           # owns every buffer: the capture allocates nothing
    ts.path_size(K)
    reset = torch.zeros((B,), dtype=torch.int32, device=DEV)
    ts.reset_output = reset
    status0 = np.full(B, solver.CMD_PUB_TRAJ, dtype=np.int32); status0[3] = solver.CMD_WAIT
    pub0 = np.zeros(B, dtype=np.int32); pub0[7] = 1
    exec0 = np.ones(B, dtype=np.int32); exec0[9] = 0

    def chain(stream=None):
        fleet.full_tick(d_f, d_path, toff, d_cloud, rp, ry, stream=stream, state=d_state, tick=ts, end_pt=d_end)

    def run(fn):
        fleet.mpc_output.copy_(d_plan); toff.zero_(); fleet.mode.zero_()
        fleet.solver.z.fill_(float("nan")); fleet.solver.exitflag.fill_(-99); fleet.solver.iters.zero_()
        fleet.pre_plan.fill_(float("nan")); fleet.have_traj.zero_()
        for k in ("fail_count", "replan_count", "kino_replan"):
            getattr(ts, k).zero_()
        ts.initialized.fill_(1); ts.exit_code.fill_(1)                                     # a fleet in flight: the plans are kept at tick 0
        ts.cmd_status.copy_(_dev(status0, np.int32)); ts.pub_end.copy_(_dev(pub0, np.int32)); ts.exec_mpc.copy_(_dev(exec0, np.int32)); ts.cmd_end_pt.zero_()
        res = []
        for t in range(T):
            for k in OO.OUT + ("ref_replan",):
                getattr(ts, k).fill_(-99)
            reset.fill_(1 if t == 2 else 0)
            fn(); toff.add_(0.05)
            res.append([x.clone() for x in [getattr(ts, k) for k in INTS + ("ref_replan", "cmd_end_pt")] + [reset, fleet.mpc_output, fleet.pre_plan, fleet.have_traj, fleet.mode]])
        torch.cuda.synchronize()
        return res

    ref = run(chain)
    result = ref[0][INTS.index("result")].cpu().numpy()
    assert result[3] == 0 and result[7] == -1 and result[9] == solver.TICK_RESULT_IDLE and result[5] == -3 and np.sum(result == 1) == B - 4
    assert ref[2][INTS.index("keep")].cpu().numpy()[0] == 0 and bool((ref[2][len(INTS) + 2] == 0).all())   # reset_output consumed: a cold start at tick 2
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        chain(side)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        chain(torch.cuda.current_stream())
    for _ in range(2):  # the first replay after capture included
        got = run(g.replay)
        for a, b in zip(got, ref):
            for x, y in zip(a, b):
                assert torch.equal(_bits(x), _bits(y))
