"""GPU tests of frp_nmpc_reference_batch (reference_kernel = getCurTraj + calculate_yaw) and frp_nmpc_mode_batch (mode_kernel =
switch_to_final), csrc/frp_reference.hip, over the case table of tests/reference_cases.py:

  ref_pos    bit-equal to oracle/reference_oracle.py and to the fixture's own sample and weight, a + w (b - a) in IEEE doubles (derived,
             not measured: the kernel compiles these lines with contraction off and every operation in them is exact or correctly rounded)
  decisions  the sample read, the look-ahead sample read (decoded from ref_yaw on paths with distinct samples), held / unwrap, the
             replan flag: those of tests/golden/reference_mp.npz (exact arithmetic on the double inputs)
  ref_yaw    against the fixture's 50 digits, within ten times the FP64 oracle's own error (tests/reference_fixture.py holds the table,
             the measured error of the kernel beside it)
  hostile    offsets nan, +-inf, <= -Ts, >= 2**31 Ts: the end of the path; the finite planners of the launch keep their bits
  mode       equal to oracle.mode_one, canaries behind mode[B - 1], and equal to what frp_nmpc_tick_end writes from the same inputs
  tick       one whole DeviceFleet.full_tick, twice, with two planners the tube marks (NaN E) and one with off = nan

Every launch has B <= 64 planners (mode: up to 600), every case runs at blockIdx > 0 once."""
import ctypes
import math
import sys

import numpy as np
import pytest

from forces_resilient_planner_amd import layout as L, solver

from . import oracle_lib as OL
from . import reference_cases as RC
from . import reference_fixture as RF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _oracle():
    sys.path.insert(0, OL.ROOT)
    from oracle import reference_oracle
    return reference_oracle


def _dev(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def run_launch(Ln, with_replan=True):
    """One launch, outputs poisoned first.  Returns ref_pos [B,N,3], ref_yaw [B,N], replan [B]."""
    import torch
    rp = torch.full((Ln.B, Ln.N, 3), float("nan"), dtype=torch.float64, device=DEV)
    ry = torch.full((Ln.B, Ln.N), float("nan"), dtype=torch.float64, device=DEV)
    fl = torch.full((Ln.B,), -99, dtype=torch.int32, device=DEV)
    ks = None if Ln.kino_size is None else _dev(Ln.kino_size, np.int32)
    solver.reference_batch_device(_dev(Ln.path), _dev(Ln.off), _dev(Ln.plans), rp, ry, fl if with_replan else None, ks, Ln.Ts)
    torch.cuda.synchronize()
    return rp.cpu().numpy(), ry.cpu().numpy(), fl.cpu().numpy()


@pytest.fixture(scope="module")
def device_results():
    """Every launch of the table, once: case index -> [(ref_pos, ref_yaw, replan, blockIdx), ...]."""
    out = {}
    for Ln in RC.launches():
        rp, ry, fl = run_launch(Ln)
        for b, c in enumerate(Ln.members):
            out.setdefault(c.index, []).append((rp[b], ry[b], int(fl[b]), b))
    return out


@pytest.fixture(scope="module")
def oracle_results():
    R = _oracle()
    return {c.index: RC.oracle_case(R, c) for c in RC.cases()}


def test_every_case_ran_and_once_behind_block_zero(device_results):
    for c in RC.cases():
        runs = device_results[c.index]
        assert any(r[3] > 0 for r in runs), c.name
        for r in runs[1:]:                                              # the same planner at two block indices: the same bits
            assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1]) and r[2] == runs[0][2], c.name


def test_ref_pos_is_bit_equal_to_the_oracle(device_results, oracle_results):
    """Every case, the hostile ones included (they are finite on output: the end of the path)."""
    for c in RC.cases():
        po, _, fo = oracle_results[c.index]
        for rp, _, fl, b in device_results[c.index]:
            assert np.array_equal(rp, po), (c.name, b, np.argwhere(rp != po)[:4])
            assert fl == int(fo), (c.name, b)


def test_decisions_are_the_fixtures(device_results):
    """The sample: ref_pos is, to the bit, a + w (b - a) from the FIXTURE's ki and w (neighbouring samples are 0.16 m apart), or the last
    sample.  The look-ahead sample: yaw_temp decoded from the kernel's own ref_yaw, (yaw_k - 0.2 yaw_{k-1}) / 0.8 less the unwrap, is
    nearest to the direction towards the fixture's sample among ki + 3 .. ki + 7 and the last one (a neighbour is > 1e-3 rad away on
    these paths, tests/test_reference_cpu.py).  Held stages and unwraps: as the fixture's branch bits say.  The replan flag: equal."""
    fx = RF.load()
    decoded = 0
    for c in RC.cases():
        rp, ry, fl, _ = device_results[c.index][0]
        ki, w, bits = fx.field(c, "ki"), fx.field(c, "w"), fx.field(c, "branch")
        size, path = c.eff_size, c.path
        assert fl == int(fx.replan(c)), c.name
        last = c.yaw0
        for i in range(c.N):
            b = int(bits[i])
            k = int(ki[i])
            if b & RF.B_INTERP:
                assert np.array_equal(rp[i], path[k] + w[i] * (path[k + 1] - path[k])), (c.name, i)
            else:
                assert np.array_equal(rp[i], path[size - 1]), (c.name, i)
            y = (ry[i] - 0.2 * last) / 0.8                               # yaw_temp after the unwrap, to a few ulp
            y -= (-2 * RC.PI if b & RF.B_MINUS else 2 * RC.PI if b & RF.B_PLUS else 0.0)
            if not b & RF.B_FAR:
                assert abs(y - last) < 1e-12 * max(1.0, abs(last)), (c.name, i, "held")
            elif c.family in ("grid", "grid_ulp", "end", "negative", "horizon", "size", "seed"):
                want = k + 5 if b & RF.B_AHEAD else size - 1
                cand = sorted({min(max(j, 0), size - 1) for j in range(k + 3, k + 8)} | {size - 1})
                ang = {j: math.atan2(path[j][1] - rp[i][1], path[j][0] - rp[i][0]) for j in cand if np.linalg.norm(path[j] - rp[i]) > 0.1}
                best = min(ang, key=lambda j: abs(ang[j] - y))
                assert np.array_equal(path[best], path[want]) and abs(ang[best] - y) < 1e-9, (c.name, i, best, want)
                decoded += 1
            last = ry[i]
    assert decoded > 5000


def test_ref_yaw_against_50_digits(device_results):
    fx = RF.load()
    worst = {k: 0.0 for k in RF.TOL}
    bad = []
    for c in RC.cases():
        hi, lo = fx.field(c, "yaw_hi"), fx.field(c, "yaw_lo")
        for _, ry, _, b in device_results[c.index]:
            e = float(RF.yaw_err(ry, hi, lo).max())
            key = RF.err_key(c)
            worst[key] = max(worst[key], e)
            if not e <= RF.TOL[key]:
                bad.append((c.name, b, e))
    print("\nref_yaw, kernel against 50 digits, max |err| / max(1, |yaw|):")
    for k in worst:
        print("  %-6s %.3g   (tolerance %.3g = 10 x oracle %.3g)" % (k, worst[k], RF.TOL[k], RF.ORACLE_ERR[k]))
    assert not bad, bad[:10]


def test_hostile_offsets_leave_the_finite_planners_alone(oracle_results):
    """One launch of finite planners; the same launch with every other planner replaced by a hostile one (nan, +-inf, <= -Ts,
    >= 2**31 Ts).  Hostile planners: the fixed oracle's answer.  Finite planners: their bits of the first launch."""
    for Ts in RC.TS_ALL:
        fin = [c for c in RC.cases() if c.family == "end" and c.Ts == Ts and c.path_id == "k30"][:24]
        hos = [c for c in RC.cases() if c.family == "hostile" and c.Ts == Ts] + [c for c in RC.cases() if c.family == "negative" and c.Ts == Ts and c.off <= -Ts]
        assert len(hos) >= 10
        hos30 = [RC.Case(c.name + "_k30", c.family, c.N, c.Ts, "k30", c.off, yaw0=c.yaw0) for c in hos]   # the same offsets on the finite planners' path
        clean = run_launch(RC.Launch(fin))
        mixed_members = [x for pair in zip(fin, hos30 + hos30) for x in pair][:48]
        mixed = run_launch(RC.Launch(mixed_members))
        R = _oracle()
        for b, c in enumerate(mixed_members):
            if c.family == "end":
                j = fin.index(c)
                assert all(np.array_equal(mixed[x][b], clean[x][j]) for x in range(3)), (Ts, c.name)
            else:
                po, yo, fo = RC.oracle_case(R, c)
                assert np.array_equal(mixed[0][b], po) and mixed[2][b] == int(fo), (Ts, c.name)
                assert np.max(np.abs(mixed[1][b] - yo) / np.maximum(1.0, np.abs(yo))) <= RF.TOL[Ts], (Ts, c.name)
                if not any(RC.in_range(q) for q in RC.stage_quotients(c)[1]):                   # hostile at every stage: the end of the path, the yaw held
                    assert np.array_equal(mixed[0][b], np.tile(c.path[-1], (c.N, 1))), (Ts, c.name)


def test_replan_pointer_may_be_null():
    Ln = next(x for x in RC.launches() if x.N == 20 and not x.shared and x.kino_size is not None)
    with_flag = run_launch(Ln)
    without = run_launch(Ln, with_replan=False)
    assert np.array_equal(with_flag[0], without[0]) and np.array_equal(with_flag[1], without[1])
    assert np.all(without[2] == -99) and set(np.unique(with_flag[2])) <= {0, 1}


def _mode_launch(g, mode_buf):
    vp = ctypes.c_void_p
    t = dict(plans=_dev(g.plans), off=_dev(g.off), sizes=_dev(g.sizes, np.int32), end=_dev(g.end_pt))
    solver._check(solver.lib().frp_nmpc_mode_batch(g.B, g.N, vp(t["plans"].data_ptr()), vp(t["off"].data_ptr()), vp(t["sizes"].data_ptr()), int(g.size_per),
                                                   vp(t["end"].data_ptr()), int(g.end_per), g.Ts, g.radius, vp(mode_buf.data_ptr()), None), "mode")
    return t


def test_mode_equals_mode_one_and_canaries_stand():
    import torch
    R = _oracle()
    assert RC.MODE_FINAL == L.MODEL_FINAL
    seen = set()
    for g in RC.mode_groups():
        buf = torch.full((g.B + 64,), RC.CANARY, dtype=torch.int32, device=DEV)
        buf[:g.B] = _dev(g.mode_in, np.int32)
        _mode_launch(g, buf)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        want = g.expect(R)
        assert np.array_equal(got[:g.B], want), (g.N, g.Ts, g.radius, g.B, g.size_per, g.end_per, np.nonzero(got[:g.B] != want)[0][:8])
        assert np.all(got[g.B:] == RC.CANARY), (g.B, "canary")
        assert np.all(got[:g.B][g.mode_in == RC.MODE_FINAL] == RC.MODE_FINAL)
        seen |= {(g.B, g.size_per, g.end_per)}
        assert 0 < want.sum() < g.B or g.B == 1
    assert {s[0] for s in seen} >= set(RC.MODE_B) and {s[1:] for s in seen} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_mode_batch_and_tick_end_write_the_same_mode():
    """csrc/frp_outcome.hip repeats mode_kernel's line (radius 1.0): the same inputs, hostile offsets included, give the same mode.  The
    solves are made to fail once (exitflag 0, counters 0): the tick keeps the plan, so both read the same rows."""
    import torch
    for g in [x for x in RC.mode_groups() if x.radius == 1.0 and x.B in (64, 257)]:
        fleet = solver.DeviceFleet(g.B, g.N, 30, 6, L.MODEL_NORMAL, (15.0, 3.0, 80.0, 15.0, 0.0))
        ts = solver.TickState(fleet)
        mode_a, mode_b = _dev(g.mode_in, np.int32), _dev(g.mode_in, np.int32)
        t = _mode_launch(g, mode_a)
        K = 4
        path = torch.zeros((K, 3), dtype=torch.float64, device=DEV)
        ts.begin()
        ts.end(torch.zeros((g.B, g.N, 17), dtype=torch.float64, device=DEV), torch.zeros((g.B,), dtype=torch.int32, device=DEV), t["plans"],
               torch.zeros((g.B, 9), dtype=torch.float64, device=DEV), t["end"], path, t["sizes"], t["off"], Ts=g.Ts, mode=mode_b)
        torch.cuda.synchronize()
        assert bool((ts.gate == solver.TICK_RUN).all()) and bool((ts.accept == 0).all())
        assert torch.equal(mode_a, mode_b), (g.N, g.Ts, g.B)
        assert not np.isfinite(g.off).all()                             # the group does hold non-finite offsets


def test_whole_tick_through_the_failed_planner_path():
    """DESIGN f-2's chain in one DeviceFleet.full_tick, two ticks, B = 6, N = 20, a 5000-point cloud: NaN tube -> NaN rows ->
    FRP_EXIT_BADFUNCEVAL -> plan kept.  Planners 1 and 4 carry a plan whose stage-2 thrust (1e5 times the hover thrust) puts that stage
    beyond nu = 80, so the tube marks them (E all NaN); planner 3 carries off = nan (the end of the path at every stage).  The
    corridor reads E in one place only, the comparison 'does the stage's inflated tube still fit the last polytope' (`... > 0`, false
    for NaN): no loop bound of frp_corridor*.hip depends on E, a marked planner gets the one decomposition of its stage 0.
    Marked planners leave tick 0 with BADFUNCEVAL and their plan bit for bit, and are cold-started at tick 1: their tube is then the
    tube of the constant plan.  The nan-offset planner and the three ordinary ones produce the bits they produce in a fleet where the
    marked planners carry ordinary plans."""
    import torch
    B, N, M, F, K, P = 6, 20, 30, 64, 60, 5000
    marked, nan_off, others = (1, 4), 3, (0, 2, 3, 5)
    rng = np.random.default_rng(21)
    s = np.arange(K) * 0.05 * 1.6
    path = np.c_[s, 0.4 * np.sin(0.8 * s), 1.0 + 0.1 * np.cos(s)]
    cloud = np.c_[rng.uniform(-3, 9, P), rng.uniform(-4, 4, P), rng.uniform(-0.5, 3, P)]
    cx = np.interp(cloud[:, 0], path[:, 0], path[:, 1]); cz = np.interp(cloud[:, 0], path[:, 0], path[:, 2])
    cloud = cloud[np.hypot(cloud[:, 1] - cx, cloud[:, 2] - cz) > 0.9]
    f_ext = rng.uniform(-1.5, 1.5, (B, 3))
    plan = np.zeros((B, N + 1, 17)); plan[..., 3] = 7.3; plan[..., 7] = 7.3
    plan[..., 8:11] = path[0] + rng.normal(0, 0.02, (B, 1, 3)); plan[..., 16] = 0.2
    wild = plan.copy()
    for p in marked:
        wild[p, 2, 3] = 7.3e5
    weights = (15.0, 3.0, 80.0, 15.0, 0.0)

    def run(plans):
        fleet = solver.DeviceFleet(B, N, M, F, L.MODEL_NORMAL, weights)
        fleet.mpc_output.copy_(fleet.to_device(plans))
        fleet.solver.exitflag.fill_(1)                                  # a fleet in flight: tick 0 keeps the plans it is given
        d_path, d_cloud, d_f = fleet.to_device(path), fleet.to_device(cloud), fleet.to_device(f_ext)
        rp = torch.zeros((B, N, 3), dtype=torch.float64, device=DEV); ry = torch.zeros((B, N), dtype=torch.float64, device=DEV)
        out = []
        for tick in range(2):
            off = np.full(B, 0.05 * tick) + np.arange(B) * 0.013
            off[nan_off] = math.nan
            fleet.full_tick(d_f, d_path, fleet.to_device(off), d_cloud, rp, ry)
            torch.cuda.synchronize()
            out.append({k: v.cpu().numpy().copy() for k, v in dict(
                ref_pos=rp, ref_yaw=ry, E=fleet.ellipsoid, poly_A=fleet.poly_A, poly_b=fleet.poly_b, poly_nfaces=fleet.poly_nfaces,
                poly_index=fleet.poly_index, z=fleet.solver.z, exitflag=fleet.solver.exitflag, plan=fleet.mpc_output).items()})
        return out

    got, control = run(wild), run(plan)
    t0, t1 = got
    for p in marked:
        assert np.isnan(t0["E"][p]).all(), p                            # the tube marked the planner
        assert t0["exitflag"][p] == L.BADFUNCEVAL, (p, t0["exitflag"][p])
        assert np.array_equal(t0["plan"][p], wild[p]), p                # the previous plan, bit for bit
        assert np.all(t0["poly_index"][p] == 0) and np.isfinite(t0["ref_pos"][p]).all()
        cold = np.zeros((N + 1, 17)); cold[:, 3] = 7.3; cold[:, 7] = 7.3; cold[:, 8:17] = wild[p, 1, 8:17]
        assert np.array_equal(t1["E"][p], solver.tube_batch_host(cold[None, :N])[0]), p          # tick 1 started from the constant plan
        assert t1["exitflag"][p] != L.BADFUNCEVAL and np.isfinite(t1["plan"][p]).all(), (p, t1["exitflag"][p])
    assert np.array_equal(t0["ref_pos"][nan_off], np.tile(path[-1], (N, 1)))
    for t, (g, c) in enumerate(zip(got, control)):
        assert np.all(c["exitflag"][list(marked)] == 1), (t, c["exitflag"])                      # ordinary plans there: solved
        for k in g:
            for p in others:
                assert np.array_equal(g[k][p], c[k][p], equal_nan=True), (t, k, p)
        assert np.all(g["exitflag"][[0, 2, 5]] == 1), (t, g["exitflag"])
