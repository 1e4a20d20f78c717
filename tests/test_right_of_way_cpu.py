"""CPU tests of right of way (include/frp_nmpc.h section 20): the oracle (tests/right_of_way_oracle.py) on hand-worked cases with the expected
arrays written out -- the order, the ranked boxes and every branch of hold and release, each named branch counted --, the two identities
of the ranked boxes against tests/peers_avoid_oracle.py, the argument rules through the library (FRP_ERR_ARG comes before the device is
looked for), the placement, and a proof on the oracles alone: two vehicles head-on on one line in the empty world."""
import collections
import ctypes

import numpy as np

from forces_resilient_planner_amd import build, capi, solver, workloads

from . import astar_path_cases as AC
from . import peers_avoid_oracle as AO
from . import peers_oracle as PO
from . import right_of_way_oracle as RO

# the hand-worked map of tests/test_peers_avoid_cpu.py: 8 x 8 x 4 voxels of 0.5 m at the origin (inv = 2.0 exactly); everybody is everybody's peer
ORIGIN, RES, GRID, R = (0.0, 0.0, 0.0), 0.5, (8, 8, 4), 10.0
N = 4
COUNT = collections.Counter()


def _run(pos, priority, half=(0.5, 0.5, 0.5), stages=(), plans=None, have=None, Q=8, oracle=RO.boxes_ranked):
    pos = np.asarray(pos, dtype=np.float64)
    B = len(pos)
    pre = np.zeros((B, N, 17)) if plans is None else plans
    have = np.zeros(B, dtype=np.int32) if have is None else np.asarray(have, dtype=np.int32)
    return RO.boxes_ranked(pos, np.ones(B, dtype=bool), pre, have, stages, half, R, ORIGIN, RES, GRID, Q, priority, COUNT)


def _rows(out, b):
    return out[0][b, :max(int(out[1][b]), 0)].tolist()


ME, PEER = (0.25, 0.25, 0.25), (2.0, 2.0, 1.0)


def _pair_plans():
    plans = np.zeros((2, N, 17))
    plans[0, :, 8:11] = (0.75, 0.25, 0.25)      # lo = floor(0.25 * 2) = 0, hi = floor(1.25 * 2) = 2 in x; -1 -> 0 ... 1 in y and z
    plans[1, :, 8:11] = (2.5, 2.0, 1.0)         # 4 ... 6 in x, 3 ... 5 in y, 1 ... 3 in z
    return plans


def test_a_the_order_a_tie_goes_to_the_lower_id_a_higher_priority_beats_it_and_none_is_all_zero():
    assert RO.outranks(None, 0, 1) and not RO.outranks(None, 1, 0) and RO.outranks([3, 3], 0, 1) and not RO.outranks([3, 3], 1, 0)
    assert RO.outranks([0, 5], 1, 0) and not RO.outranks([0, 5], 0, 1) and RO.outranks([-1, -2], 0, 1) and not RO.outranks(None, 2, 2)
    d2 = 1.75 * 1.75 * 2 + 0.75 * 0.75
    for priority in (None, [5, 5], [1, 0]):             # vehicle 0 outranks vehicle 1
        out = _run([ME, PEER], priority, stages=(1,), plans=_pair_plans(), have=[1, 1])
        assert _rows(out, 0) == [[3, 3, 1, 5, 5, 3]]                                    # the body of 1 alone: its plan binds nobody above it
        assert _rows(out, 1) == [[0, 0, 0, 1, 1, 1], [0, 0, 0, 2, 1, 1]]                # the body of 0 and stage 1 of its plan
        assert out[4].tolist() == [0, 2] and out[5].tolist() == [R * R, d2] and out[1].tolist() == [1, 2] and out[3].tolist() == [0, 0]
    out = _run([ME, PEER], [0, 5], stages=(1,), plans=_pair_plans(), have=[1, 1])        # a higher priority beats the lower id
    assert _rows(out, 0) == [[3, 3, 1, 5, 5, 3], [4, 3, 1, 6, 5, 3]] and _rows(out, 1) == [[0, 0, 0, 1, 1, 1]]
    assert out[4].tolist() == [2, 0] and out[5].tolist() == [d2, R * R]


def test_b_the_two_identities_against_the_peer_boxes():
    rng = np.random.default_rng(5)
    B = 40
    pos = np.zeros((B, 9)); pos[:, :3] = rng.random((B, 3)) * (3.5, 3.5, 1.8) + 0.1
    plans = rng.random((B, N, 17)) * 3.0
    have = (rng.random(B) < 0.6).astype(np.int32)
    ent = np.ones(B, dtype=bool)
    args = ((0.2, 0.2, 0.3), 0.9, ORIGIN, RES, GRID, 64)
    full = AO.boxes(pos, ent, plans, have, (0, 2), *args)
    bodies = AO.boxes(pos, ent, plans, have, (), *args)
    seen = collections.Counter()
    for priority in (None, np.arange(B, dtype=np.int32), rng.integers(0, 3, B).astype(np.int32)):
        got = RO.boxes_ranked(pos, ent, plans, have, (0, 2), *args, priority, COUNT)
        D2 = PO.dist2(pos[:, :3])
        for b in range(B):
            peers = [q for q in range(B) if q != b and D2[b, q] <= 0.9 * 0.9]
            up = [RO.outranks(priority, q, b) for q in peers]
            for cond, want, tag in ((all(up), full, "all_outrank"), (not any(up), bodies, "outranks_all")):
                if peers and cond:
                    seen[tag] += 1
                    assert all(got[i][b] == want[i][b] for i in (1, 2, 3)) and np.array_equal(got[0][b], want[0][b]), (tag, b)
            assert got[4][b] <= max(abs(int(got[1][b])), 0) and (got[5][b] == 0.81) == (not any(up))
    assert seen["all_outrank"] >= 3 and seen["outranks_all"] >= 3
    assert not all(np.array_equal(a, b) for a, b in zip(full, bodies))                  # ... and the two differ: the plans matter


def test_c_no_plan_k_0_and_8_exact_fill_one_too_many_65_peers_and_nobody_above():
    pos = [ME, PEER]
    plans = np.zeros((2, N, 17))
    for k in range(N):
        plans[0, k, 8:11] = (0.75 + 0.5 * k, 0.25, 0.25)
    eight = (0, 1, 2, 3, 0, 1, 2, 3)
    out0 = _run(pos, None, stages=(), plans=plans, have=[1, 0])
    out8 = _run(pos, None, stages=eight, plans=plans, have=[1, 0], Q=9)
    assert out0[1].tolist() == [1, 1] and out8[1].tolist() == [1, 9] and out8[4].tolist() == [0, 9]
    assert _rows(out8, 1)[:5] == [[0, 0, 0, 1, 1, 1], [0, 0, 0, 2, 1, 1], [1, 0, 0, 3, 1, 1], [2, 0, 0, 4, 1, 1], [3, 0, 0, 5, 1, 1]] and _rows(out8, 1)[5:] == _rows(out8, 1)[1:5]
    nobody = _run(pos, None, stages=eight, plans=plans, have=[0, 1], Q=9)               # the peer above has no plan; the one below has one
    assert nobody[1].tolist() == [1, 1] and nobody[4].tolist() == [0, 1]
    short = _run(pos, None, stages=eight, plans=plans, have=[1, 0], Q=8)                # one row too many: nothing stored, and it is still counted
    assert short[1].tolist() == [1, -9] and not short[0][1].any() and short[4].tolist() == [0, 9]
    # 66 vehicles in a row: planner 65 has 65 peers, all above it, the nearest 64 kept; planner 0 has nobody above
    pos = [(0.05 + 0.05 * i, 2.0, 1.0) for i in range(66)]
    out = _run(pos, None, half=(0.0, 0.0, 0.0), Q=64)
    assert out[2][65] == 1 and out[1][65] + out[3][65] == 64 and out[4][65] == out[1][65] and out[5][65] == PO.dist2(np.array(pos))[65, 64]
    assert out[4][0] == 0 and out[5][0] == R * R and out[2][0] == 1
    assert out[5][33] == PO.dist2(np.array(pos))[33, 32] and 0 < out[4][33] < out[1][33]


# ---- hold and release ----
PAR = dict(r_release=1.0, n_clear=2, a_brake=2.0, hold_timeout=5)


class Row:
    """One planner under the rule, with everything the step reads and writes."""

    def __init__(self, state=4, have_target=1, status=RO.NO_PATH, up_boxes=2, up_d2=0.25, odom=(1.0, 2.0, 1.2, 3.0, 0.0, 4.0, 0, 0, 0), **par):
        i = lambda v: np.array([v], dtype=np.int32)
        self.y = RO.new_yield(1)
        self.fsm = dict(state=i(state), have_target=i(have_target), have_traj=i(1), exec_mpc=i(1), plan_fail_count=i(2), cmd_status=i(3), pub_end=i(0))
        self.end_pt, self.cmd_end = np.array([[7.0, 8.0, 1.2]]), np.zeros((1, 3))
        self.odom, self.status, self.fleet_have = np.array([odom], dtype=np.float64), i(status), i(1)
        self.up_boxes, self.up_d2 = i(up_boxes), np.array([up_d2])
        self.par = dict(PAR, **par)

    def step(self, goal=None, **edit):
        for n, v in edit.items():
            getattr(self, n)[0] = v
        g = (None, None) if goal is None else (np.array([goal], dtype=np.float64), np.array([1], dtype=np.int32))
        RO.yield_step(self.y, self.fsm, self.end_pt, self.cmd_end, self.odom, self.status, self.up_boxes, self.up_d2, g[0], g[1], self.fleet_have, count=COUNT, **self.par)
        return {n: (v[0].tolist() if v.ndim > 1 else int(v[0])) for n, v in self.y.items()}


def test_d_goals_pass_through_and_are_latched_while_holding():
    r = Row(status=0)
    got = r.step(goal=(1.0, 2.0, 3.0))
    assert got["goal"] == [1.0, 2.0, 3.0] and got["fresh"] == 1 and got["holding"] == 0
    assert r.step()["fresh"] == 0 and r.y["goal"][0].tolist() == [1.0, 2.0, 3.0]
    r = Row()
    assert r.step()["holding"] == 1 and r.y["held_goal"][0].tolist() == [7.0, 8.0, 1.2]
    got = r.step(goal=(4.0, 5.0, 6.0))
    assert got["held_goal"] == [4.0, 5.0, 6.0] and got["fresh"] == 0 and got["goal"] == [0.0, 0.0, 0.0] and got["holding"] == 1


def test_e_entry_its_stores_its_refusals_and_the_stop_point():
    r = Row()
    got = r.step()
    # |v| = 5, lead = 5 / (2 * 2) = 1.25: stop = p + v * 1.25
    assert r.cmd_end[0].tolist() == [4.75, 2.0, 6.2] and got["holding"] == 1 and got["holds"] == 1 and got["hold_age"] == 0 and got["fresh"] == 0
    assert {n: int(v[0]) for n, v in r.fsm.items()} == dict(state=RO.WAIT_TARGET, have_target=0, have_traj=0, exec_mpc=0, plan_fail_count=0, cmd_status=RO.PUB_END, pub_end=1)
    assert r.status[0] == RO.CONSUMED == 0 and r.fleet_have[0] == 0 and r.y["held_goal"][0].tolist() == [7.0, 8.0, 1.2]
    r = Row(a_brake=np.inf)
    r.step()
    assert r.cmd_end[0].tolist() == [1.0, 2.0, 1.2] and r.y["holding"][0] == 1
    r = Row(state=RO.WAIT_TARGET, have_target=0)                           # the state machine dropped the target after four failures: the hold still starts
    assert r.step()["holding"] == 1 and r.y["held_goal"][0].tolist() == [7.0, 8.0, 1.2]
    for kw in (dict(state=RO.EXEC_TRAJ), dict(up_boxes=0), dict(status=2), dict(status=0)):
        r = Row(**kw)
        before = {n: v.copy() for n, v in r.fsm.items()}
        got = r.step()
        assert got["holding"] == 0 and got["holds"] == 0 and all(np.array_equal(before[n], r.fsm[n]) for n in before) and r.status[0] == kw.get("status", RO.NO_PATH), kw
    r = Row()
    got = r.step(goal=(1.0, 1.0, 1.0))                                     # a fresh goal: it goes through, no hold this step
    assert got["holding"] == 0 and got["fresh"] == 1 and r.status[0] == RO.NO_PATH
    assert r.step()["holding"] == 1                                        # ... the next step holds
    for bad in ((np.nan, 2.0, 1.2, 3.0, 0.0, 4.0, 0, 0, 0), (1.0, 2.0, 1.2, 3.0, np.inf, 4.0, 0, 0, 0)):
        r = Row(odom=bad)
        got = r.step()
        assert got["holding"] == 0 and got["bad"] == 1 and r.status[0] == RO.NO_PATH and r.fsm["state"][0] == 4
        assert r.step()["bad"] == 2


def test_f_clear_not_clear_the_count_reset_release_timeout_and_longest_hold():
    r = Row()
    r.step()
    got = r.step()                                                          # d2 = 0.25 <= 1: not clear
    assert (got["hold_age"], got["clear_count"], got["hold_periods"], got["longest_hold"], got["holding"]) == (1, 0, 1, 1, 1)
    got = r.step(up_d2=1.0)                                                 # d2 == r2 is not beyond it
    assert got["clear_count"] == 0
    got = r.step(up_d2=np.nextafter(1.0, 2.0))
    assert (got["hold_age"], got["clear_count"], got["holding"], got["fresh"]) == (3, 1, 1, 0)
    got = r.step(up_d2=0.5)                                                 # the count starts again
    assert (got["hold_age"], got["clear_count"], got["holding"]) == (4, 0, 1)
    got = r.step(up_d2=0.5)                                                 # hold_age reaches hold_timeout = 5
    assert (got["holding"], got["fresh"], got["releases"], got["timeouts"], got["goal"], got["longest_hold"], got["hold_periods"]) == (0, 1, 1, 1, [7.0, 8.0, 1.2], 5, 5)
    assert r.step()["fresh"] == 0 and r.status[0] == 0                      # released: nothing more until a search fails again
    r.status[0] = RO.NO_PATH
    assert r.step()["holds"] == 2
    r.step(up_boxes=0)                                                      # no box of an outranking peer is clear whatever d2 says
    got = r.step(goal=(9.0, 9.0, 9.0))                                      # a goal latched in the step that releases is the goal released
    assert (got["holding"], got["fresh"], got["releases"], got["timeouts"], got["goal"], got["longest_hold"], got["hold_periods"]) == (0, 1, 2, 1, [9.0, 9.0, 9.0], 5, 7)


def test_g_reset_under_a_mask():
    y = RO.new_yield(3)
    for n in RO.INT_STATE + RO.F64_STATE:
        y[n][:] = 7
    RO.yield_reset(y, np.array([1, 0, 1], dtype=np.int32))
    assert all(y[n][1].tolist() in (7, [7.0] * 3) and not y[n][0].any() and not y[n][2].any() for n in y)
    RO.yield_reset(y)
    assert not any(v.any() for v in y.values())


def test_h_every_named_branch_was_taken():
    missing = [n for n in RO.BRANCHES_BOXES + RO.BRANCHES_STEP if COUNT[n] == 0]
    assert not missing, missing


# ---- the argument rules through the library ----
def _good():
    k = (ctypes.c_double * 64)()
    a = ctypes.addressof(k)
    p = capi.PeersArgs(4, 1, (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_int * 3)(4, 4, 4), 1.0, 1.0, 0.5, 0.25, *([a] * 14))
    v = capi.PeersBoxArgs(4, 1, 2, (ctypes.c_double * 3)(0.2, 0.2, 0.2), (ctypes.c_double * 3)(0, 0, 0), 0.5, (ctypes.c_int * 3)(8, 8, 4), *([a] * 7))
    y = capi.YieldArgs(4, 2, 5, 1.0, 2.0, *([a] * 20))
    f = capi.Fsm(4, *([a] * 21))
    return p, v, y, f, a


def test_i_the_c_abi_refuses_every_bad_argument_before_it_looks_for_a_device():
    l = solver.lib()
    nan, inf = float("nan"), float("inf")
    n = 0
    ranked = lambda p, v, a, pos=1, stride=9, ob=1, od=1: l.frp_nmpc_peers_boxes_ranked(ctypes.byref(p) if p else None, ctypes.byref(v) if v else None, a if pos else None,
                                                                                         stride, None, a if ob else None, a if od else None, None)
    for what, edit in (("N 0", dict(N=0)), ("K < 0", dict(K=-1)), ("K 9", dict(K=9)), ("Q < 0", dict(Q=-1)), ("half < 0", dict(half=(0.1, -0.1, 0.1))), ("half nan", dict(half=(nan, 0.1, 0.1))),
                       ("resolution 0", dict(resolution=0.0)), ("origin inf", dict(origin=(0.0, inf, 0.0))), ("grid 0", dict(grid=(8, 0, 4))), ("pre_plan NULL", dict(pre_plan=None)),
                       ("have_traj NULL", dict(have_traj=None)), ("stages NULL with K", dict(stages=None)), ("boxes NULL with Q", dict(boxes=None)), ("count NULL", dict(count=None)),
                       ("overflow NULL", dict(overflow=None)), ("dropped_own NULL", dict(dropped_own=None)), ("rows beyond int", dict(Q=1 << 28))):
        p, v, y, f, a = _good()
        for fld, val in edit.items():
            setattr(v, fld, type(getattr(v, fld))(*val) if isinstance(val, tuple) else val)
        assert ranked(p, v, a) == capi.FRP_ERR_ARG == l.frp_nmpc_peers_boxes(ctypes.byref(p), ctypes.byref(v), a, 9, None), what
        n += 1
    p, v, y, f, a = _good()
    for what, rc in (("p NULL", ranked(None, v, a)), ("v NULL", ranked(p, None, a)), ("pos NULL", ranked(p, v, a, pos=0)), ("stride 2", ranked(p, v, a, stride=2)),
                     ("outrank_boxes NULL", ranked(p, v, a, ob=0)), ("outrank_d2 NULL", ranked(p, v, a, od=0))):
        assert rc == capi.FRP_ERR_ARG, what
        n += 1
    p.S = 2
    assert ranked(p, v, a) == capi.FRP_ERR_ARG
    step = lambda y, f: l.frp_nmpc_yield_step(ctypes.byref(y) if y else None, ctypes.byref(f) if f else None, None)
    edits = [("B 0", dict(B=0)), ("B other than the fsm's", dict(B=3)), ("n_clear 0", dict(n_clear=0)), ("hold_timeout 0", dict(hold_timeout=0)), ("r_release < 0", dict(r_release=-1.0)),
             ("r_release nan", dict(r_release=nan)), ("r_release inf", dict(r_release=inf)), ("a_brake 0", dict(a_brake=0.0)), ("a_brake nan", dict(a_brake=nan)),
             ("goal_in without fresh_in", dict(fresh_in=None)), ("fresh_in without goal_in", dict(goal_in=None))]
    edits += [(fld + " NULL", {fld: None}) for fld, _ in capi.YieldArgs._fields_[5:] if fld not in ("goal_in", "fresh_in", "fleet_have_traj")]
    for what, edit in edits:
        p, v, y, f, a = _good()
        for fld, val in edit.items():
            setattr(y, fld, val)
        assert step(y, f) == capi.FRP_ERR_ARG, what
        n += 1
        own = what.split()[0] in ("B", "holding", "clear_count", "hold_age", "held_goal", "goal", "fresh", "holds", "releases", "timeouts", "hold_periods", "longest_hold", "bad")
        if own and what != "B other than the fsm's":
            assert l.frp_nmpc_yield_reset(ctypes.byref(y), None, None) == capi.FRP_ERR_ARG, what
            n += 1
    for fld in ("state", "have_target", "have_traj", "exec_mpc", "plan_fail_count", "cmd_status", "pub_end", "end_pt"):
        p, v, y, f, a = _good()
        setattr(f, fld, None)
        assert step(y, f) == capi.FRP_ERR_ARG, fld
        n += 1
    p, v, y, f, a = _good()
    assert step(None, f) == step(y, None) == l.frp_nmpc_yield_reset(None, None, None) == capi.FRP_ERR_ARG
    assert n > 55
    if l.frp_nmpc_device_count() == 0:
        y.goal_in = y.fresh_in = y.fleet_have_traj = None               # the optional ones absent, a_brake infinite: all fine
        y.a_brake = inf
        assert step(y, f) == capi.FRP_ERR_NO_DEVICE == l.frp_nmpc_yield_reset(ctypes.byref(y), None, None) == ranked(p, v, a)


def test_j_placement_build_and_documents():
    hdr = open(build.ROOT + "/include/frp_nmpc.h").read()
    assert hdr.index("---- (20) ") < hdr.index("---- (19) ") and "frp_nmpc_peers_boxes_ranked" in hdr
    names = ["frp_nmpc_peers_boxes_ranked", "frp_nmpc_yield_step", "frp_nmpc_yield_reset"]
    i = solver.EXPORTS.index(names[0])
    assert solver.EXPORTS[i:i + 3] == names and solver.EXPORTS[i + 3] == "frp_nmpc_peers_boxes" and all(hasattr(solver.lib(), n) for n in names)
    assert capi.C_TYPES[capi.YieldArgs] == ("frp_nmpc_yield", "frp_nmpc.h") and solver.RightOfWay.__module__.endswith("flight")
    assert "frp_peers_yield.hip" in build.SOURCES and build.PER_SOURCE_FLAGS["frp_peers_yield.hip"] == ["-ffp-contract=off"]
    ident = open(build.ROOT + "/profiles/right_of_way_identity.txt").read()
    assert "RESULT: all units identical" in ident and all(u + " [shipped flags]: IDENTICAL" in ident for u in ("frp_peers.hip", "frp_peers_boxes.hip", "frp_astar.hip", "frp_astar_peers.hip",
                                                                                                                "frp_fsm.hip", "frp_command.hip", "frp_outcome.hip", "frp_ipm_lds.hip"))
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "frp_nmpc_yield_step" in open(build.ROOT + "/" + doc).read(), doc
    import inspect
    assert inspect.signature(solver.FleetPeers.boxes).parameters["priority"].default is None


# ---- a proof on the oracles alone: two vehicles head-on on one line in the empty world, stages stamped ----
def test_k_head_on_the_order_lets_one_search_through_and_the_other_holds_and_is_released():
    w = workloads.astar_world(0, "empty", allocate_num=12000)
    grid = w["occ"].shape
    state = np.zeros((2, 9)); state[0, :3] = (-1.0, 0.05, 1.05); state[1, :3] = (1.0, 0.05, 1.05); state[0, 3], state[1, 3] = 1.0, -1.0
    pre = np.zeros((2, 20, 17))
    for k in range(20):
        pre[0, k, 8:11] = (-1.0 + 0.1 * k, 0.05, 1.05)
        pre[1, k, 8:11] = (1.0 - 0.1 * k, 0.05, 1.05)
    have, stages, ent = np.ones(2, dtype=np.int32), (2, 5, 9, 14, 19), np.ones(2, dtype=bool)
    q = dict(start_pt=state[:, :3].copy(), start_v=state[:, 3:6].copy(), start_a=np.zeros((2, 3)), end_pt=np.array([(4.0, 0.05, 1.05), (-4.0, 0.05, 1.05)]), end_v=np.zeros((2, 3)),
             f_ext=np.zeros((2, 3)))
    args = (state, ent, pre, have, stages, (0.3, 0.3, 0.3), 5.0, w["origin"], w["resolution"], grid, 16)
    sym = AO.boxes(*args)
    rk = RO.boxes_ranked(*args, None)
    assert sym[1].tolist() == [5, 5] and sym[3].tolist() == [1, 1]            # each sees the other's body and four of its five stages; the last lies over its own voxel
    assert rk[1].tolist() == [1, 5] and rk[4].tolist() == [0, 5] and rk[5].tolist() == [25.0, 4.0] and np.array_equal(rk[0][1], sym[0][1])
    # symmetric boxes: BOTH searches end NO_PATH -- each start is walled in by the other's stages on the line
    both = AO.plan_with_boxes(w, q, sym[0], sym[1])
    assert both["status"].tolist() == [AC.STATUS_NO_PATH, AC.STATUS_NO_PATH]
    # ranked boxes: the outranking vehicle finds a path round the other's body; the outranked one still fails
    one = AO.plan_with_boxes(w, q, rk[0], rk[1])
    assert one["status"][0] != AC.STATUS_NO_PATH and one["status"][1] == AC.STATUS_NO_PATH
    n0 = int(one["kino_size"][0])
    vox = [tuple(int(np.floor((x[k] - w["origin"][k]) / w["resolution"])) for k in range(3)) for x in one["kino_path"][0, :n0]]
    assert n0 > 1 and not any(all(rk[0][0, 0, k] <= v[k] <= rk[0][0, 0, 3 + k] for k in range(3)) for v in vox)
    # ... and that NO_PATH fires the enter rule for vehicle 1 alone
    i = lambda *v: np.array(v, dtype=np.int32)
    y = RO.new_yield(2)
    fsm = dict(state=i(5, 3), have_target=i(1, 1), have_traj=i(1, 1), exec_mpc=i(1, 0), plan_fail_count=i(0, 1), cmd_status=i(3, 3), pub_end=i(0, 0))
    status, cmd_end, fleet_have = one["status"].astype(np.int32), np.zeros((2, 3)), i(1, 1)
    par = dict(r_release=1.5, n_clear=3, a_brake=2.0, hold_timeout=100)
    RO.yield_step(y, fsm, q["end_pt"], cmd_end, state, status, rk[4], rk[5], None, None, fleet_have, **par)
    assert y["holding"].tolist() == [0, 1] and fsm["state"].tolist() == [5, RO.WAIT_TARGET] and fleet_have.tolist() == [1, 0] and status[1] == 0
    assert cmd_end[1].tolist() == [0.75, 0.05, 1.05]                         # 1 m/s braked at 2 m/s^2: a quarter of a metre on
    # held, vehicle 1 stamps no stage: vehicle 0's next boxes are its body alone (they were before, by rank; now by have_traj too)
    again = RO.boxes_ranked(state, ent, pre, fleet_have, stages, *args[5:], None)
    assert again[1].tolist() == [1, 5]
    # the peer passes: beyond r_release it is clear, and after n_clear steps the goal comes back
    state[0, 0] = 2.6                                                          # 1.6 m behind vehicle 1
    for k in range(3):
        far = RO.boxes_ranked(state, ent, pre, fleet_have, stages, *args[5:], None)
        assert far[5][1] == 1.6 * 1.6 or abs(far[5][1] - 2.56) < 1e-12
        RO.yield_step(y, fsm, q["end_pt"], cmd_end, state, status, far[4], far[5], None, None, fleet_have, **par)
        assert y["holding"][1] == (0 if k == 2 else 1) and y["fresh"][1] == (1 if k == 2 else 0)
    assert y["goal"][1].tolist() == [-4.0, 0.05, 1.05] and y["releases"].tolist() == [0, 1] and y["timeouts"].tolist() == [0, 0] and y["hold_periods"].tolist() == [0, 3]
