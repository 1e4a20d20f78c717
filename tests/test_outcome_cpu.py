"""CPU tests of the tick outcome (include/frp_nmpc_outcome.h): the restatement tests/outcome_oracle.py against a table of hand-worked
scenarios whose expected values are literals; the scripted fleet of tests/outcome_cases.py counted branch by branch, so that a case
list that lost one fails here instead of testing less on the GPU; and the boundary of the built library without a device.
The rule is structurally unpinned: the reference holds no test vectors for it, so the oracle is a restatement (its docstring)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from forces_resilient_planner_amd import solver

from . import outcome_cases as OC
from . import outcome_oracle as OO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K = 20, 64


@pytest.fixture(scope="module")
def runs():
    """The oracle over the scripted sequence, once per shape of end_pt / kino_path / kino_size."""
    out = {}
    for per in (True, False):
        static, initial, steps = OC.sequence(per_planner=per)
        after, met = OC.run_oracle(static, initial, steps)
        out[per] = dict(static=static, initial=initial, steps=steps, after=after, met=met)
    return out


def _count(run, pred):
    return sum(1 for t, tick in enumerate(run["met"]) for b, m in enumerate(tick) if pred(t, b, *m))


def test_cases_are_the_issues_fleet(runs):
    r = runs[True]
    assert (OC.B, OC.N, OC.K, OC.TICKS) == (256, 20, 64, 8) and len(r["steps"]) == 8
    s = r["steps"][0]
    assert s["z"].shape == (256, 20, 17) and s["mpc_output"].shape == (256, 21, 17) and s["state"].shape == (256, 9)
    again = OC.sequence()
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(again[2], r["steps"]) for k in a if k != "host")   # deterministic


def test_a_every_result_code_is_reached(runs):
    for code in (1, 0, -1, -2, -3, OO.RESULT_IDLE):
        n = _count(runs[True], lambda t, b, gate, branch, seen, result: result == code)
        assert n >= 4, (code, n)
    assert OO.RESULT_IDLE not in (1, 0, -1, -2, -3) and solver.TICK_RESULT_IDLE == OO.RESULT_IDLE
    for g in (OO.RUN, OO.IDLE, OO.AT_END, OO.ENDING):
        assert _count(runs[True], lambda t, b, gate, *_: gate == g) >= 4, g


def test_b_every_acceptance_branch_is_reached(runs):
    for br in ("success", "maxit_accepted", "replan_raised", "failure"):
        assert _count(runs[True], lambda t, b, gate, branch, seen, result: branch == br) >= 8, br
    # MAXIT with replan_count <= 3 is NOT accepted, and another exit with replan_count > 3 is not either: both in the list
    st = runs[True]["steps"]
    assert _count(runs[True], lambda t, b, gate, branch, seen, result: branch == "failure" and st[t]["exitflag"][b] == 0) >= 4
    a0 = runs[True]["after"][0]
    role3 = np.arange(OC.B) % 16 == 3
    assert np.any(role3 & (a0["accept"] == 1) & (st[0]["exitflag"] == 0)) and np.any(role3 & (a0["accept"] == 0) & (a0["replan_count"] == 4))


def test_c_both_shapes_of_the_shared_inputs_are_reached(runs):
    a, b = runs[True]["static"], runs[False]["static"]
    assert a["end_pt"].shape == (256, 3) and a["kino_path"].shape == (256, K, 3) and a["kino_size"].shape == (256,)
    assert b["end_pt"].shape == (3,) and b["kino_path"].shape == (K, 3) and b["kino_size"].shape == (1,)
    assert len(np.unique(a["kino_size"])) > 1 and len(np.unique(a["end_pt"], axis=0)) > 3
    for per in (True, False):
        assert _count(runs[per], lambda t, b, gate, *_: gate == OO.RUN) > 1000
    # the two shapes decide differently where the per-planner goal does: the shared form is no copy of the other
    assert any(not np.array_equal(x["result"], y["result"]) for x, y in zip(runs[True]["after"], runs[False]["after"]))


def test_d_reset_output_is_reached(runs):
    r = runs[True]
    n_run = n_gated = 0
    for t, s in enumerate(r["steps"]):
        a = r["after"][t]
        hit = s["reset_output"] != 0
        n_run += int(np.sum(hit & (a["gate"] == OO.RUN) & (a["keep"] == 0)))
        n_gated += int(np.sum(hit & (a["gate"] != OO.RUN) & (a["initialized"] == 0)))
        assert np.all(a["reset_output"] == 0) and np.all(a["keep"][a["gate"] != OO.RUN] == 1)
    # a healthy planner (role 12: every solve a success) cold-starts only because of it
    a3, a2 = r["after"][3], r["after"][2]
    role12 = np.arange(OC.B) % 16 == 12
    assert np.all(a3["keep"][role12] == 0) and np.all(a2["keep"][role12] == 1) and np.all(r["after"][4]["keep"][role12] == 1)
    assert n_run >= 16 and n_gated >= 1, (n_run, n_gated)


def test_e_a_replan_flag_survives_minus_three_and_fires_later(runs):
    r = runs[True]
    n = 0
    for b in range(OC.B):
        kept = None
        for t in range(OC.TICKS):
            gate, branch, seen, result = r["met"][t][b]
            if result == -3 and r["after"][t]["kino_replan"][b] == 1:
                kept = t
            elif kept is not None and gate == OO.RUN:
                if result == -2 and not seen["raised_now"]:
                    n += 1
                kept = None
    assert n >= 8, n


def test_f_precedence_minus_three_over_minus_one_over_minus_two(runs):
    far = lambda s: s["d_odom"] > 2.0
    near = lambda s: s["d_goal"] < 0.15
    all3 = _count(runs[True], lambda t, b, gate, branch, seen, result: seen is not None and far(seen) and near(seen) and seen["pending"] and result == -3)
    m1 = _count(runs[True], lambda t, b, gate, branch, seen, result: seen is not None and not far(seen) and near(seen) and seen["pending"] and result == -1)
    m3 = _count(runs[True], lambda t, b, gate, branch, seen, result: seen is not None and far(seen) and seen["pending"] and not near(seen) and result == -3)
    assert all3 >= 8 and m1 >= 8 and m3 >= 8, (all3, m1, m3)
    # and after a -1 the flag is still up
    assert _count(runs[True], lambda t, b, gate, branch, seen, result: result == -1 and seen is not None and runs[True]["after"][t]["kino_replan"][b] == 1) >= 8


def test_g_exact_thresholds_are_reached(runs):
    r = runs[True]
    two = _count(r, lambda t, b, gate, branch, seen, result: seen is not None and seen["d_odom"] == 2.0 and result != -3)
    one = _count(r, lambda t, b, gate, branch, seen, result: seen is not None and seen["d_goal"] == 1.0 and seen["max_index"] < K and r["after"][t]["mode"][b] == OO.MODEL_NORMAL)
    assert two >= 16 and one >= 16, (two, one)
    # built from representable numbers: the differences are (2, 0, 0) and (1, 0, 0) to the bit
    s = r["steps"][0]; b = 7
    assert (s["z"][b, 1, 8:11] - s["state"][b, 0:3]).tolist() == [2.0, 0.0, 0.0]
    assert (s["z"][b, N - 1, 8:11] - r["static"]["end_pt"][b]).tolist() == [-1.0, 0.0, 0.0]
    # and the other side of each threshold is in the list too
    assert _count(r, lambda t, b, gate, branch, seen, result: seen is not None and 2.0 < seen["d_odom"] < 2.6) >= 8
    assert _count(r, lambda t, b, gate, branch, seen, result: seen is not None and 0.15 <= seen["d_goal"] < 1.0 and r["after"][t]["mode"][b] == OO.MODEL_FINAL) >= 8
    # mode by the path's end and the local end
    assert _count(r, lambda t, b, gate, branch, seen, result: seen is not None and seen["max_index"] >= K and seen["d_goal"] >= 1.0) >= 8
    assert _count(r, lambda t, b, gate, branch, seen, result: seen is not None and seen["local_end"]) >= 8
    # a rejected solve decides on the plan's rows, an accepted one on z's
    assert _count(r, lambda t, b, gate, branch, seen, result: seen is not None and branch == "failure" and r["steps"][t]["z"][b, 1, 8] == 50.0 and result == 1) >= 16
    assert _count(r, lambda t, b, gate, branch, seen, result: seen is not None and branch == "success" and r["steps"][t]["mpc_output"][b, 1, 8] == 50.0 and result == 1) >= 16


# ---- (i) hand-worked scenarios: every expected value is a literal ----
def _rows(n, x1=0.0, xe=0.0, y=0.0):
    """n rows whose row 1 sits at (x1, y, 1) and whose row N - 1 at (xe, y, 1)."""
    r = [[0.0] * 17 for _ in range(n)]
    for row in r:
        row[10] = 1.0; row[9] = y
    r[1][8] = x1; r[N - 1][8] = xe
    return r


PATH = [[0.25 * k, 0.0, 1.0] for k in range(K)]
GOAL = [15.75, 0.0, 1.0]


def _tick(p, exitflag=1, z=(0.0, 0.0), plan=(0.0, 0.0), odom_x=0.0, goal=GOAL, size=K, toff=0.0, ref_replan=0, reset=0, path=PATH):
    p.tick_begin(reset)
    p.tick_end(_rows(N, *z), exitflag, _rows(N + 1, *plan), [odom_x, 0.0, 1.0] + [0.0] * 6, goal, path, size, toff, ref_replan)
    return (p.gate, p.keep, p.accept, p.result, p.replan, p.fail_count, p.replan_count, p.kino_replan, p.exit_code, p.initialized, p.cmd_status, p.pub_end,
            p.exec_mpc, p.mode)


#            name                                   planner state                         tick inputs                                (gate keep acc res rpl fail rc kr ec init status pub exec mode)
SCENARIOS = [("first tick, success",                {},                                   dict(),                                    (0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0)),
             ("second tick keeps the plan",         dict(initialized=1, exit_code=1),     dict(),                                    (0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0)),
             ("a failure cold-starts the next",     dict(initialized=1, exit_code=-7),    dict(),                                    (0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0)),
             ("plain failure",                      dict(initialized=1, exit_code=1),     dict(exitflag=-7),                         (0, 1, 0, 1, 0, 1, 0, 0, -7, 1, 0, 0, 1, 0)),
             ("third failure raises the replan",    dict(fail_count=2, replan_count=1),   dict(exitflag=-6),                         (0, 0, 0, -2, 1, 0, 2, 0, -6, 1, 0, 0, 0, 0)),
             ("MAXIT after four replans accepted",  dict(fail_count=1, replan_count=4),   dict(exitflag=0),                          (0, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0)),
             ("MAXIT after three is a failure",     dict(fail_count=1, replan_count=3),   dict(exitflag=0),                          (0, 0, 0, 1, 0, 2, 3, 0, 0, 1, 0, 0, 1, 0)),
             ("fail_count counted before :408",     dict(fail_count=2, replan_count=4),   dict(exitflag=-7),                         (0, 0, 0, -2, 1, 0, 5, 0, -7, 1, 0, 0, 0, 0)),
             ("WAIT gates: 0, exec_mpc off",        dict(cmd_status=4, fail_count=1, exit_code=-7, initialized=1), dict(exitflag=1), (2, 1, 0, 0, 0, 1, 0, 0, -7, 1, 4, 0, 0, 0)),
             ("pub_end gates: -1",                  dict(pub_end=1, cmd_status=3),        dict(exitflag=1),                          (3, 1, 0, -1, 0, 0, 0, 0, 0, 0, 3, 1, 1, 0)),
             ("idle: nothing",                      dict(exec_mpc=0, kino_replan=1),      dict(exitflag=1, ref_replan=1),            (1, 1, 0, -4, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0)),
             ("idle beats WAIT",                    dict(exec_mpc=0, cmd_status=4),       dict(),                                    (1, 1, 0, -4, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0)),
             ("reference asks for a replan",        dict(initialized=1, exit_code=1),     dict(ref_replan=1),                        (0, 1, 1, -2, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0)),
             ("odometry 2.5 away: -3 keeps flag",   dict(initialized=1, exit_code=1),     dict(odom_x=-2.5, ref_replan=1),           (0, 1, 1, -3, 0, 0, 0, 1, 1, 1, 4, 0, 0, 0)),
             ("odometry exactly 2 away: fine",      dict(initialized=1, exit_code=1),     dict(z=(2.0, 0.0)),                        (0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0)),
             ("at the goal: -1 keeps flag",         dict(initialized=1, exit_code=1, kino_replan=1), dict(z=(0.0, 15.625)),          (0, 1, 1, -1, 0, 0, 0, 1, 1, 1, 0, 1, 1, 1)),
             ("-3 over -1",                         dict(initialized=1, exit_code=1),     dict(z=(0.0, 15.625), odom_x=4.0),         (0, 1, 1, -3, 0, 0, 0, 0, 1, 1, 4, 0, 0, 1)),
             ("exactly 1.0 from the goal",          dict(initialized=1, exit_code=1),     dict(z=(0.0, 14.75)),                      (0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0)),
             ("0.5 from the goal: final mode",      dict(initialized=1, exit_code=1),     dict(z=(0.0, 15.25)),                      (0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 1)),
             ("horizon past the path: final mode",  dict(initialized=1, exit_code=1),     dict(toff=2.5),                            (0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 1)),
             ("local end: short path, far goal",    dict(initialized=1, exit_code=1),     dict(size=30),                             (0, 1, 1, -2, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0)),
             ("short path that ends at the goal",   dict(initialized=1, exit_code=1),     dict(size=30, goal=[7.25, 0.0, 1.0]),      (0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0)),
             ("rejected: the plan's rows decide",   dict(initialized=1, exit_code=1),     dict(exitflag=-7, z=(9.0, 15.75), plan=(0.0, 0.0)), (0, 1, 0, 1, 0, 1, 0, 0, -7, 1, 0, 0, 1, 0)),
             ("accepted: z's rows decide",          dict(initialized=1, exit_code=1),     dict(z=(0.0, 0.0), plan=(9.0, 15.75)),     (0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0)),
             ("reset_output cold-starts",           dict(initialized=1, exit_code=1),     dict(reset=1),                             (0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0)),
             ("reset_output on a gated planner",    dict(initialized=1, exit_code=1, pub_end=1), dict(reset=1),                      (3, 1, 0, -1, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0))]


@pytest.mark.parametrize("name,state,inputs,want", SCENARIOS, ids=[s[0] for s in SCENARIOS])
def test_i_hand_worked_scenario(name, state, inputs, want):
    got = _tick(OO.Planner(**state), **inputs)
    assert got == want, (name, got, want)


def test_i_table_is_long_enough_and_cmd_end_pt_is_the_goal():
    assert len(SCENARIOS) >= 12
    p = OO.Planner(initialized=1, exit_code=1)
    _tick(p, z=(0.0, 15.625))
    assert p.cmd_end_pt == [15.75, 0.0, 1.0]
    q = OO.Planner(initialized=1, exit_code=1)
    _tick(q, z=(0.0, 0.0))
    assert q.cmd_end_pt == [0.0, 0.0, 0.0]
    assert OO.norm3([3.0, 4.0, 12.0], [0.0, 0.0, 0.0]) == 13.0


def test_max_index_is_the_truncated_quotient():
    p = OO.Planner(initialized=1, exit_code=1)
    _tick(p, toff=0.0)
    assert p.seen["max_index"] == int((20 * 0.05 + 0.0) / 0.05) == 20
    _tick(p, toff=0.074)
    assert p.seen["max_index"] == 21
    _tick(p, toff=-0.3)
    assert p.seen["max_index"] == 14 or p.seen["max_index"] == 13   # (0.7 / 0.05 in doubles: whichever the division yields, truncated)
    assert p.seen["max_index"] == int((20 * 0.05 - 0.3) / 0.05)


# ---- (j) the boundary, without a device ----
FRP_ERR_NO_DEVICE, FRP_ERR_ARG = -1001, -1003
NAMES = ["frp_nmpc_tick_begin", "frp_nmpc_tick_end"]
TICK_GOOD = dict(B=4, **{n: 0x1000 * (i + 1) for i, (n, _) in enumerate(solver.Tick._fields_[1:])})
IN_GOOD = dict(N=20, K=64, Ts=0.05, z=0x20000, exitflag=0x21000, mpc_output=0x22000, state=0x23000, end_pt=0x24000, end_per_planner=1, kino_path=0x25000,
               path_per_planner=1, kino_size=0x26000, size_per_planner=1, time_offset=0x27000, ref_replan=0x28000, mode=0x29000)


def _has_gpu():
    try:
        return solver.lib().frp_nmpc_device_count() > 0
    except Exception:
        return False


def _structs(tick_kw=None, in_kw=None):
    a = dict(TICK_GOOD); a.update(tick_kw or {})
    b = dict(IN_GOOD); b.update(in_kw or {})
    return solver.Tick(*[a[f] for f, _ in solver.Tick._fields_]), solver.TickIn(*[b[f] for f, _ in solver.TickIn._fields_])


def _begin(reset=0x30000, **kw):
    t, _ = _structs(kw)      # the addresses are never dereferenced on the host; nothing is launched
    return solver.lib().frp_nmpc_tick_begin(ctypes.byref(t), ctypes.c_void_p(reset) if reset else None, None)


def _end(tick_kw=None, **kw):
    t, i = _structs(tick_kw, kw)
    return solver.lib().frp_nmpc_tick_end(ctypes.byref(t), ctypes.byref(i), None)


def test_the_two_calls_are_declared_and_exported_and_the_structs_are_the_headers(tmp_path):
    lib = solver.lib()
    assert solver.OUTCOME_EXPORTS == NAMES
    for n in NAMES:
        assert hasattr(lib, n), n
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    assert '#include "frp_nmpc_outcome.h"' in hdr and "#define FRP_NMPC_ABI_VERSION 7" in hdr
    own = open(os.path.join(ROOT, "include", "frp_nmpc_outcome.h")).read()
    for n in NAMES:
        assert n + "(" in own
    lines = []
    for cname, py in (("frp_nmpc_tick", solver.Tick), ("frp_nmpc_tick_in", solver.TickIn)):
        lines.append(f'_Static_assert(sizeof({cname}) == {ctypes.sizeof(py)}, "size");')
        for fld, _ in py._fields_:
            lines.append(f'_Static_assert(offsetof({cname}, {fld}) == {getattr(py, fld).offset}, "{fld}");')
    lines.append('_Static_assert(FRP_TICK_RUN == 0 && FRP_TICK_IDLE == 1 && FRP_TICK_AT_END == 2 && FRP_TICK_ENDING == 3 && FRP_TICK_RESULT_IDLE == -4, "gates");')
    assert (solver.TICK_RUN, solver.TICK_IDLE, solver.TICK_AT_END, solver.TICK_ENDING) == (OO.RUN, OO.IDLE, OO.AT_END, OO.ENDING) == (0, 1, 2, 3)
    assert (OO.INIT_POSITION, OO.ROTATE_YAW, OO.PUB_END, OO.PUB_TRAJ, OO.WAIT) == (solver.CMD_INIT_POSITION, solver.CMD_ROTATE_YAW, solver.CMD_PUB_END, solver.CMD_PUB_TRAJ, solver.CMD_WAIT)
    for inc in ("frp_nmpc.h", "frp_nmpc_outcome.h"):   # through frp_nmpc.h, and on its own; strict C99 plus the C11 assertion
        src = tmp_path / ("layout_" + inc.replace(".", "_") + ".c")
        src.write_text('#include <stddef.h>\n#include "' + inc + '"\n' + "\n".join(lines) + "\nint main(void) { return 0; }\n")
        subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(src) + ".o"])


REQUIRED_TICK = [n for n, _ in solver.Tick._fields_[1:] if n != "exec_mpc"]
REQUIRED_IN = ["z", "exitflag", "mpc_output", "state", "end_pt", "kino_path", "kino_size", "time_offset", "ref_replan"]
BAD_TICK = [dict(B=0), dict(B=-3)] + [{n: None} for n in REQUIRED_TICK]
BAD_IN = ([dict(N=1), dict(N=0), dict(N=65), dict(N=-2), dict(K=0), dict(K=-1), dict(Ts=0.0), dict(Ts=-0.05), dict(Ts=float("nan")), dict(Ts=float("inf")),
           dict(Ts=float("-inf"))] + [{n: None} for n in REQUIRED_IN])
_ids = lambda bad: ["-".join(f"{k}={v}" for k, v in kw.items()) for kw in bad]


@pytest.mark.parametrize("kw", BAD_TICK, ids=_ids(BAD_TICK))
def test_tick_struct_errors_come_before_any_device_call_in_both_entries(kw):
    assert _begin(**kw) == FRP_ERR_ARG
    assert _end(tick_kw=kw) == FRP_ERR_ARG


@pytest.mark.parametrize("kw", BAD_IN, ids=_ids(BAD_IN))
def test_tick_end_input_errors_come_before_any_device_call(kw):
    assert _end(**kw) == FRP_ERR_ARG


def test_null_structs():
    lib = solver.lib()
    t, i = _structs()
    assert lib.frp_nmpc_tick_begin(None, None, None) == FRP_ERR_ARG
    assert lib.frp_nmpc_tick_end(None, ctypes.byref(i), None) == FRP_ERR_ARG
    assert lib.frp_nmpc_tick_end(ctypes.byref(t), None, None) == FRP_ERR_ARG


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_valid_arguments_without_a_device_fail_loudly():
    """Accepted arguments reach the device check and nothing else: no CPU path.  exec_mpc, reset_output and mode are optional."""
    assert _begin() == FRP_ERR_NO_DEVICE and _begin(reset=0) == FRP_ERR_NO_DEVICE and _begin(exec_mpc=None) == FRP_ERR_NO_DEVICE and _begin(B=1) == FRP_ERR_NO_DEVICE
    assert _end() == FRP_ERR_NO_DEVICE and _end(mode=None) == FRP_ERR_NO_DEVICE and _end(tick_kw=dict(exec_mpc=None)) == FRP_ERR_NO_DEVICE
    assert _end(N=2, K=1) == FRP_ERR_NO_DEVICE and _end(N=64) == FRP_ERR_NO_DEVICE
    assert _end(end_per_planner=0, path_per_planner=0, size_per_planner=0) == FRP_ERR_NO_DEVICE
