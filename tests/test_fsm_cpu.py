"""CPU tests of the fleet state machine (include/frp_nmpc_fsm.h): the restatement tests/fsm_oracle.py against a table of hand-worked
scenarios whose expected values are literals; the scripted fleet of tests/fsm_cases.py counted edge by edge and branch by branch, so that a
script that lost one fails here instead of testing less on the GPU; the header, the exports and the ctypes mirrors; and the boundary of the
built library without a device.
The layer is structurally unpinned: the reference holds no test vectors for it, so the oracle is a restatement (its docstring)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from forces_resilient_planner_amd import solver

from . import fsm_cases as FC
from . import fsm_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INIT, WAIT, YAW, GEN, REPLAN, EXEC = range(6)
NAN = float("nan")
ODOM = [0.0, 0.0, 1.0, 0.5, -0.25, 0.125, 0.0, 0.0, 0.0]           # position, velocity, euler (yaw 0)
FLAT = [[0.0] * 17 for _ in range(20)]


def _odom(yaw):
    return ODOM[:8] + [yaw]


def _plan():
    """rows whose position is (i, 2 i, 1), velocity (1, 2, 0), thrust 7.4, level attitude: the world acceleration is (0, 0, 7.4 / 0.74 - 9.81)"""
    rows = [[0.0] * 17 for _ in range(20)]
    for i, r in enumerate(rows):
        r[3] = 7.4; r[8] = float(i); r[9] = 2.0 * i; r[10] = 1.0; r[11] = 1.0; r[12] = 2.0
    return rows


# ---- (i) hand-worked scenarios: (name, initial state, callback, inputs, expected fields), every expected value a literal ----
EXEC_IN = dict(state=ODOM, pre_plan=FLAT, exit_code=1, t_cur=0.0625, now=7.5)
SCENARIOS = [
    # goalCallback
    ("goal taken, z fixed at 1.2",              {},                                        "goal",  dict(goal=[3.0, -2.0, 0.7]),          dict(trigger=1, have_target=1, end_pt=[3.0, -2.0, 1.2])),
    ("goal z = -0.1 is not below -0.1",         {},                                        "goal",  dict(goal=[3.0, -2.0, -0.1]),         dict(trigger=1, have_target=1, end_pt=[3.0, -2.0, 1.2])),
    ("goal z = -0.11 ignored",                  dict(end_pt=[9.0, 9.0, 9.0]),              "goal",  dict(goal=[3.0, -2.0, -0.11]),        dict(trigger=0, have_target=0, end_pt=[9.0, 9.0, 9.0])),
    ("goal z = NaN taken (NaN < -0.1 is false)", {},                                       "goal",  dict(goal=[3.0, -2.0, NAN]),          dict(trigger=1, have_target=1, end_pt=[3.0, -2.0, 1.2])),
    ("no message, no goal",                     {},                                        "goal",  dict(goal=[3.0, -2.0, 1.0], fresh=0), dict(trigger=0, have_target=0, end_pt=[0.0, 0.0, 0.0])),
    # extforceCallback
    ("force ignored before consider_force",     dict(state=EXEC, have_target=1),           "force", dict(force=[5.0, 0.0, 0.0]),          dict(state=EXEC, external_acc=[0.0, 0.0, 0.0], last_external_acc=[0.0, 0.0, 0.0], surpass_count=0)),
    ("quiet force: zeroed, remembered",         dict(state=EXEC, consider_force=1, have_target=1, surpass_count=2, external_acc=[1.0, 1.0, 1.0]),
                                                                                           "force", dict(force=[0.5, -0.25, 0.125]),      dict(state=EXEC, external_acc=[0.0, 0.0, 0.0], last_external_acc=[0.5, -0.25, 0.125], surpass_count=0, replan_force_surpass=0)),
    ("loud force that changed: replan",         dict(state=EXEC, consider_force=1, have_target=1),
                                                                                           "force", dict(force=[0.0, -2.0, 0.25]),        dict(state=REPLAN, external_acc=[0.0, -2.0, 0.25], last_external_acc=[0.0, -2.0, 0.25], surpass_count=1, replan_force_surpass=1, have_target=1)),
    ("loud force, no target: no transition",    dict(state=WAIT, consider_force=1),        "force", dict(force=[0.0, -2.0, 0.25]),        dict(state=WAIT, external_acc=[0.0, -2.0, 0.25], last_external_acc=[0.0, -2.0, 0.25], surpass_count=1, replan_force_surpass=1)),
    ("loud force that did not change",          dict(state=EXEC, consider_force=1, have_target=1, surpass_count=3, last_external_acc=[2.0, 0.0, 0.0]),
                                                                                           "force", dict(force=[2.25, 0.0, 0.5]),         dict(state=EXEC, external_acc=[2.25, 0.0, 0.5], last_external_acc=[2.0, 0.0, 0.0], surpass_count=0, replan_force_surpass=0)),
    ("change exactly the bound: not > bound",   dict(state=EXEC, consider_force=1, have_target=1, last_external_acc=[1.5, 0.0, 0.0]),
                                                                                           "force", dict(force=[1.0, 0.0, 0.0]),          dict(state=EXEC, surpass_count=0, last_external_acc=[1.5, 0.0, 0.0])),
    ("fierce force: REPLAN overwritten by WAIT", dict(state=EXEC, consider_force=1, have_target=1),
                                                                                           "force", dict(force=[0.0, 0.0, -10.5]),        dict(state=WAIT, have_target=0, external_acc=[0.0, 0.0, -10.5], surpass_count=1, replan_force_surpass=1)),
    ("change of exactly 10: not fierce",        dict(state=EXEC, consider_force=1, have_target=1),
                                                                                           "force", dict(force=[10.0, 0.0, 0.0]),         dict(state=REPLAN, have_target=1)),
    ("fierce force without a target",           dict(state=GEN, consider_force=1),         "force", dict(force=[11.0, 0.0, 0.0]),         dict(state=WAIT, have_target=0)),
    # mpcCallback
    ("result 1: nothing",                       dict(state=EXEC, exec_mpc=1, have_target=1), "mpc", dict(result=1),                       dict(state=EXEC, exec_mpc=1, have_target=1)),
    ("result -1: nothing",                      dict(state=EXEC, exec_mpc=1, have_target=1), "mpc", dict(result=-1),                      dict(state=EXEC, exec_mpc=1, have_target=1)),
    ("result idle: nothing",                    dict(state=YAW, have_target=1),            "mpc",   dict(result=-4),                      dict(state=YAW, exec_mpc=0, have_target=1)),
    ("result 0: the end",                       dict(state=EXEC, exec_mpc=1, have_target=1, have_traj=1), "mpc", dict(result=0),          dict(state=WAIT, exec_mpc=0, have_target=0, have_traj=1)),
    ("result -2: replan",                       dict(state=EXEC, exec_mpc=1, have_target=1), "mpc", dict(result=-2),                      dict(state=REPLAN, exec_mpc=0, have_target=1)),
    ("result -3: stop, the target stays",       dict(state=EXEC, exec_mpc=1, have_target=1), "mpc", dict(result=-3),                      dict(state=WAIT, exec_mpc=0, have_target=1)),
    # checkReplanCallback
    ("goal blocked while executing",            dict(state=EXEC, have_target=1, have_traj=1), "safety", dict(goal_blocked=1, first_hit=-1), dict(state=REPLAN, have_target=1)),
    ("goal blocked while planning",             dict(state=GEN, have_target=1),            "safety", dict(goal_blocked=1, first_hit=-1),  dict(state=WAIT, have_target=0)),
    ("goal blocked, no target: nothing",        dict(state=GEN),                           "safety", dict(goal_blocked=1, first_hit=-1),  dict(state=GEN, have_target=0)),
    ("path collides while executing",           dict(state=EXEC, have_target=1, have_traj=1), "safety", dict(goal_blocked=0, first_hit=0), dict(state=REPLAN, have_target=1)),
    ("path collision drags WAIT_TARGET along",  dict(state=WAIT, have_traj=1),             "safety", dict(goal_blocked=0, first_hit=35),  dict(state=REPLAN, have_target=0)),
    ("goal dropped AND old path collides",      dict(state=YAW, have_target=1, have_traj=1), "safety", dict(goal_blocked=1, first_hit=5), dict(state=REPLAN, have_target=0)),
    ("path hit without a trajectory: nothing",  dict(state=EXEC, have_target=1),           "safety", dict(goal_blocked=0, first_hit=5),   dict(state=EXEC)),
    # execFSMCallback
    ("INIT without odometry",                   dict(have_target=1),                       "exec",  {},                                   dict(state=INIT, search=0)),
    ("INIT with odometry, no target",           dict(have_odom=1),                         "exec",  {},                                   dict(state=INIT, search=0)),
    ("INIT with both",                          dict(have_odom=1, have_target=1),          "exec",  {},                                   dict(state=WAIT, search=0)),
    ("WAIT_TARGET without a target",            dict(state=WAIT, consider_force=1),        "exec",  {},                                   dict(state=WAIT, consider_force=0, search=0)),
    ("WAIT_TARGET with one",                    dict(state=WAIT, have_target=1, consider_force=1), "exec", {},                            dict(state=YAW, call_init_yaw=1, consider_force=1, search=0)),
    ("INIT_YAW first step, aligned",            dict(state=YAW, call_init_yaw=1, end_pt=[4.0, 0.0, 1.2]), "exec", dict(state=_odom(0.75)), dict(state=YAW, call_init_yaw=0, init_yaw=0.0, cmd_status=0, change_yaw_time=0.0, search=0)),
    ("INIT_YAW first step, exactly 0.8 off",    dict(state=YAW, call_init_yaw=1, end_pt=[1.0, 0.0, 1.2], pub_end=1), "exec", dict(state=_odom(0.8)),
                                                                                                                                          dict(state=YAW, call_init_yaw=0, init_yaw=0.0, cmd_status=1, pub_end=0, change_yaw_time=7.5, yaw_odom=_odom(0.8), search=0)),
    ("INIT_YAW behind: atan2(0, -1) = pi",      dict(state=YAW, call_init_yaw=1, end_pt=[-1.0, 0.0, 1.2]), "exec", {},                   dict(state=YAW, call_init_yaw=0, init_yaw=math.pi, cmd_status=1, change_yaw_time=7.5)),
    ("INIT_YAW turning, exactly 0.8 off",       dict(state=YAW, init_yaw=0.0),             "exec",  dict(state=_odom(-0.8)),              dict(state=YAW, consider_force=0, search=0)),
    ("INIT_YAW turned",                         dict(state=YAW, init_yaw=0.0),             "exec",  dict(state=_odom(-0.75)),             dict(state=GEN, consider_force=1, search=0)),
    ("GEN_NEW_TRAJ searches from the odometry", dict(state=GEN, exec_mpc=1, plan_fail_count=3), "exec", dict(pre_plan=_plan()),           dict(state=GEN, exec_mpc=0, search=1, start_pt=[0.0, 0.0, 1.0], start_vel=[0.5, -0.25, 0.125], start_acc=[0.0, 0.0, 0.0], retry_pt=[0.0, 0.0, 1.0], retry_vel=[0.5, -0.25, 0.125])),
    ("GEN_NEW_TRAJ gives up at the fifth",      dict(state=GEN, have_target=1, plan_fail_count=4), "exec", {},                            dict(state=WAIT, have_target=0, plan_fail_count=0, search=0)),
    ("REPLAN_TRAJ gives up too",                dict(state=REPLAN, have_target=1, plan_fail_count=4, exec_mpc=1), "exec", {},             dict(state=WAIT, have_target=0, plan_fail_count=0, exec_mpc=0, search=0)),
    ("REPLAN_TRAJ from the plan, mid-stage",    dict(state=REPLAN),                        "exec",  dict(pre_plan=_plan(), t_cur=0.0625), dict(state=REPLAN, search=1, start_pt=[1.25, 2.5, 1.0], start_vel=[1.0, 2.0, 0.0], retry_pt=[0.0, 0.0, 1.0], retry_vel=[0.5, -0.25, 0.125])),
    ("REPLAN_TRAJ on a stage boundary",         dict(state=REPLAN),                        "exec",  dict(pre_plan=_plan(), t_cur=0.1),    dict(search=1, start_pt=[2.0, 4.0, 1.0], start_vel=[1.0, 2.0, 0.0])),
    ("REPLAN_TRAJ, t_cur < 0: the odometry",    dict(state=REPLAN),                        "exec",  dict(pre_plan=_plan(), t_cur=-0.01),  dict(search=1, start_pt=[0.0, 0.0, 1.0], start_vel=[0.5, -0.25, 0.125], start_acc=[0.0, 0.0, 0.0])),
    ("REPLAN_TRAJ, t_cur / Ts = N - 1",         dict(state=REPLAN),                        "exec",  dict(pre_plan=_plan(), t_cur=19 * 0.05), dict(search=1, start_pt=[0.0, 0.0, 1.0], start_acc=[0.0, 0.0, 0.0])),
    ("REPLAN_TRAJ, t_cur NaN",                  dict(state=REPLAN),                        "exec",  dict(pre_plan=_plan(), t_cur=NAN),    dict(search=1, start_pt=[0.0, 0.0, 1.0], start_acc=[0.0, 0.0, 0.0])),
    ("REPLAN_TRAJ after a failed solve",        dict(state=REPLAN),                        "exec",  dict(pre_plan=_plan(), exit_code=0),  dict(search=1, start_pt=[0.0, 0.0, 1.0], start_acc=[0.0, 0.0, 0.0])),
    ("GEN_NEW_TRAJ never reads the plan",       dict(state=GEN),                           "exec",  dict(pre_plan=_plan(), t_cur=0.0625), dict(search=1, start_pt=[0.0, 0.0, 1.0], start_acc=[0.0, 0.0, 0.0])),
    ("EXEC_TRAJ steady",                        dict(state=EXEC, exec_mpc=1),              "exec",  {},                                   dict(state=EXEC, search=0)),
    ("EXEC_TRAJ, new goal while solving",       dict(state=EXEC, exec_mpc=1, trigger=1),   "exec",  {},                                   dict(state=REPLAN, search=0, exec_mpc=1)),
    ("EXEC_TRAJ, new goal, not solving",        dict(state=EXEC, trigger=1),               "exec",  {},                                   dict(state=EXEC, search=0)),
    # the search's verdict
    ("search succeeded",                        dict(state=GEN, trigger=1, replan_force_surpass=1, plan_fail_count=2, pub_end=1, mode=1, cmd_status=1),
                                                                                           "end",   dict(search=1, status=FO.REACH_HORIZON, now=3.25), dict(state=EXEC, have_traj=1, trigger=0, exec_mpc=1, replan_force_surpass=0, plan_fail_count=0, kino_start_time=3.25, mode=0, cmd_status=3, pub_end=0)),
    ("REACH_END_BUT_SHOT_FAILS is a success",   dict(state=REPLAN),                        "end",   dict(search=1, status=4, now=1.0),    dict(state=EXEC, exec_mpc=1, cmd_status=3)),
    ("search failed in GEN_NEW_TRAJ",           dict(state=GEN, plan_fail_count=1, trigger=1), "end", dict(search=1, status=FO.NO_PATH, now=3.25), dict(state=GEN, plan_fail_count=2, have_traj=0, trigger=1, exec_mpc=0, kino_start_time=0.0, cmd_status=0)),
    ("search failed in REPLAN_TRAJ: to GEN",    dict(state=REPLAN, plan_fail_count=3),     "end",   dict(search=1, status=FO.NO_PATH, now=3.25), dict(state=GEN, plan_fail_count=4)),
    ("no search: the status is stale",          dict(state=EXEC, plan_fail_count=1),       "end",   dict(search=0, status=FO.NO_PATH, now=3.25), dict(state=EXEC, plan_fail_count=1)),
]


def _apply(p, call, kw):
    out = {}
    if call == "goal":
        p.goal(kw["goal"], kw.get("fresh", 1))
    elif call == "force":
        p.force(kw["force"], kw.get("fresh", 1), 0.5)
    elif call == "mpc":
        p.mpc(kw["result"])
    elif call == "safety":
        p.safety(kw["goal_blocked"], kw["first_hit"])
    elif call == "exec":
        a = dict(EXEC_IN); a.update(kw)
        start = p.exec_begin(a["state"], a["pre_plan"], a["exit_code"], a["t_cur"], a["now"], 20, 0.05, 0.74, 9.81)
        out = dict(start or {}); out["search"] = int(start is not None)
    elif call == "end":
        p.exec_end(kw["search"], kw["status"], kw["now"])
    out.update(p.snapshot())
    return out


@pytest.mark.parametrize("name,initial,call,inputs,want", SCENARIOS, ids=[s[0] for s in SCENARIOS])
def test_i_hand_worked_scenario(name, initial, call, inputs, want):
    got = _apply(FO.Planner(**initial), call, inputs)
    for k, v in want.items():
        assert got[k] == v, (name, k, got[k], v)


def test_i_the_table_has_a_row_per_branch_and_the_world_acceleration_is_worked_by_hand():
    calls = [s[2] for s in SCENARIOS]
    assert {c: calls.count(c) for c in set(calls)} == dict(goal=5, force=9, mpc=6, safety=7, exec=23, end=5)
    # a level plan row with thrust 7.4 and mass 0.74: (0, 0, 10 - 9.81); rolled by 90 degrees: the thrust points along -y
    p = FO.Planner(state=REPLAN)
    got = _apply(p, "exec", dict(pre_plan=_plan(), t_cur=0.0625))
    assert got["start_acc"][0] == 0.0 and got["start_acc"][1] == 0.0 and got["start_acc"][2] == 7.4 / 0.74 - 9.81
    tw = FO.thrust_world(math.pi / 2, 0.0, 0.0, 2.0)
    assert abs(tw[0]) < 1e-15 and abs(tw[1] + 2.0) < 1e-15 and abs(tw[2]) < 1e-15
    tw = FO.thrust_world(0.0, math.pi / 2, math.pi / 2, 2.0)    # pitched forward, then yawed left: the thrust points along +y
    assert abs(tw[0]) < 1e-15 and abs(tw[1] - 2.0) < 1e-15 and abs(tw[2]) < 1e-15


def test_i_plan_fail_count_goes_to_four_and_the_fifth_attempt_gives_up():
    p = FO.Planner(state=GEN, have_target=1)
    for n in range(1, 5):
        assert p.exec_begin(ODOM, FLAT, 1, 0.0, 1.0) is not None
        p.exec_end(1, FO.NO_PATH, 1.0)
        assert (p.state, p.plan_fail_count, p.have_target) == (GEN, n, 1)
    assert p.exec_begin(ODOM, FLAT, 1, 0.0, 1.0) is None
    assert (p.state, p.plan_fail_count, p.have_target) == (WAIT, 0, 0)


# ---- (ii) the script reaches everything: a condition on tests/fsm_cases.py ----
@pytest.fixture(scope="module")
def run():
    events = FC.sequence()
    fleet, after, met = FC.run_oracle(events, FC.B)
    return dict(events=events, after=after, met=met, all=set().union(*[s for m in met for s in m]))


EDGES = [("exec", INIT, WAIT), ("exec", WAIT, YAW), ("exec", YAW, GEN), ("exec", GEN, WAIT), ("exec", REPLAN, WAIT), ("exec", EXEC, REPLAN),
         ("exec_end", GEN, EXEC), ("exec_end", REPLAN, EXEC), ("exec_end", GEN, GEN), ("exec_end", REPLAN, GEN),
         ("mpc", EXEC, WAIT), ("mpc", EXEC, REPLAN),
         ("safety_goal", EXEC, REPLAN), ("safety_goal", YAW, WAIT), ("safety_path", EXEC, REPLAN), ("safety_path", WAIT, REPLAN),
         ("force", EXEC, REPLAN), ("force", GEN, REPLAN), ("force", REPLAN, WAIT)]
BRANCHES = ["goal:taken", "goal:ignored", "force:not_considered", "force:quiet", "force:loud_changed", "force:replan", "force:fierce", "force:loud_steady",
            "init:no_odom", "init:no_target", "wait:no_target", "yaw:rotate", "yaw:aligned", "yaw:turning", "plan:give_up", "start:odom", "start:plan",
            "exec:steady", ("searched_from", GEN), ("searched_from", REPLAN)] + [("mpc", r) for r in (1, 0, -1, -2, -3, FO.RESULT_IDLE)]


def test_ii_the_script_is_the_issues_fleet(run):
    kinds = [e["kind"] for e in run["events"]]
    assert (FC.B, FC.PERIODS, FC.STEPS) == (48, 14, 2) and kinds.count("mpc") == 14 and kinds.count("exec") == 28 and kinds.count("goal") == kinds.count("force") == kinds.count("safety") == 14
    again = FC.sequence()
    for a, b in zip(again, run["events"]):
        assert a["kind"] == b["kind"] and all(np.array_equal(a[k], b[k], equal_nan=True) if isinstance(a[k], np.ndarray) and a[k].dtype.kind == "f" else np.array_equal(a[k], b[k]) for k in a if k != "kind")


@pytest.mark.parametrize("edge", EDGES, ids=[f"{w}:{a}->{b}" for w, a, b in EDGES])
def test_ii_every_edge_of_the_transition_table_is_reached(run, edge):
    assert ("edge",) + edge in run["all"], edge


def test_ii_every_branch_is_reached(run):
    missing = [b for b in BRANCHES if b not in run["all"]]
    assert not missing, missing
    # the force branch whose REPLAN_TRAJ is overwritten: both transitions in ONE callback
    both = sum(1 for m in run["met"] for s in m if "force:replan" in s and "force:fierce" in s)
    assert both >= 3, both
    # a goal with a NaN z that is taken
    assert any(e["kind"] == "goal" and np.any(np.isnan(e["goal"][:, 2]) & (e["fresh"] != 0)) for e in run["events"])
    # a search without a target (the dragged WAIT_TARGET planner)
    n = 0
    for e, a in zip(run["events"], run["after"]):
        if e["kind"] == "exec":
            n += int(np.sum((a["search"] == 1) & (a["after_begin"]["have_target"] == 0)))
    assert n >= 3, n


def test_ii_both_start_sources_and_the_edges_of_the_plan_test_are_reached(run):
    src = {"plan": 0, "odom": 0}
    seen = dict(boundary=0, negative=0, last=0, nan=0, huge=0, failed=0, gen=0)
    for e, a, m in zip(run["events"], run["after"], run["met"]):
        if e["kind"] != "exec":
            continue
        for b, s in enumerate(a["start"]):
            if s is None:
                continue
            src[s["source"]] += 1
            t = e["t_cur"][b]
            replan = ("searched_from", REPLAN) in m[b]
            ok = replan and e["exit_code"][b] == 1
            seen["boundary"] += ok and s["source"] == "plan" and math.fmod(t, FC.TS) == 0.0 and t > 0
            seen["negative"] += ok and t < 0 and s["source"] == "odom"
            seen["last"] += ok and t / FC.TS == FC.N - 1 and s["source"] == "odom"
            seen["nan"] += ok and t != t and s["source"] == "odom"
            seen["huge"] += ok and t > 1e200 and s["source"] == "odom"
            seen["failed"] += replan and e["exit_code"][b] != 1 and 0 <= t < 0.9 and s["source"] == "odom"
            seen["gen"] += (not replan) and e["exit_code"][b] == 1 and 0 <= t < 0.9 and s["source"] == "odom"
    assert src["plan"] >= 10 and src["odom"] >= 10, src
    assert all(v >= 3 for v in seen.values()), seen


# ---- (iii) header, exports, ctypes mirrors ----
NAMES = ["frp_nmpc_fsm_goal", "frp_nmpc_fsm_force", "frp_nmpc_fsm_mpc", "frp_nmpc_fsm_safety", "frp_nmpc_fsm_exec_begin", "frp_nmpc_fsm_exec_end"]


def test_iii_exports_are_the_headers_declarations_and_the_structs_are_the_headers(tmp_path):
    lib = solver.lib()
    own = open(os.path.join(ROOT, "include", "frp_nmpc_fsm.h")).read()
    declared = re.findall(r"^int (frp_nmpc_fsm_\w+)\(", own, flags=re.M)
    assert declared == NAMES == solver.FSM_EXPORTS
    for n in NAMES:
        assert hasattr(lib, n), n
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    assert hdr.count('#include "frp_nmpc_fsm.h"') == 1 and "#define FRP_NMPC_ABI_VERSION 7" in hdr and solver.ABI_VERSION == 7
    assert lib.frp_nmpc_abi_version() == 7
    for word in ("STRUCTURALLY UNPINNED", "clocks", "odometry callbacks", "displayPath", "displayGoalPoint", "four-thread spinner", "uninitialised"):
        assert word in own, word
    lines = []
    for cname, py in (("frp_nmpc_fsm", solver.Fsm), ("frp_nmpc_fsm_exec_in", solver.FsmExecIn)):
        lines.append(f'_Static_assert(sizeof({cname}) == {ctypes.sizeof(py)}, "size");')
        for fld, _ in py._fields_:
            lines.append(f'_Static_assert(offsetof({cname}, {fld}) == {getattr(py, fld).offset}, "{fld}");')
    lines.append('_Static_assert(FRP_FSM_INIT == 0 && FRP_FSM_WAIT_TARGET == 1 && FRP_FSM_INIT_YAW == 2 && FRP_FSM_GEN_NEW_TRAJ == 3 && FRP_FSM_REPLAN_TRAJ == 4 && FRP_FSM_EXEC_TRAJ == 5, "states");')
    states = (solver.FSM_INIT, solver.FSM_WAIT_TARGET, solver.FSM_INIT_YAW, solver.FSM_GEN_NEW_TRAJ, solver.FSM_REPLAN_TRAJ, solver.FSM_EXEC_TRAJ)
    assert states == (FO.INIT, FO.WAIT_TARGET, FO.INIT_YAW, FO.GEN_NEW_TRAJ, FO.REPLAN_TRAJ, FO.EXEC_TRAJ) == (0, 1, 2, 3, 4, 5)
    assert (FO.CMD_ROTATE_YAW, FO.CMD_PUB_TRAJ, FO.NO_PATH, FO.RESULT_IDLE) == (solver.CMD_ROTATE_YAW, solver.CMD_PUB_TRAJ, solver.ASTAR_NO_PATH, solver.TICK_RESULT_IDLE)
    for inc in ("frp_nmpc.h", "frp_nmpc_fsm.h"):   # through frp_nmpc.h, and on its own; strict C99 plus the C11 assertion
        src = tmp_path / ("layout_" + inc.replace(".", "_") + ".c")
        src.write_text('#include <stddef.h>\n#include "' + inc + '"\n' + "\n".join(lines) + "\nint main(void) { return 0; }\n")
        subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(src) + ".o"])
    c99 = tmp_path / "c99.c"
    c99.write_text('#include "frp_nmpc_fsm.h"\nint main(void) { frp_nmpc_fsm f; f.B = FRP_FSM_EXEC_TRAJ; return f.B - 5; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(c99), "-o", str(c99) + ".o"])


# ---- (iv) the boundary, without a device ----
FRP_ERR_NO_DEVICE, FRP_ERR_ARG = -1001, -1003
FSM_GOOD = dict(B=4, **{n: 0x1000 * (i + 1) for i, (n, _) in enumerate(solver.Fsm._fields_[1:])})
IN_GOOD = dict(N=20, Ts=0.05, mass=0.74, g=9.81, **{n: 0x40000 + 0x1000 * i for i, (n, _) in enumerate(solver.FsmExecIn._fields_[4:])})
A, Bp, C = 0x80000, 0x81000, 0x82000


def _has_gpu():
    try:
        return solver.lib().frp_nmpc_device_count() > 0
    except Exception:
        return False


def _fsm(**kw):
    a = dict(FSM_GOOD); a.update(kw)
    return solver.Fsm(*[a[f] for f, _ in solver.Fsm._fields_])


def _calls(f, in_kw=None, bound=0.5, ptr=(A, Bp, C)):
    """Every entry with the struct f (a solver.Fsm or None); the addresses are never dereferenced on the host and nothing is launched."""
    lib = solver.lib()
    pf = ctypes.byref(f) if f is not None else None
    a, b, c = [ctypes.c_void_p(p) if p else None for p in ptr]
    i = dict(IN_GOOD); i.update(in_kw or {})
    ein = solver.FsmExecIn(*[i[n] for n, _ in solver.FsmExecIn._fields_])
    return dict(goal=lib.frp_nmpc_fsm_goal(pf, a, b, None), force=lib.frp_nmpc_fsm_force(pf, a, b, bound, None), mpc=lib.frp_nmpc_fsm_mpc(pf, a, None),
                safety=lib.frp_nmpc_fsm_safety(pf, a, b, None), exec_begin=lib.frp_nmpc_fsm_exec_begin(pf, ctypes.byref(ein), None),
                exec_end=lib.frp_nmpc_fsm_exec_end(pf, a, b, c, None))


REQUIRED_FSM = [n for n, _ in solver.Fsm._fields_[1:] if n != "mode"]
BAD_FSM = [dict(B=0), dict(B=-3)] + [{n: None} for n in REQUIRED_FSM]
BAD_IN = ([dict(N=1), dict(N=0), dict(N=65), dict(N=-2)] + [{k: v} for k in ("Ts", "mass") for v in (0.0, -0.05, NAN, float("inf"), float("-inf"))] +
          [dict(g=NAN), dict(g=float("inf"))] + [{n: None} for n, _ in solver.FsmExecIn._fields_[4:]])
_ids = lambda bad: ["-".join(f"{k}={v}" for k, v in kw.items()) for kw in bad]


@pytest.mark.parametrize("kw", BAD_FSM, ids=_ids(BAD_FSM))
def test_iv_struct_errors_come_before_any_device_call_in_all_six_entries(kw):
    assert set(_calls(_fsm(**kw)).values()) == {FRP_ERR_ARG}


@pytest.mark.parametrize("kw", BAD_IN, ids=_ids(BAD_IN))
def test_iv_exec_input_errors_come_before_any_device_call(kw):
    assert _calls(_fsm(), in_kw=kw)["exec_begin"] == FRP_ERR_ARG


@pytest.mark.parametrize("bound", [-0.5, NAN, float("inf"), float("-inf"), -1e-300])
def test_iv_a_bad_noise_bound_is_refused(bound):
    assert _calls(_fsm(), bound=bound)["force"] == FRP_ERR_ARG


def test_iv_null_structs_and_null_arguments():
    assert set(_calls(None).values()) == {FRP_ERR_ARG}
    lib = solver.lib()
    f = _fsm()
    assert lib.frp_nmpc_fsm_exec_begin(ctypes.byref(f), None, None) == FRP_ERR_ARG
    r = _calls(f, ptr=(0, Bp, C))
    assert all(r[k] == FRP_ERR_ARG for k in ("goal", "force", "mpc", "safety", "exec_end"))
    r = _calls(f, ptr=(A, 0, C))
    assert all(r[k] == FRP_ERR_ARG for k in ("goal", "force", "safety", "exec_end"))
    assert _calls(f, ptr=(A, Bp, 0))["exec_end"] == FRP_ERR_ARG


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_iv_valid_arguments_without_a_device_fail_loudly():
    """Accepted arguments reach the device check and nothing else: no CPU path.  mode is optional; a bound of 0 is a bound."""
    assert set(_calls(_fsm()).values()) == {FRP_ERR_NO_DEVICE}
    assert set(_calls(_fsm(mode=None, B=1)).values()) == {FRP_ERR_NO_DEVICE}
    assert _calls(_fsm(), bound=0.0)["force"] == FRP_ERR_NO_DEVICE
    assert _calls(_fsm(), in_kw=dict(N=2))["exec_begin"] == FRP_ERR_NO_DEVICE and _calls(_fsm(), in_kw=dict(N=64, g=0.0))["exec_begin"] == FRP_ERR_NO_DEVICE
