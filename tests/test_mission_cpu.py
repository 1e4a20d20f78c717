"""CPU tests of the mission's specification (include/frp_nmpc.h section 17): tests/mission_oracle.py against scenarios worked by hand, the
branches the synthetic cases of tests/mission_cases.py take (a gap fails), the clock's formula against FleetFSM.clock_for, the conditions
the random-mode cases have to meet on their map, the independence of a draw from sharding and from R, and the C-ABI: every argument rule
through the library (FRP_ERR_ARG comes before the device is looked for), the header's placement and the export order."""
import ctypes
import math
import os

import numpy as np
import pytest

from forces_resilient_planner_amd import build, capi, solver

from . import mission_cases as MC
from . import mission_oracle as MO

NAN = float("nan")
ROUTE = [[[1.0, 2.0, 1.5], [3.0, 2.0, 1.0], [3.0, 4.0, 1.25]]]      # one vehicle, W = 3


def _route_par(**kw):
    a = dict(route=ROUTE, route_len=[3], arrive_radius=0.5, dwell=0.5, leg_timeout=0.0)
    a.update(kw)
    return MO.params(**a)


def _state(v):
    return {k: (list(x) if isinstance(x, list) else x) for k, x in v.items()}


def _expect(v, **kw):
    want = MO.new_vehicle()
    want.update(kw)
    assert _state(v) == want, (_state(v), want)


# ---- the scenarios, by hand ----
def test_a_route_is_flown_leg_by_leg_and_ends_done():
    par, v = _route_par(), MO.new_vehicle()
    # t_mark = 0 at first; now = 0.25 is inside the dwell of 0.5: nothing
    assert MO.step(v, par, 0, 0.25, 1, 0, [0, 0, 0], [0, 0, 0]) == {"idle:dwell"}
    _expect(v)
    # the dwell boundary: now - t_mark == dwell issues waypoint 0
    assert MO.step(v, par, 0, 0.5, 1, 0, [0, 0, 0], [0, 0, 0]) == {"route:issue"}
    _expect(v, phase=1, leg=0, issued=1, t_mark=0.5, goal=[1.0, 2.0, 1.5], fresh=1)
    # in flight with the target held: fresh falls back to 0, nothing else moves
    assert MO.step(v, par, 0, 0.75, 1, 1, [1.0, 2.0, 1.2], [0.5, 1.0, 1.2]) == {"flying:on_time"}
    _expect(v, phase=1, leg=0, issued=1, t_mark=0.5, goal=[1.0, 2.0, 1.5])
    # the target is let go 0.25 + 0.25 + 0 -> d2 = 0.125 <= 0.25: reached after 1.5 s; the dwell starts at now
    assert MO.step(v, par, 0, 2.0, 1, 0, [1.0, 2.0, 1.2], [0.75, 1.75, 1.2]) == {"flying:reached", "flying:leg_time_max", "idle:dwell"}
    _expect(v, leg=0, issued=1, reached=1, t_mark=2.0, leg_time_sum=1.5, leg_time_max=1.5, goal=[1.0, 2.0, 1.5])
    assert MO.step(v, par, 0, 2.5, 1, 0, [1.0, 2.0, 1.2], [0.75, 1.75, 1.2]) == {"route:issue"}
    _expect(v, phase=1, leg=1, issued=2, reached=1, t_mark=2.5, leg_time_sum=1.5, leg_time_max=1.5, goal=[3.0, 2.0, 1.0], fresh=1)
    # let go a metre away: dropped; a shorter reached leg later leaves leg_time_max
    assert MO.step(v, par, 0, 3.0, 1, 0, [3.0, 2.0, 1.2], [2.0, 2.0, 1.2]) == {"flying:dropped", "idle:dwell"}
    _expect(v, leg=1, issued=2, reached=1, dropped=1, t_mark=3.0, leg_time_sum=1.5, leg_time_max=1.5, goal=[3.0, 2.0, 1.0])
    assert MO.step(v, par, 0, 3.5, 1, 0, [3.0, 2.0, 1.2], [2.0, 2.0, 1.2]) == {"route:issue"}
    assert MO.step(v, par, 0, 4.0, 1, 0, [3.0, 4.0, 1.2], [3.0, 4.0, 1.2]) == {"flying:reached", "idle:dwell"}
    _expect(v, leg=2, issued=3, reached=2, dropped=1, t_mark=4.0, leg_time_sum=2.0, leg_time_max=1.5, goal=[3.0, 4.0, 1.25])
    # leg + 1 == route_len: DONE, and DONE stays
    assert MO.step(v, par, 0, 4.5, 1, 0, [3.0, 4.0, 1.2], [3.0, 4.0, 1.2]) == {"route:done"}
    _expect(v, phase=2, leg=2, issued=3, reached=2, dropped=1, t_mark=4.0, leg_time_sum=2.0, leg_time_max=1.5, goal=[3.0, 4.0, 1.25])
    assert MO.step(v, par, 0, 9.0, 1, 0, [3.0, 4.0, 1.2], [3.0, 4.0, 1.2]) == {"done:leaves"}
    _expect(v, phase=2, leg=2, issued=3, reached=2, dropped=1, t_mark=4.0, leg_time_sum=2.0, leg_time_max=1.5, goal=[3.0, 4.0, 1.25])


def test_b_a_looped_route_wraps_and_an_arrival_without_dwell_issues_in_the_same_call():
    par, v = _route_par(loop=True, dwell=0.0, route_len=[2]), MO.new_vehicle()
    assert MO.step(v, par, 0, 1.0, 1, 0, [0, 0, 0], [0, 0, 0]) == {"route:issue"}
    assert MO.step(v, par, 0, 2.0, 1, 0, [1.0, 2.0, 1.2], [1.0, 2.0, 1.2]) == {"flying:reached", "flying:leg_time_max", "route:issue"}
    _expect(v, phase=1, leg=1, issued=2, reached=1, t_mark=2.0, leg_time_sum=1.0, leg_time_max=1.0, goal=[3.0, 2.0, 1.0], fresh=1)
    # leg 2 of a route of two: waypoint 0 again -- the third slot of the row is never read
    assert MO.step(v, par, 0, 4.0, 1, 0, [3.0, 2.0, 1.2], [3.0, 2.0, 1.2]) == {"flying:reached", "flying:leg_time_max", "route:issue", "route:wrap"}
    _expect(v, phase=1, leg=2, issued=3, reached=2, t_mark=4.0, leg_time_sum=3.0, leg_time_max=2.0, goal=[1.0, 2.0, 1.5], fresh=1)


def test_c_a_timeout_abandons_the_leg_and_issues_the_next_goal_in_the_same_call():
    par, v = _route_par(dwell=0.2, leg_timeout=1.0), MO.new_vehicle()
    assert MO.step(v, par, 0, 0.5, 1, 0, [0, 0, 0], [0, 0, 0]) == {"route:issue"}
    # now - t_mark == leg_timeout is on time: the comparison is >
    assert MO.step(v, par, 0, 1.5, 1, 1, [1.0, 2.0, 1.2], [0, 0, 1.2]) == {"flying:on_time"}
    # 1.75 - 0.5 > 1: abandoned, and waypoint 1 at once although 1.75 - (1.75 - 0.2) rounds below the dwell of 0.2
    assert 1.75 - (1.75 - 0.2) < 0.2
    assert MO.step(v, par, 0, 1.75, 1, 1, [1.0, 2.0, 1.2], [0, 0, 1.2]) == {"flying:abandoned", "route:issue"}
    _expect(v, phase=1, leg=1, issued=2, abandoned=1, t_mark=1.75, goal=[3.0, 2.0, 1.0], fresh=1)
    # without odometry the abandoned vehicle waits IDLE with t_mark = now - dwell
    v2 = MO.new_vehicle()
    MO.step(v2, par, 0, 0.5, 1, 0, [0, 0, 0], [0, 0, 0])
    assert MO.step(v2, par, 0, 2.0, 0, 1, [1.0, 2.0, 1.2], [0, 0, 1.2]) == {"flying:abandoned", "idle:no_odom"}
    _expect(v2, leg=0, issued=1, abandoned=1, t_mark=2.0 - 0.2, goal=[1.0, 2.0, 1.5])
    # a timeout of 0 never abandons
    par0, v3 = _route_par(leg_timeout=0.0), MO.new_vehicle()
    MO.step(v3, par0, 0, 0.5, 1, 0, [0, 0, 0], [0, 0, 0])
    assert MO.step(v3, par0, 0, 1.0e9, 1, 1, [1.0, 2.0, 1.2], [0, 0, 1.2]) == {"flying:on_time"}


def test_d_no_odometry_a_nan_position_a_nan_clock_and_a_moved_end_point():
    par, v = _route_par(dwell=0.0), MO.new_vehicle()
    assert MO.step(v, par, 0, 1.0, 0, 0, [0, 0, 0], [0, 0, 0]) == {"idle:no_odom"}
    _expect(v)
    assert MO.step(v, par, 0, NAN, 1, 0, [0, 0, 0], [0, 0, 0]) == {"idle:dwell"}                    # NaN - 0 >= 0 fails
    _expect(v)
    assert MO.step(v, par, 0, 1.0, 1, 0, [0, 0, 0], [NAN, 0, 0]) == {"route:issue"}                 # a waypoint is issued as it is
    # the position is NaN when the target goes: d2 <= r2 fails, dropped
    assert MO.step(v, par, 0, 2.0, 1, 0, [1.0, 2.0, 1.2], [1.0, NAN, 1.2]) == {"flying:dropped", "route:issue"}
    _expect(v, phase=1, leg=1, issued=2, dropped=1, t_mark=2.0, goal=[3.0, 2.0, 1.0], fresh=1)
    # the safety search moved the end point to (3.5, 2.5, 1.4): arrival is measured THERE, z included
    assert MO.step(v, par, 0, 3.0, 1, 0, [3.5, 2.5, 1.4], [3.0, 2.0, 1.0]) == {"flying:dropped", "route:issue"}     # 0.25 + 0.25 + 0.16 > 0.25
    assert MO.step(v, par, 0, 4.0, 1, 0, [3.5, 4.25, 1.5], [3.25, 4.0, 1.25]) == {"flying:reached", "flying:leg_time_max", "route:done"}   # 3 x 0.0625 <= 0.25
    _expect(v, phase=2, leg=2, issued=3, reached=1, dropped=2, t_mark=4.0, leg_time_sum=1.0, leg_time_max=1.0, goal=[3.0, 4.0, 1.25])


@pytest.mark.parametrize("n", [0, 4, -1])
def test_e_a_route_len_outside_1_to_w_ends_the_mission_and_reads_no_waypoint(n):
    par, v = _route_par(dwell=0.0, route_len=[n]), MO.new_vehicle()
    par["route"] = [[[NAN] * 3] * 3]
    assert MO.step(v, par, 0, 1.0, 1, 0, [0, 0, 0], [0, 0, 0]) == {"route:bad_len"}
    _expect(v, phase=2)


def test_f_random_mode_by_hand():
    par = MO.params(goal_box=(-2.0, 2.0, 10.0, 12.0), min_dist=1.0, max_dist=3.0, R=2, seed=7, id0=40, dwell=0.0)
    cand = [MO.candidate(par, 3, 0, c) for c in range(6)]
    assert all(-2.0 <= x < 2.0 and 10.0 <= y < 12.0 for x, y in cand) and len(set(cand)) == 6
    # the candidate is the header's formula on the generator of section 15
    from .disturbance_oracle import mix, stream_key
    h = mix((stream_key(7, 43, 0) + 0x4D495353) % 2 ** 64)
    assert cand[2] == (-2.0 + (mix((h + 4) % 2 ** 64) >> 11) / 2.0 ** 53 * 4.0, 10.0 + (mix((h + 5) % 2 ** 64) >> 11) / 2.0 ** 53 * 2.0)
    # a position from which candidates 0 ... 3 are out of [min_dist, max_dist] and 4 is inside
    far = (cand[4][0] - 1.5, cand[4][1])
    d = lambda c, p: math.hypot(c[0] - p[0], c[1] - p[1])
    v = MO.new_vehicle()
    pos = [far[0], far[1], 1.2]
    n_bad = next(c for c in range(6) if 1.0 <= d(cand[c], far) <= 3.0)
    calls = 0
    while v["phase"] == MO.IDLE:
        met = MO.step(v, par, 3, 5.0 + calls, 1, 0, [0, 0, 0], pos)
        calls += 1
    assert calls == n_bad // 2 + 1 and v["blocked"] == n_bad // 2 and v["tries"] == 0 and v["leg"] == 0 and v["fresh"] == 1
    assert v["goal"] == [cand[n_bad][0], cand[n_bad][1], 1.2] and v["t_mark"] == 5.0 + calls - 1
    # a NaN position is within no distance band: blocked, tries += R
    w = MO.new_vehicle()
    assert MO.step(w, par, 3, 5.0, 1, 0, [0, 0, 0], [NAN, 0.0, 1.2]) == {"random:distance", "random:blocked"}
    _expect(w, blocked=1, tries=2)


def test_g_reset_and_the_goal_callback():
    v = MO.new_vehicle()
    MO.step(v, _route_par(dwell=0.0), 0, 1.0, 1, 0, [0, 0, 0], [0, 0, 0])
    MO.reset(v)
    _expect(v)
    assert MO.goal_callback(0, [9.0, 9.0, 9.0], [1.0, 2.0, 1.5], 1) == (1, [1.0, 2.0, 1.2])
    assert MO.goal_callback(0, [9.0, 9.0, 9.0], [1.0, 2.0, 1.5], 0) == (0, [9.0, 9.0, 9.0])


# ---- the synthetic cases ----
def test_h_the_synthetic_cases_take_every_branch():
    count = {b: 0 for b in MC.BRANCHES}
    for name in MC.CASES:
        _, frames, met = MC.run(name, 260)
        assert len(frames) == MC.CALLS
        assert met <= set(MC.BRANCHES), met - set(MC.BRANCHES)          # a branch the list does not know is a gap of the list
        for b in met:
            count[b] += 1
    missing = [b for b, n in count.items() if n == 0]
    assert not missing, missing
    # the small sizes on their own: B = 5 still arrives, drops, times out and draws
    small = set().union(*(MC.run(name, 5)[2] for name in MC.CASES))
    assert {"flying:reached", "flying:dropped", "flying:abandoned", "route:issue", "random:issue", "random:blocked"} <= small


def test_i_the_clock_is_clock_for_to_the_bit():
    for k in (0, 1, 7, 2 ** 20, 2 ** 40):
        for t0 in (0.0, MC.T0, 1.0e-3):
            for steps in (1, 5):
                want = solver.FleetFSM.clock_for(t0 + 0.05 * k, steps)
                got = MO.clock(k, t0, 0.05, solver.FSM_EXEC_PERIOD, steps + 2)
                assert [x.hex() for x in got] == [float(x).hex() for x in want], (k, t0, steps)
    # ... which a repeated += 0.05 is not
    t = 0.0
    for _ in range(7):
        t += 0.05
    assert t != MO.clock(7, 0.0, 0.05, 0.01, 1)[0]


def test_j_the_random_cases_meet_their_conditions_on_the_map():
    m = MC.map_oracle()
    assert tuple(m.grid_size) == (40, 40, 20)
    for B in MC.SIZES:
        _, frames, _ = MC.run("random_r4_open", B)
        assert np.all(frames[0][1]["issued"][frames[0][0]["have_odom"] != 0] == 1), B      # a goal within R = 4 tries, for every vehicle that may fly
        assert np.all(frames[-1][1]["issued"] >= 1), B
        for name in ("random_r4_walled", "random_r4_edge"):
            _, frames, met = MC.run(name, B)
            last = frames[-1][1]
            assert np.all(last["issued"] == 0) and np.all(last["blocked"] >= MC.CALLS - 2) and np.all(last["tries"] == 4 * last["blocked"]), (name, B)
            assert "random:occupied" in met and "random:issue" not in met
    assert "random:issue_later" in MC.run("random_r4_open", 5)[2] and "random:occupied" in MC.run("random_r4_open", 5)[2]
    assert "random:issue_later" in MC.run("random_r1_open", 260)[2]


def test_k_a_fleet_is_its_halves_and_one_call_of_four_tries_is_four_calls_of_one():
    for name in ("random_r4", "random_r4_open", "route_w3"):
        _, whole, _ = MC.run(name, 10)
        _, lo, _ = MC.run(name, 5, 0)
        _, hi, _ = MC.run(name, 5, 5)
        for n in range(MC.CALLS):
            for f, a in whole[n][1].items():
                both = np.concatenate([lo[n][1][f], hi[n][1][f]])
                assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, both.view(np.uint64) if both.dtype == np.float64 else both), (name, n, f)
    # R: the same vehicle, position and time; what differs is how often `blocked` is counted
    for name, with_map in (("random_r4", False), ("random_r4_open", True), ("random_r4_walled", True)):
        par4, occ = MC.case_params(name, 12)
        par1, _ = MC.case_params(name, 12, R=1)
        later = 0
        for b in range(12):
            a, c = MO.new_vehicle(), MO.new_vehicle()
            pos = MC.start_pos(b)
            MO.step(a, par4, b, 1.0, 1, 0, [0, 0, 0], pos, occ)
            for _ in range(4):
                MO.step(c, par1, b, 1.0, 1, int(c["phase"] == MO.FLYING), [0, 0, 0], pos, occ)     # (once it flies, the target is held)
            later += c["blocked"] > 0 and c["issued"] == 1
            for f in ("phase", "leg", "tries", "issued", "t_mark", "goal"):
                assert a[f] == c[f], (name, b, f)
            assert (a["blocked"], c["blocked"]) in ((0, c["blocked"]), (1, 4)) and c["blocked"] <= 4
        assert later > 0 or name != "random_r4_open"


# ---- the C-ABI ----
def good_struct(route_mode):
    """A valid frp_nmpc_mission whose pointers are never followed (the refusals come first): (struct, keep-alive)."""
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    m = capi.MissionArgs(1, 3 if route_mode else 0, 0 if route_mode else 4, 0, 0.3, 0.0, 0.0, (ctypes.c_double * 4)(-1.0, 1.0, -1.0, 1.0), 1.2, 0.0, 5.0, 1.2, 1, 0,
                         p if route_mode else None, p if route_mode else None, *([p] * 13))
    return m, buf


def good_fsm():
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    return capi.Fsm(1, *([p] * (len(capi.Fsm._fields_) - 1))), buf


def good_map():
    """A valid 40 x 40 x 20 map description and its workspace size; the pointers are never followed."""
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    m = capi.OccMap((ctypes.c_double * 3)(*MC.MAP_ORIGIN), (ctypes.c_double * 3)(*MC.MAP_SIZE), MC.MAP_RES, (ctypes.c_int * 3)(40, 40, 20), 0.12, 0.97, 0.8,
                    (ctypes.c_double * 3)(6.0, 6.0, 3.0), p, p)
    return m, buf, 40 * 40 * 4


def refusals():
    """(what, a function of the library that makes the refused call, keep-alive) for every rule of the header."""
    out = []
    scratch = (ctypes.c_double * 16)()
    p = ctypes.addressof(scratch)
    fsm, fkeep = good_fsm()
    omap, mkeep, ws_bytes = good_map()
    body = capi.OccMapBody(0.27, 0.0425)
    keep = [scratch, fsm, fkeep, omap, mkeep, body]

    def step(m, f=fsm, state=p, clock=p, mp=None, bd=None, ws=None, nb=0):
        r, fr = ctypes.byref(m), ctypes.byref(f) if f is not None else None
        return lambda l: l.frp_nmpc_mission_step(r, fr, state, clock, ctypes.byref(mp) if mp is not None else None, ctypes.byref(bd) if bd is not None else None, ws, nb, None)

    def bad(what, change, route_mode, **kw):
        m, k = good_struct(route_mode)
        change(m)
        keep.extend([m, k])
        out.append((what, step(m, **kw), None))

    for mode in (True, False):
        tag = "route" if mode else "random"
        for field in ("phase", "leg", "tries", "t_mark", "issued", "reached", "dropped", "abandoned", "blocked", "leg_time_sum", "leg_time_max", "goal", "fresh"):
            bad(f"{tag}: {field} NULL", lambda m, field=field: setattr(m, field, None), mode)
        for v in (0, -2):
            bad(f"{tag}: B = {v}", lambda m, v=v: setattr(m, "B", v), mode)
        for field in ("arrive_radius", "dwell", "leg_timeout"):
            for v in (-1e-9, NAN, float("inf")):
                bad(f"{tag}: {field} = {v}", lambda m, field=field, v=v: setattr(m, field, v), mode)
        bad(f"{tag}: state NULL", lambda m: None, mode, state=None)
        bad(f"{tag}: clock NULL", lambda m: None, mode, clock=None)
        bad(f"{tag}: fsm NULL", lambda m: None, mode, f=None)
        for field in ("have_odom", "have_target", "end_pt"):
            f2, k2 = good_fsm()
            setattr(f2, field, None)
            keep.extend([f2, k2])
            bad(f"{tag}: fsm.{field} NULL", lambda m: None, mode, f=f2)
        f3, k3 = good_fsm()
        f3.B = 2
        keep.extend([f3, k3])
        bad(f"{tag}: fsm.B != B", lambda m: None, mode, f=f3)
    # the modes
    bad("neither mode", lambda m: setattr(m, "R", 0), False)
    bad("both modes", lambda m: setattr(m, "R", 4), True)
    for v in (0, -1):
        bad(f"route: W = {v}", lambda m, v=v: setattr(m, "W", v), True)
    bad("route: route_len NULL", lambda m: setattr(m, "route_len", None), True)
    bad("route: a map", lambda m: None, True, mp=omap, bd=body, ws=p, nb=ws_bytes)
    for v in (-1, capi.MISSION_MAX_TRIES + 1, 1 << 30):
        bad(f"random: R = {v}", lambda m, v=v: setattr(m, "R", v), False)
    bad("random: W = 3", lambda m: setattr(m, "W", 3), False)
    bad("random: route_len given", lambda m: setattr(m, "route_len", p), False)

    def setbox(i, v):
        def f(m):
            m.goal_box[i] = v
        return f
    for i in range(4):
        for v in (NAN, float("inf"), -float("inf")):
            bad(f"random: goal_box[{i}] = {v}", setbox(i, v), False)
    bad("random: empty box in x", setbox(1, -1.0), False)
    bad("random: inverted box in y", setbox(2, 2.0), False)
    for v in (NAN, float("inf")):
        bad(f"random: z_goal = {v}", lambda m, v=v: setattr(m, "z_goal", v), False)
    for field in ("min_dist", "max_dist"):
        for v in (-0.5, NAN, float("inf")):
            bad(f"random: {field} = {v}", lambda m, field=field, v=v: setattr(m, field, v), False)
    bad("random: min_dist > max_dist", lambda m: setattr(m, "min_dist", 6.0), False)
    # the map
    bad("map without body", lambda m: None, False, mp=omap, ws=p, nb=ws_bytes)
    bad("map without workspace", lambda m: None, False, mp=omap, bd=body, nb=ws_bytes)
    bad("body without map", lambda m: None, False, bd=body)
    bad("workspace too small", lambda m: None, False, mp=omap, bd=body, ws=p, nb=ws_bytes - 1)
    bad_map, bk, _ = good_map()
    bad_map.resolution = 0.0
    keep.extend([bad_map, bk])
    bad("an invalid map", lambda m: None, False, mp=bad_map, bd=body, ws=p, nb=ws_bytes)
    bad_grid, gk, _ = good_map()
    bad_grid.grid[0] = 41
    keep.extend([bad_grid, gk])
    bad("a grid that is not the map's", lambda m: None, False, mp=bad_grid, bd=body, ws=p, nb=ws_bytes)
    bad("half extents beyond 31", lambda m: setattr(m, "inflate_ratio", 12.0), False, mp=omap, bd=body, ws=p, nb=ws_bytes)     # ceil(0.27 * 12 / 0.1) = 33
    bad("inflate_ratio NaN", lambda m: setattr(m, "inflate_ratio", NAN), False, mp=omap, bd=body, ws=p, nb=ws_bytes)
    # clock and reset
    out += [(w, c, None) for w, c in [
        ("clock k NULL", lambda l: l.frp_nmpc_mission_clock(None, 0.0, 0.05, 0.01, 3, p, 1, None)), ("clock out NULL", lambda l: l.frp_nmpc_mission_clock(p, 0.0, 0.05, 0.01, 3, None, 1, None)),
        ("clock n = 0", lambda l: l.frp_nmpc_mission_clock(p, 0.0, 0.05, 0.01, 0, p, 1, None)), ("clock n = 65", lambda l: l.frp_nmpc_mission_clock(p, 0.0, 0.05, 0.01, 65, p, 1, None)),
        ("clock t0 NaN", lambda l: l.frp_nmpc_mission_clock(p, NAN, 0.05, 0.01, 3, p, 1, None)), ("clock period < 0", lambda l: l.frp_nmpc_mission_clock(p, 0.0, -0.05, 0.01, 3, p, 1, None)),
        ("clock period inf", lambda l: l.frp_nmpc_mission_clock(p, 0.0, float("inf"), 0.01, 3, p, 1, None)), ("clock dt NaN", lambda l: l.frp_nmpc_mission_clock(p, 0.0, 0.05, NAN, 3, p, 1, None)),
        ("clock advance < 0", lambda l: l.frp_nmpc_mission_clock(p, 0.0, 0.05, 0.01, 3, p, -1, None)), ("reset ms NULL", lambda l: l.frp_nmpc_mission_reset(None, None, None))]]
    for field in ("phase", "leg", "goal", "fresh", "leg_time_max"):
        m, k = good_struct(True)
        setattr(m, field, None)
        keep.extend([m, k])
        out.append((f"reset {field} NULL", lambda l, r=ctypes.byref(m): l.frp_nmpc_mission_reset(r, None, None), None))
    m, k = good_struct(False)
    m.B = 0
    keep.extend([m, k])
    out.append(("reset B = 0", lambda l, r=ctypes.byref(m): l.frp_nmpc_mission_reset(r, None, None), None))
    return out, keep


def test_l_the_c_abi_refuses_every_bad_argument_before_it_looks_for_a_device():
    l = solver.lib()
    table, keep = refusals()
    assert len(table) > 110
    for what, call, _ in table:
        assert call(l) == capi.FRP_ERR_ARG, what
    # ... and the good structs are not refused for their arguments: without a device the answer is FRP_ERR_NO_DEVICE (with one these
    # host pointers must not be launched on, so the call is made on a machine without a device alone)
    if l.frp_nmpc_device_count() == 0:
        fsm, fk = good_fsm()
        omap, mk, nb = good_map()
        body = capi.OccMapBody(0.27, 0.0425)
        p = ctypes.addressof(fk)
        for mode in (True, False):
            m, k = good_struct(mode)
            assert l.frp_nmpc_mission_step(ctypes.byref(m), ctypes.byref(fsm), p, p, None, None, None, 0, None) == capi.FRP_ERR_NO_DEVICE
            assert l.frp_nmpc_mission_reset(ctypes.byref(m), None, None) == capi.FRP_ERR_NO_DEVICE
        m, k = good_struct(False)
        assert l.frp_nmpc_mission_step(ctypes.byref(m), ctypes.byref(fsm), p, p, ctypes.byref(omap), ctypes.byref(body), p, nb, None) == capi.FRP_ERR_NO_DEVICE
        assert l.frp_nmpc_mission_clock(p, 0.0, 0.05, 0.01, 3, p, 1, None) == capi.FRP_ERR_NO_DEVICE


def test_m_the_header_places_section_17_and_the_unit_is_built_like_its_neighbours():
    hdr = open(os.path.join(build.ROOT, "include", "frp_nmpc.h")).read()
    assert "#define FRP_NMPC_ABI_VERSION 7" in hdr and solver.ABI_VERSION == 7
    at = {n: hdr.index(f"---- ({n}) ") for n in (14, 15, 16, 17)}
    assert hdr.rindex('#include "frp_nmpc_') < at[15] < at[16] < at[17] < at[14]
    sec = hdr[at[17]:at[14]]
    assert "NO REFERENCE COUNTERPART" in sec and "CHOSEN, not derived" in sec and "typedef struct frp_nmpc_mission {" in sec
    names = ["frp_nmpc_mission_step", "frp_nmpc_mission_clock", "frp_nmpc_mission_reset"]
    i = solver.EXPORTS.index(names[0])
    assert solver.EXPORTS[i:i + 3] == names and solver.EXPORTS[i - 1] == "frp_nmpc_sensor_noise_scan" and solver.EXPORTS[i + 3] == "frp_nmpc_flight_record_samples"
    assert all(hasattr(solver.lib(), n) for n in names)
    assert capi.C_TYPES[capi.MissionArgs] == ("frp_nmpc_mission", "frp_nmpc.h") and solver.Mission.__module__.endswith(".flight")
    assert (capi.MISSION_IDLE, capi.MISSION_FLYING, capi.MISSION_DONE, capi.MISSION_TAG) == (MO.IDLE, MO.FLYING, MO.DONE, MO.TAG)
    assert capi.MISSION_TAG not in (capi.SENSOR_NOISE_TAG_STATE, capi.SENSOR_NOISE_TAG_DEPTH, capi.SENSOR_NOISE_TAG_SCAN)
    assert "frp_mission.hip" in build.SOURCES and build.PER_SOURCE_FLAGS["frp_mission.hip"] == ["-ffp-contract=off"]
    code = lambda f: "\n".join(ln for ln in open(os.path.join(build.CSRC, f)).read().splitlines() if not ln.lstrip().startswith("//"))
    src = code("frp_mission.hip")
    assert '#include "frp_disturbance.hpp"' in src and '#include "frp_occmap_check.hpp"' in src
    assert "__shared__" not in src and "atomic" not in src and "asm" not in src and "__syncthreads" not in src
    assert "0x9E3779B97F4A7C15" not in src and "surround_free(" in src                       # the generator is included, not copied
    chk = code("frp_occmap_check.hip")
    assert '#include "frp_occmap_check.hpp"' in chk and "bool surround_free(" not in chk and "bool surround_free(" in code("frp_occmap_check.hpp")
    for doc in ("README.md", "DESIGN.md"):
        assert "Mission" in open(os.path.join(build.ROOT, doc)).read(), doc
