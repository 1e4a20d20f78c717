"""The statement of right of way (include/frp_nmpc.h section 20) in NumPy: the order among vehicles, the ranked peer boxes and the hold-and-
release rule.  Written before the kernels.  The boxes are tests/peers_avoid_oracle.py's: its bound (voxel_f), its constants and
tests/peers_oracle.py's distances are imported, the drop order and the clip are its loop's, and the two identities -- every peer outranks
the planner: its rows; the planner outranks every peer: its rows with K = 0 -- bind this loop to AO.boxes itself (the tests assert them).
AO.boxes is not called per planner with a masked have_traj, which states the same thing: at 260 planners that is minutes.  Every
difference, sum and product is a float64 operation of its own, so the device (built without contraction) gives the same bits.  `count`
(a collections.Counter or None) takes one tick per named branch."""
import numpy as np

from . import peers_avoid_oracle as AO
from . import peers_oracle as PO

NO_PATH, CONSUMED = 3, 0                       # FRP_ASTAR_NO_PATH; what AstarPlanner's constructor leaves in status
WAIT_TARGET, EXEC_TRAJ, PUB_END = 1, 5, 2      # FRP_FSM_*, FRP_CMD_PUB_END
BRANCHES_BOXES = ("priority_none", "tie_to_lower_id", "higher_priority_wins", "outranking_peer", "outranked_peer", "stages_skipped", "no_outranking_peer",
                  "exact_fill", "overflow_q", "more_than_64")
BRANCHES_STEP = ("goal_through", "goal_latched", "no_goal", "refused_exec_traj", "refused_no_outrank_boxes", "refused_other_status", "refused_fresh_goal",
                 "enter", "enter_after_drop", "brake_finite", "brake_inf", "bad_odometry", "clear", "not_clear", "count_reset", "release_clear",
                 "release_timeout", "still_holding", "longest_hold", "idle")
INT_STATE = ("holding", "clear_count", "hold_age", "fresh", "holds", "releases", "timeouts", "hold_periods", "longest_hold", "bad")
F64_STATE = ("held_goal", "goal")
FSM_FIELDS = ("state", "have_target", "have_traj", "exec_mpc", "plan_fail_count", "cmd_status", "pub_end")

_tick = AO._tick


def outranks(priority, q, b, count=None):
    """Does q outrank b: a higher priority, or the same and a lower id.  priority None: all zero."""
    pq, pb = (0, 0) if priority is None else (int(priority[q]), int(priority[b]))
    if pq != pb:
        _tick(count, "higher_priority_wins")
        return pq > pb
    _tick(count, "tie_to_lower_id")
    return q < b


def boxes_ranked(state, ent, pre_plan, have_traj, stages, half, R, origin, resolution, grid, Q, priority, count=None):
    """AO.boxes with the order: the stages of peer q's plan are centres for planner b only where q outranks b.  Returns (boxes [B,Q,6], count,
    overflow, dropped_own, outrank_boxes [B] int32, outrank_d2 [B] f64)."""
    state = np.asarray(state, dtype=np.float64)
    B, N = state.shape[0], pre_plan.shape[1]
    R2 = np.float64(R) * np.float64(R)
    inv = np.float64(1.0) / np.float64(resolution)
    half = np.asarray(half, dtype=np.float64)
    D2 = PO.dist2(state[:, :3])
    out = np.zeros((B, Q, 6), dtype=np.int32)
    cnt, overflow, dropped, up_boxes = (np.zeros((B,), dtype=np.int32) for _ in range(4))
    up_d2 = np.full((B,), R2, dtype=np.float64)
    if priority is None:
        _tick(count, "priority_none")
    for b in range(B):
        if not ent[b]:
            continue
        with np.errstate(invalid="ignore"):
            q = np.nonzero(ent & (np.arange(B) != b) & (D2[b] <= R2))[0]
        q = q[np.lexsort((q, D2[b, q]))]
        if q.size > AO.MAX_NEAR:
            _tick(count, "more_than_64")
            overflow[b] = 1
            q = q[:AO.MAX_NEAR]
        own = [AO.voxel_f(state[b, k], origin[k], inv) for k in range(3)]
        rows, n_up, first_up = [], 0, None
        for p in q:
            up = outranks(priority, int(p), b, count)
            _tick(count, "outranking_peer" if up else "outranked_peer")
            if up and first_up is None:
                first_up = D2[b, p]
            centres = [state[p, :3]]
            if have_traj[p] != 0 and up:
                centres += [pre_plan[p, st, 8:11] for st in stages if 0 <= st < N]
            elif have_traj[p] != 0 and len(stages):
                _tick(count, "stages_skipped")
            for c in centres:
                with np.errstate(invalid="ignore", over="ignore"):
                    lo = [AO.voxel_f(np.float64(c[k]) - half[k], origin[k], inv) for k in range(3)]
                    hi = [AO.voxel_f(np.float64(c[k]) + half[k], origin[k], inv) for k in range(3)]
                if not all(abs(v) <= AO.FINITE for v in lo + hi):
                    continue
                if any(hi[k] < 0.0 or lo[k] > float(grid[k] - 1) for k in range(3)):
                    continue
                if all(lo[k] <= own[k] <= hi[k] for k in range(3)):
                    dropped[b] += 1
                    continue
                rows.append([0 if lo[k] < 0.0 else int(lo[k]) for k in range(3)] + [grid[k] - 1 if hi[k] > float(grid[k] - 1) else int(hi[k]) for k in range(3)])
                n_up += 1 if up else 0
        up_boxes[b] = n_up
        if first_up is None:
            _tick(count, "no_outranking_peer")
        else:
            up_d2[b] = first_up
        n = len(rows)
        if n > Q:
            _tick(count, "overflow_q")
            cnt[b] = -n
            continue
        if n:
            out[b, :n] = np.array(rows, dtype=np.int32)
        if n == Q and n:
            _tick(count, "exact_fill")
        cnt[b] = n
    return out, cnt, overflow, dropped, up_boxes, up_d2


def new_yield(B):
    y = {n: np.zeros((B,), dtype=np.int32) for n in INT_STATE}
    y.update({n: np.zeros((B, 3), dtype=np.float64) for n in F64_STATE})
    return y


def yield_reset(y, mask=None):
    sel = np.ones(len(y["holding"]), dtype=bool) if mask is None else np.asarray(mask) != 0
    for n in INT_STATE + F64_STATE:
        y[n][sel] = 0


def stop_point(p, v, a_brake):
    """p + v * (|v| / (2 a_brake)), one rounding per operation; a_brake = +inf gives p."""
    p, v = np.asarray(p, dtype=np.float64), np.asarray(v, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        lead = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) / (np.float64(2.0) * np.float64(a_brake))
        return p + v * lead


def yield_step(y, fsm, end_pt, cmd_end_pt, state, status, outrank_boxes, outrank_d2, goal_in, fresh_in, fleet_have_traj, r_release, n_clear, a_brake, hold_timeout,
               count=None):
    """One frp_nmpc_yield_step, in place: y (new_yield), fsm (dict of FSM_FIELDS [B] int32), cmd_end_pt [B,3], status [B] and fleet_have_traj
    ([B] or None) are written; end_pt [B,3], state [B,9], outrank_boxes, outrank_d2, goal_in / fresh_in (or None) are read."""
    B = len(y["holding"])
    r2 = np.float64(r_release) * np.float64(r_release)
    for b in range(B):
        was = y["holding"][b] != 0
        fin = fresh_in is not None and fresh_in[b] != 0
        fresh = 0
        if fin:
            if was:
                _tick(count, "goal_latched")
                y["held_goal"][b] = goal_in[b]
            else:
                _tick(count, "goal_through")
                y["goal"][b] = goal_in[b]
                fresh = 1
        else:
            _tick(count, "no_goal")
        if not was:
            wants = status[b] == NO_PATH and outrank_boxes[b] > 0 and fsm["state"][b] != EXEC_TRAJ
            if fin and wants:
                _tick(count, "refused_fresh_goal")
            elif status[b] != NO_PATH:
                _tick(count, "idle" if status[b] == CONSUMED else "refused_other_status")
            elif outrank_boxes[b] <= 0:
                _tick(count, "refused_no_outrank_boxes")
            elif fsm["state"][b] == EXEC_TRAJ:
                _tick(count, "refused_exec_traj")
            if wants and not fin:
                od = state[b]
                if not np.all(np.abs(od[:6]) <= AO.FINITE):
                    _tick(count, "bad_odometry")
                    y["bad"][b] += 1
                else:
                    _tick(count, "enter_after_drop" if fsm["have_target"][b] == 0 else "enter")
                    _tick(count, "brake_inf" if np.isinf(a_brake) else "brake_finite")
                    y["held_goal"][b] = end_pt[b]
                    cmd_end_pt[b] = stop_point(od[0:3], od[3:6], a_brake)
                    status[b] = CONSUMED
                    fsm["have_target"][b] = 0
                    fsm["state"][b] = WAIT_TARGET
                    fsm["exec_mpc"][b] = 0
                    fsm["plan_fail_count"][b] = 0
                    fsm["have_traj"][b] = 0
                    if fleet_have_traj is not None:
                        fleet_have_traj[b] = 0
                    fsm["cmd_status"][b] = PUB_END
                    fsm["pub_end"][b] = 1
                    y["holding"][b] = 1
                    y["holds"][b] += 1
                    y["hold_age"][b] = 0
                    y["clear_count"][b] = 0
        else:
            age = y["hold_age"][b] + 1
            y["hold_age"][b] = age
            y["hold_periods"][b] += 1
            if age > y["longest_hold"][b]:
                _tick(count, "longest_hold")
                y["longest_hold"][b] = age
            clear = bool(outrank_d2[b] > r2) or outrank_boxes[b] == 0
            if clear:
                _tick(count, "clear")
                cc = y["clear_count"][b] + 1
            else:
                _tick(count, "count_reset" if y["clear_count"][b] > 0 else "not_clear")
                cc = 0
            y["clear_count"][b] = cc
            timeout = cc < n_clear and age >= hold_timeout
            if cc >= n_clear or timeout:
                _tick(count, "release_timeout" if timeout else "release_clear")
                y["goal"][b] = y["held_goal"][b]
                fresh = 1
                y["holding"][b] = 0
                y["releases"][b] += 1
                if timeout:
                    y["timeouts"][b] += 1
            else:
                _tick(count, "still_holding")
        y["fresh"][b] = fresh
