"""A deterministic script for the fleet state machine (include/frp_nmpc_fsm.h): B planners, PERIODS periods of goals, forces, odometry,
safety verdicts, exec steps with their A* statuses, and tick results, written straight into the arrays the six entry points read -- no map,
no search and no solve is needed.  The planner's role is b % 16; roles 0-13 each walk one path through NMPCManage (the comments name
it), roles 14 and 15 draw their inputs from a seeded generator.  The tick result of a planner is scripted only while it executes
(exec_mpc != 0 in the oracle, which the generator runs in lock-step); otherwise it is RESULT_IDLE, as frp_nmpc_tick_end reports it.

A period is, in this order: host writes (have_odom) -> goal -> force -> safety -> STEPS exec steps (exec_begin, the scripted A* status,
exec_end) -> mpc.  The odometry sits at (0, 0, 1); only its yaw (slot 8) moves.  A goal at (4, 0, .) makes dir = (4, 0): atan2 is exactly 0."""
import numpy as np

from . import fsm_oracle as FO

B, N, PERIODS, STEPS, TS, MASS, G, BOUND = 48, 20, 14, 2, 0.05, 0.74, 9.81, 0.5
ROLES = 16


def sequence(B=B, N=N, periods=PERIODS, seed=0):
    """Returns a list of events, each a dict with `kind`:
      host   name, idx, value                       written into the state array `name` before the next call
      goal   goal [B,3], fresh [B]
      force  force [B,3], fresh [B]
      safety goal_blocked [B], first_hit [B]
      exec   state [B,9], pre_plan [B,N,17], exit_code [B], t_cur [B], now (float), astar_status [B]
      mpc    result [B]"""
    rng = np.random.default_rng(seed)
    role = np.arange(B) % ROLES
    at = lambda r: np.nonzero(role == r)[0]
    fleet = [FO.Planner() for _ in range(B)]
    events = []
    yaw = np.zeros(B)
    for p in range(periods):
        # ---- defaults of the period ----
        goal = np.zeros((B, 3)); gfresh = np.zeros(B, dtype=np.int32)
        force = np.zeros((B, 3)); ffresh = np.zeros(B, dtype=np.int32)
        blocked = np.zeros(B, dtype=np.int32); first_hit = np.full(B, -1, dtype=np.int32)
        status = np.full((STEPS, B), FO.REACH_END, dtype=np.int32)
        exit_code = np.ones(B, dtype=np.int32)
        t_cur = np.stack([np.full(B, 0.0625 + 0.01 * k) for k in range(STEPS)])
        want = np.ones(B, dtype=np.int32)          # the tick result of a planner that executes
        odom_from = {3: 3}                         # role 3 hears its first odometry at period 3, everybody else at 0
        pre_plan = rng.normal(size=(B, N, 17)); pre_plan[:, :, 3] = 7.3 + 0.1 * pre_plan[:, :, 3]; pre_plan[:, :, 14:17] *= 0.2

        def goal_to(r, xyz):
            goal[at(r)] = xyz; gfresh[at(r)] = 1

        def force_on(r, xyz):
            force[at(r)] = xyz; ffresh[at(r)] = 1

        for r in range(14):
            if p == odom_from.get(r, 0):
                events.append(dict(kind="host", name="have_odom", idx=at(r), value=1))
        for r in (0, 1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13):
            if p == 0:
                goal_to(r, (0.0, 4.0, 0.0) if r == 1 else (4.0, 0.0, 0.0))
        # 0: a whole life: aligned at once, plans at period 2, executes, reaches the end (-1, then 0), takes a second goal behind it
        #    (period 7: a yaw rotation), turns, plans again
        if p == 5: want[at(0)] = -1
        if p == 6: want[at(0)] = 0
        if p == 7: goal_to(0, (-3.0, 2.0, 5.0))
        if p >= 8: yaw[at(0)] = 2.5
        # 1: the goal is at +90 degrees: callInitYaw at period 1, turning for two periods, aligned at 3; a NEW goal while executing
        #    (period 5): trigger && exec_mpc -> REPLAN_TRAJ from the plan
        if p >= 3: yaw[at(1)] = 1.5
        if p == 3: status[:, at(1)] = FO.REACH_HORIZON
        if p == 5: goal_to(1, (4.0, 0.0, 0.0))
        # 2: forces: quiet (3), a step with a target (4: REPLAN_TRAJ; t_cur < 0 -> from the odometry), steady (5), fierce (6: REPLAN_TRAJ
        #    overwritten by WAIT_TARGET), and one more that is no longer considered (8)
        if p == 3: force_on(2, (0.25, 0.125, -0.25))
        if p == 4: force_on(2, (2.0, 0.0, 0.0)); t_cur[:, at(2)] = -0.01
        if p == 5: force_on(2, (2.25, 0.0, 0.0))
        if p == 6: force_on(2, (20.0, 0.0, 0.0))
        if p == 8: force_on(2, (3.0, 0.0, 0.0))
        # 3: no odometry until period 3, no target until period 5
        if p == 5: goal_to(3, (4.0, 0.0, 0.0))
        # 4: goals below the floor: z = -0.11 is ignored (0), z = -0.1 is taken (1); a NaN z is taken too (9)
        if p == 0: goal_to(4, (4.0, 0.0, -0.11))
        if p == 1: goal_to(4, (4.0, 0.0, -0.1))
        if p == 9: goal_to(4, (4.0, 1.0, float("nan")))
        # 5: the search fails four times (periods 2 and 3); the fifth attempt gives up: GEN_NEW_TRAJ -> WAIT_TARGET
        if p in (2, 3): status[:, at(5)] = FO.NO_PATH
        # 6: the goal is blocked while executing (4): REPLAN_TRAJ, whose search fails -> GEN_NEW_TRAJ, whose search succeeds
        if p == 4: blocked[at(6)] = 1; status[0, at(6)] = FO.NO_PATH; status[1, at(6)] = FO.REACH_END_BUT_SHOT_FAILS
        # 7: the goal is blocked while aligning (1): the target is dropped
        if p == 1: blocked[at(7)] = 1
        # 8: the path collides while executing (3): REPLAN_TRAJ with t_cur exactly on a stage boundary; reaches the end (5); the OLD path
        #    collides (6): a WAIT_TARGET planner is dragged to REPLAN_TRAJ and searches without a target, as written
        if p == 3: first_hit[at(8)] = 5; t_cur[:, at(8)] = 0.1
        if p == 5: want[at(8)] = 0
        if p == 6: first_hit[at(8)] = 0
        # 9: the solver asks for a replan (-2 at 3) after a failed solve (exit_code 0: from the odometry); far odometry (-3 at 5)
        if p == 3: want[at(9)] = -2
        if p == 4: exit_code[at(9)] = 0
        if p == 5: want[at(9)] = -3
        # 10: reaches the end (3); a loud force while consider_force is still up and the target is gone (4): no replan
        if p == 3: want[at(10)] = 0
        if p == 4: force_on(10, (1.0, -2.0, 0.5))
        # 11: replans every other period from t_cur = (N - 1) Ts (4: the odometry), NaN (6), just inside the last stage (8), a quotient
        #     beyond int (10)
        if p in (3, 5, 7, 9): want[at(11)] = -2
        if p == 4: t_cur[:, at(11)] = (N - 1) * TS
        if p == 6: t_cur[:, at(11)] = float("nan")
        if p == 8: t_cur[:, at(11)] = (N - 1) * TS - 0.02
        if p == 10: t_cur[:, at(11)] = 1e300
        # 12: goal blocked AND path hit while executing (4); goal "blocked" without a target (8, after reaching the end at 6): nothing
        if p == 4: blocked[at(12)] = 1; first_hit[at(12)] = 10
        if p == 6: want[at(12)] = 0
        if p == 8: blocked[at(12)] = 1
        # 13: four failed searches (2, 3), then a force step (4) moves GEN_NEW_TRAJ to REPLAN_TRAJ: REPLAN_TRAJ gives up
        if p in (2, 3): status[:, at(13)] = FO.NO_PATH
        if p == 4: force_on(13, (0.0, 3.0, 0.0))
        # 14, 15: seeded draws
        for r in (14, 15):
            i = at(r)
            if p == 0:
                events.append(dict(kind="host", name="have_odom", idx=i, value=1))
            new = rng.random(len(i)) < (1.0 if p == 0 else 0.15)
            goal[i] = np.c_[rng.uniform(-5, 5, len(i)), rng.uniform(-5, 5, len(i)), rng.choice([0.0, 1.0, -0.2], len(i))]; gfresh[i] = new
            force[i] = rng.choice([0.1, 0.4, 0.6, 1.2, 3.0, 15.0], (len(i), 3)) * rng.choice([-1.0, 1.0], (len(i), 3)); ffresh[i] = rng.random(len(i)) < 0.6
            blocked[i] = rng.random(len(i)) < 0.1
            first_hit[i] = np.where(rng.random(len(i)) < 0.1, rng.integers(0, 40, len(i)), -1)
            status[:, i] = rng.choice([FO.REACH_HORIZON, FO.REACH_END, FO.NO_PATH, FO.NO_PATH, FO.REACH_END_BUT_SHOT_FAILS], (STEPS, len(i)))
            exit_code[i] = rng.choice([1, 1, 1, 0, -7], len(i))
            t_cur[:, i] = rng.uniform(-0.05, 1.1, (STEPS, len(i)))
            want[i] = rng.choice([1, 1, 1, 1, -1, 0, -2, -3], len(i))
            yaw[i] = rng.uniform(-3.0, 3.0, len(i))
        # ---- the period's events, the oracle in lock-step ----
        state = rng.normal(size=(B, 9)); state[:, 0:3] = (0.0, 0.0, 1.0); state[:, 8] = yaw
        for e in events:
            if e["kind"] == "host" and not e.get("done"):
                for b in e["idx"]:
                    setattr(fleet[b], e["name"], e["value"])
                e["done"] = True
        events.append(dict(kind="goal", goal=goal, fresh=gfresh))
        events.append(dict(kind="force", force=force, fresh=ffresh))
        events.append(dict(kind="safety", goal_blocked=blocked, first_hit=first_hit))
        for b, pl in enumerate(fleet):
            pl.goal(goal[b], gfresh[b]); pl.force(force[b], ffresh[b], BOUND); pl.safety(blocked[b], first_hit[b])
        for k in range(STEPS):
            now = 0.05 * p + 0.01 * k
            events.append(dict(kind="exec", state=state, pre_plan=pre_plan, exit_code=exit_code, t_cur=t_cur[k].copy(), now=now, astar_status=status[k].copy()))
            for b, pl in enumerate(fleet):
                pl.exec_end(pl.exec_begin(state[b], pre_plan[b], exit_code[b], t_cur[k][b], now, N, TS, MASS, G) is not None, status[k][b], now)
        result = np.array([want[b] if pl.exec_mpc else FO.RESULT_IDLE for b, pl in enumerate(fleet)], dtype=np.int32)
        events.append(dict(kind="mpc", result=result))
        for b, pl in enumerate(fleet):
            pl.mpc(result[b])
    for e in events:
        e.pop("done", None)
    return events


def run_oracle(events, B, N=N):
    """The oracle over the events.  Returns (fleet, after, met): after[i] = the fleet's arrays after event i (None for host events; for an
    exec event also `search` [B] and `start` [B] = exec_begin's dict or None), met[i][b] = the set of branches planner b met in event i."""
    fleet = [FO.Planner() for _ in range(B)]
    after, met = [], []
    for e in events:
        kind = e["kind"]
        extra = {}
        m = [set() for _ in range(B)]
        if kind == "host":
            for b in e["idx"]:
                setattr(fleet[b], e["name"], e["value"])
            after.append(None); met.append(m)
            continue
        for b, pl in enumerate(fleet):
            if kind == "goal":
                pl.goal(e["goal"][b], e["fresh"][b])
            elif kind == "force":
                pl.force(e["force"][b], e["fresh"][b], BOUND)
            elif kind == "safety":
                pl.safety(e["goal_blocked"][b], e["first_hit"][b])
            elif kind == "mpc":
                pl.mpc(e["result"][b])
            elif kind == "exec":
                was = pl.state
                start = pl.exec_begin(e["state"][b], e["pre_plan"][b], e["exit_code"][b], e["t_cur"][b], e["now"], N, TS, MASS, G)
                extra.setdefault("start", []).append(start)
                extra.setdefault("after_begin", []).append(pl.snapshot())
                m[b] |= pl.met
                pl.met = set()
                pl.exec_end(start is not None, e["astar_status"][b], e["now"])
                if start is not None:
                    m[b].add(("searched_from", was))
            m[b] |= pl.met
        a = arrays(fleet)
        if kind == "exec":
            a["search"] = np.array([s is not None for s in extra["start"]], dtype=np.int32)
            a["start"] = extra["start"]
            a["after_begin"] = arrays_of(extra["after_begin"])
        after.append(a); met.append(m)
    return fleet, after, met


def arrays_of(snaps):
    out = {k: np.array([s[k] for s in snaps], dtype=np.int32) for k in FO.INTS}
    out.update({k: np.array([s[k] for s in snaps], dtype=np.float64) for k in FO.VECS + FO.SCALARS})
    return out


def arrays(fleet):
    return arrays_of([p.snapshot() for p in fleet])
