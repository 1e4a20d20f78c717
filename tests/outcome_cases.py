"""Deterministic inputs for the tick outcome (include/frp_nmpc_outcome.h): a fleet of B planners and a scripted sequence of ticks,
written straight into the arrays frp_nmpc_tick_begin / frp_nmpc_tick_end read -- no solve is needed.  The planner's role is b % 16;
roles 0-13 each walk one path through the rule (the comments name it), roles 14 and 15 draw their inputs from a seeded generator.
Between ticks the script plays the parts that are not on the device: the FSM that re-enables a planner (exec_mpc, cmd_status,
pub_end) and the command timer that raises reset_output.

Geometry (every number a short binary fraction, so the thresholds can be met exactly): the path is p_k = (0.25 k, 0, 1); by default
the goal is its last sample, the odometry is (0, 0, 1), z's row i sits at (0.125 i, 0, 1) and the plan's at (0.125 i, 0.25, 1)."""
import numpy as np

from . import outcome_oracle as OO

B, N, K, TICKS, TS = 256, 20, 64, 8, 0.05
ROLES = 16


def sequence(B=B, N=N, K=K, ticks=TICKS, per_planner=True, seed=0):
    """Returns (static, initial, steps).
    static: end_pt, kino_path, kino_size -- [B,3], [B,K,3], [B] when per_planner, else planner 0's [3], [K,3], [1].
    initial: the state arrays before tick 0 (OO.STATE + cmd_end_pt + mode).
    steps[t]: z [B,N,17], exitflag [B], mpc_output [B,N+1,17], state [B,9], time_offset [B], ref_replan [B], reset_output [B] and
    host: a list of (name, indices, value) written into the state arrays before tick_begin."""
    rng = np.random.default_rng(seed)
    role = np.arange(B) % ROLES
    at = lambda r: np.nonzero(role == r)[0]
    path = np.zeros((B, K, 3)); path[:, :, 0] = 0.25 * np.arange(K)[None, :]; path[:, :, 2] = 1.0
    kino_size = np.full(B, K, dtype=np.int32)
    end_pt = path[:, K - 1].copy()
    far_end = 0.125 * (N - 1)                      # x of z's default last row
    end_pt[at(5)] = (5.125, 0.0, 1.0)              # role 5: the goal 0.125 beyond the last row it plans at tick 2
    end_pt[at(6)] = (far_end + 0.125, 0.0, 1.0)    # role 6: the goal 0.125 beyond the DEFAULT last row
    end_pt[at(7)] = (6.0, 0.0, 1.0)                # role 7: exactly 1.0 from the last row (5, 0, 1) it plans
    kino_size[at(9)] = min(30, K)                  # role 9: the horizon reaches past half of a short path that ends far from the goal
    end_pt[at(11)] = (far_end + 0.5, 0.0, 1.0)     # role 11: within 1.0 of the goal, not within 0.15
    initial = {k: np.zeros(B, dtype=np.int32) for k in OO.STATE + ("mode",)}
    initial["cmd_status"][:] = OO.INIT_POSITION
    initial["exec_mpc"][:] = 1
    initial["cmd_end_pt"] = np.zeros((B, 3))
    initial["replan_count"][at(3)] = 4             # role 3: repeated replans behind it
    initial["exec_mpc"][at(8)] = 0                 # role 8: not executing yet
    steps = []
    for t in range(ticks):
        z = rng.normal(size=(B, N, 17)); mo = rng.normal(size=(B, N + 1, 17))
        z[:, :, 8] = 0.125 * np.arange(N)[None, :]; z[:, :, 9] = 0.0; z[:, :, 10] = 1.0
        mo[:, :, 8] = 0.125 * np.arange(N + 1)[None, :]; mo[:, :, 9] = 0.25; mo[:, :, 10] = 1.0
        state = rng.normal(size=(B, 9)); state[:, 0:3] = (0.0, 0.0, 1.0)
        exitflag = np.ones(B, dtype=np.int32)
        toff = np.zeros(B); ref_replan = np.zeros(B, dtype=np.int32); reset = np.zeros(B, dtype=np.int32)
        host = []
        # 1: a plain failure, then successes
        if t == 0:
            exitflag[at(1)] = -7
        # 2: three failures raise a replan (-2, exec_mpc <- 0); the FSM re-enables it at tick 4, three more failures
        if t in (0, 1, 2, 4, 5, 6):
            exitflag[at(2)] = -6
        if t == 4:
            host.append(("exec_mpc", at(2), 1))
        # 3: MAXIT after replan_count > 3 is accepted at tick 0; at tick 1 MAXIT is a plain failure again; half of them get another exit instead
        if t in (0, 1):
            exitflag[at(3)] = 0
            if t == 0:
                exitflag[at(3)[1::2]] = -7
        # 4: tick 1: odometry 2.5 away with a replan pending -> -3, WAIT, kino_replan kept; tick 3: re-enabled but still WAIT -> 0;
        #    tick 5: the FSM starts a trajectory again -> the kept flag fires as -2
        if t == 1:
            state[at(4), 0] = -2.375; ref_replan[at(4)] = 1
        if t == 3:
            host.append(("exec_mpc", at(4), 1))
        if t == 5:
            host.append(("exec_mpc", at(4), 1)); host.append(("cmd_status", at(4), OO.PUB_TRAJ))
        # 5: tick 2 reaches the goal with a replan pending -> -1 (over -2), pub_end; ENDING until the timer's PUB_END raises reset_output
        #    and the FSM clears pub_end at tick 5: a cold start
        if t == 2:
            z[at(5), N - 1, 8] = 5.0; ref_replan[at(5)] = 1
        if t == 5:
            reset[at(5)] = 1; host.append(("pub_end", at(5), 0))
        # 6: tick 0: far odometry AND at the goal AND a replan pending -> -3; tick 2: re-enabled -> -1 with the flag still pending;
        #    tick 4: pub_end cleared, the plan ends elsewhere -> -2
        if t == 0:
            state[at(6), 0] = -3.0; ref_replan[at(6)] = 1
        if t == 2:
            host.append(("exec_mpc", at(6), 1)); host.append(("cmd_status", at(6), OO.PUB_TRAJ))
        if t >= 4:
            z[at(6), N - 1, 8] = 3.0; mo[at(6), N - 1, 8] = 3.0
        if t == 4:
            host.append(("pub_end", at(6), 0))
        # 7: the thresholds met exactly: row 1 is (2, 0, 0) from the odometry -- not > 2.0 -- and the last row (1, 0, 0) from the goal --
        #    not < 1.0: result 1, mode stays (for N > 2: with N = 2 the two rows are one)
        z[at(7), 1, 8] = 2.0
        z[at(7), N - 1, 8] = 5.0
        # 8: idle until the FSM enables it at tick 4
        if t == 4:
            host.append(("exec_mpc", at(8), 1))
        # 9: the local end (:439) raises the replan at tick 0
        # 10: the time offset grows until the horizon runs past the path: the mode switches
        toff[at(10)] = 0.625 * t
        # 11: within 1.0 of the goal: the mode switches at tick 0 (a constant input)
        # 12: the timer raises reset_output on a healthy planner at tick 3: cold start, nothing else
        if t == 3:
            reset[at(12)] = 1
        # 13: a rejected solve decides on the PLAN's rows: z's row 1 is far from the odometry, the plan's is not (even ticks); an accepted one
        #     on z's: the plan's row 1 is far, z's is not (odd ticks)
        if t % 2 == 0:
            exitflag[at(13)] = -7; z[at(13), 1, 8] = 50.0
        else:
            mo[at(13), 1, 8] = 50.0
        # 14, 15: seeded draws
        for r in (14, 15):
            i = at(r)
            exitflag[i] = rng.choice([1, 1, 1, 0, -7, -6, 2], size=len(i))
            ref_replan[i] = rng.random(len(i)) < 0.15
            state[i, 0:3] += rng.normal(0, 0.9, (len(i), 3))
            toff[i] = rng.uniform(0, 3.0, len(i))
            reset[i] = rng.random(len(i)) < 0.1
            if t % 3 == 2:
                host.append(("exec_mpc", i, 1)); host.append(("cmd_status", i[::2], OO.PUB_TRAJ)); host.append(("pub_end", i[::3], 0))
        steps.append(dict(z=z, exitflag=exitflag, mpc_output=mo, state=state, time_offset=toff, ref_replan=ref_replan, reset_output=reset, host=host))
    static = dict(end_pt=end_pt, kino_path=path, kino_size=kino_size)
    if not per_planner:
        static = dict(end_pt=end_pt[0].copy(), kino_path=path[0].copy(), kino_size=kino_size[:1].copy())
    return static, initial, steps


def run_oracle(static, initial, steps, Ts=TS):
    """The oracle over the sequence.  Returns (per-tick arrays after tick_end -- OO.Fleet.arrays() plus `reset_output` as tick_begin left it --,
    per-tick list of what each planner met: (gate, branch, seen, result))."""
    Bn = len(initial["exec_mpc"])
    f = OO.Fleet(Bn)
    for b, p in enumerate(f.p):
        for k in OO.STATE + ("mode",):
            setattr(p, k, int(initial[k][b]))
        p.cmd_end_pt = [float(v) for v in initial["cmd_end_pt"][b]]
    after, met = [], []
    for s in steps:
        for name, idx, value in s["host"]:
            for b in idx:
                setattr(f.p[b], name, int(value))
        left = f.tick_begin(s["reset_output"])
        a = f.tick_end(s["z"], s["exitflag"], s["mpc_output"], s["state"], static["end_pt"], static["kino_path"], static["kino_size"],
                       s["time_offset"], s["ref_replan"], Ts)
        a["reset_output"] = left
        after.append(a)
        met.append([(p.gate, p.branch, p.seen, p.result) for p in f.p])
    return after, met
