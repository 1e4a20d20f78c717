"""The tick outcome (include/frp_nmpc_outcome.h) restated line by line in plain Python floats and ints: NMPCManage::mpcCallback's guard
and consequences (plan_manage/src/nmpc_manage.cpp:50-97) and the decisions of NMPCSolver::solveNMPC (plan_manage/src/nmpc_solver.cpp:
351-482).  The reference holds no test vectors for this rule, so this file is a restatement, not a recording: the hand-worked table of
tests/test_outcome_cpu.py is what pins it.  Line numbers are nmpc_solver.cpp's unless nmpc_manage.cpp is named."""
import math

import numpy as np

INIT_POSITION, ROTATE_YAW, PUB_END, PUB_TRAJ, WAIT = range(5)   # enum CMD_STATUS (nmpc_utils.h:115-122)
RUN, IDLE, AT_END, ENDING = range(4)                            # FRP_TICK_*
RESULT_IDLE = -4                                                # FRP_TICK_RESULT_IDLE
MODEL_NORMAL, MODEL_FINAL = 0, 1

STATE = ("fail_count", "replan_count", "kino_replan", "exit_code", "initialized", "cmd_status", "pub_end", "exec_mpc")
OUT = ("gate", "keep", "accept", "result", "replan")


def norm3(a, b):
    """(a - b).norm() of Eigen for three doubles: sqrt((d0 * d0 + d1 * d1) + d2 * d2), one rounding per operation."""
    d0, d1, d2 = float(a[0]) - float(b[0]), float(a[1]) - float(b[1]), float(a[2]) - float(b[2])
    return math.sqrt((d0 * d0 + d1 * d1) + d2 * d2)


class Planner:
    """One NMPCSolver with the exec_mpc_ of its NMPCManage, as the constructors leave them."""

    def __init__(self, **kw):
        self.fail_count = 0
        self.replan_count = 0
        self.kino_replan = 0
        self.exit_code = 0
        self.initialized = 0
        self.cmd_status = INIT_POSITION
        self.pub_end = 0
        self.cmd_end_pt = [0.0, 0.0, 0.0]
        self.exec_mpc = 1
        self.mode = MODEL_NORMAL
        self.gate = self.keep = self.accept = self.result = self.replan = None
        self.seen = None     # what the last RUN tick_end met (for the tests' counting; not state)
        self.branch = None   # which arm of :398-421 the last tick_end took: "success", "maxit_accepted", "replan_raised", "failure"; None when gated
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)

    def tick_begin(self, reset_output=0):
        """Returns the reset_output the call leaves (always 0)."""
        if reset_output != 0:                       # :981, the command timer's PUB_END
            self.initialized = 0
        if not self.exec_mpc:                       # nmpc_manage.cpp:52
            self.gate = IDLE
        elif self.cmd_status == WAIT:               # :355
            self.gate = AT_END
        elif self.pub_end:                          # :356
            self.gate = ENDING
        else:
            self.gate = RUN
        if self.gate == RUN:
            self.keep = int(bool(self.initialized) and self.exit_code == 1)   # :363: initMPCOutput unless both hold
            self.initialized = 1                                               # :283
        else:
            self.keep = 1
        return 0

    def tick_end(self, z, exitflag, mpc_output, state, end_pt, kino_path, kino_size, time_offset, ref_replan, Ts=0.05, N=None):
        """z [N][17], mpc_output [N+1][17] (the plan before the update), state [9], end_pt [3], kino_path [K][3]."""
        N = len(z) if N is None else N
        self.branch = None
        self.seen = None
        if self.gate != RUN:
            self.result = {AT_END: 0, ENDING: -1, IDLE: RESULT_IDLE}[self.gate]
            self.accept = 0
            self.replan = 0
            if self.gate == AT_END:                 # nmpc_manage.cpp:66-73
                self.exec_mpc = 0
            return self.result
        self.exit_code = int(exitflag)              # :387 / :394
        if ref_replan:                              # getCurTraj, :136-140
            self.kino_replan = 1
        update_result = False
        if self.exit_code == 1:                     # :398
            self.fail_count = 0
            self.replan_count = 0
            update_result = True
            self.branch = "success"
        else:
            self.fail_count += 1                    # :407
            self.branch = "failure"
            if self.replan_count > 3 and self.exit_code == 0:   # :408
                self.fail_count = 0
                self.replan_count = 0
                update_result = True
                self.branch = "maxit_accepted"
            elif self.fail_count > 2:               # :414
                self.fail_count = 0
                self.replan_count += 1
                self.kino_replan = 1
                self.branch = "replan_raised"
        self.accept = int(update_result)
        rows = z if update_result else mpc_output   # :423-429: the plan as the update leaves it (positions are not touched by the yaw wrap)
        ref_end = [float(v) for v in rows[N - 1][8:11]]          # :435 (.at(19) for N = 20)
        row1 = [float(v) for v in rows[1][8:11]]
        max_index = int((N * Ts + float(time_offset)) / Ts)     # :436
        kino_size = int(kino_size)
        last = min(max(kino_size, 1), len(kino_path)) - 1       # (the library's clamp; inside [1, K] it is kino_size - 1)
        pending = self.kino_replan                  # (raised before this call, by the references or by :414-420)
        if max_index > 0.5 * kino_size and norm3(end_pt, kino_path[last]) > 0.7:   # :439
            self.kino_replan = 1
        if max_index >= kino_size or norm3(ref_end, end_pt) < 1.0:                 # :446
            self.mode = MODEL_FINAL
        # what the tests count (not state): the two distances, the flag as the return module meets it, and how it was raised
        self.seen = dict(d_odom=norm3(row1, state[0:3]), d_goal=norm3(ref_end, end_pt), pending=int(self.kino_replan), max_index=max_index,
                         local_end=bool(self.kino_replan and not pending), raised_now=bool(ref_replan) or self.branch == "replan_raised" or bool(self.kino_replan and not pending))
        if norm3(row1, state[0:3]) > 2.0:           # :452
            self.cmd_status = WAIT
            self.result = -3
        elif norm3(ref_end, end_pt) < 0.15:         # :466
            self.pub_end = 1
            self.cmd_end_pt = [float(v) for v in end_pt]
            self.result = -1
        elif self.kino_replan:                      # :475
            self.kino_replan = 0
            self.result = -2
        else:
            self.result = 1
        self.replan = int(self.result == -2)
        if self.result in (-2, -3):                 # nmpc_manage.cpp:78-93 (0 is the gate's)
            self.exec_mpc = 0
        return self.result


class Fleet:
    """B planners with the array view the device tests compare against."""

    def __init__(self, B):
        self.p = [Planner() for _ in range(B)]

    def arrays(self):
        out = {k: np.array([getattr(p, k) if getattr(p, k) is not None else 0 for p in self.p], dtype=np.int32) for k in STATE + OUT + ("mode",)}
        out["cmd_end_pt"] = np.array([p.cmd_end_pt for p in self.p], dtype=np.float64)
        return out

    def tick_begin(self, reset_output=None):
        for b, p in enumerate(self.p):
            p.tick_begin(0 if reset_output is None else int(reset_output[b]))
        return np.zeros(len(self.p), dtype=np.int32)

    def tick_end(self, z, exitflag, mpc_output, state, end_pt, kino_path, kino_size, time_offset, ref_replan, Ts=0.05):
        end_pt, kino_path, kino_size = np.asarray(end_pt), np.asarray(kino_path), np.asarray(kino_size).reshape(-1)
        for b, p in enumerate(self.p):
            p.tick_end(z[b], exitflag[b], mpc_output[b], state[b], end_pt[b] if end_pt.ndim == 2 else end_pt,
                       kino_path[b] if kino_path.ndim == 3 else kino_path, kino_size[b] if kino_size.size > 1 else kino_size[0],
                       time_offset[b], ref_replan[b], Ts)
        return self.arrays()
