"""NMPCManage (plan_manage/src/nmpc_manage.cpp of the reference, "NM") restated line by line in plain Python ints and floats: one Planner
object per planner, one method per callback.  The executable statement of what include/frp_nmpc_fsm.h's six calls do.

This layer is STRUCTURALLY UNPINNED: the reference holds no test vectors for its state machine, so this file is a restatement, pinned by
the hand-worked scenarios of tests/test_fsm_cpu.py.  What is not restated: the clocks (`now`, `t_cur` are arguments), the odometry callbacks
(`have_odom` and `state` are the caller's), prints and displays, the two sleeps of mpcCallback, the four-thread spinner (callbacks happen
in the order of the calls).  The A* is an input: exec_end takes its status.  The reference leaves end_pt_, external_acc_,
last_external_acc_ and init_yaw_ uninitialised; they start at 0 here."""
import math

INIT, WAIT_TARGET, INIT_YAW, GEN_NEW_TRAJ, REPLAN_TRAJ, EXEC_TRAJ = range(6)   # enum FSM_EXEC_STATE
CMD_INIT_POSITION, CMD_ROTATE_YAW, CMD_PUB_END, CMD_PUB_TRAJ, CMD_WAIT = range(5)  # enum CMD_STATUS (nmpc_utils.h:115-122)
REACH_HORIZON, REACH_END, NO_PATH, REACH_END_BUT_SHOT_FAILS = 1, 2, 3, 4       # KinodynamicAstar::search
MODEL_NORMAL, MODEL_FINAL = 0, 1
RESULT_IDLE = -4

INTS = ("state", "have_odom", "have_target", "have_traj", "trigger", "call_init_yaw", "consider_force", "replan_force_surpass", "surpass_count",
        "plan_fail_count", "exec_mpc", "cmd_status", "pub_end", "mode")
VECS = ("end_pt", "external_acc", "last_external_acc", "yaw_odom")
SCALARS = ("init_yaw", "change_yaw_time", "kino_start_time")


def smax(a, b):
    """std::max(a, b)"""
    return b if a < b else a


def max_abs3(x, y, z):
    """max(max(abs(x), abs(y)), abs(z)) (NM:371, :383)"""
    return smax(smax(abs(x), abs(y)), abs(z))


def qmul(a, b):
    """Eigen's quaternion product, scalar form; (w, x, y, z)"""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz,
            aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx)


def thrust_world(roll, pitch, yaw, thrust):
    """eulerToRot(euler) * (0, 0, thrust) (nmpc_solver.cpp:554-564): Quaternion(cos(a / 2), ..sin(a / 2)..) per axis, q = qz * qy * qx,
    the third column of Quaternion::toRotationMatrix times the thrust"""
    qx = (math.cos(roll / 2), math.sin(roll / 2), 0.0, 0.0)
    qy = (math.cos(pitch / 2), 0.0, math.sin(pitch / 2), 0.0)
    qz = (math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2))
    w, x, y, z = qmul(qmul(qz, qy), qx)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, txx, txz, tyy, tyz = tx * w, ty * w, tx * x, tz * x, ty * y, tz * y
    return [(txz + twy) * thrust, (tyz - twx) * thrust, (1.0 - (txx + tyy)) * thrust]


def in_plan(t, Ts, N):
    """cur_index < planning_horizon_ - 1 && t_cur >= 0.0 (nmpc_solver.cpp:164-167), on the doubles: for t >= 0 the truncation is a floor and
    floor(q) < N - 1 <=> q < N - 1; a NaN fails (the reference's cast of it is undefined)"""
    return t >= 0.0 and t / Ts < float(N - 1)


def start_state(replan, exit_code, t_cur, pre_plan, state, N, Ts, mass, g):
    """getKinoPath's head (nmpc_solver.cpp:151-186).  Returns (start_pt, start_vel, start_acc, source), source 'plan' or 'odom'."""
    pt, vel, acc = [float(v) for v in state[0:3]], [float(v) for v in state[3:6]], [0.0, 0.0, 0.0]   # :151-153
    if replan and exit_code == 1 and in_plan(t_cur, Ts, N):                                           # :160, :167
        i = int(t_cur / Ts)                                                                            # :164
        w = math.fmod(t_cur, Ts) / Ts
        q = [float(pre_plan[i][j]) + w * (float(pre_plan[i + 1][j]) - float(pre_plan[i][j])) for j in range(17)]   # :169
        tw = thrust_world(q[14], q[15], q[16], q[3])                                                   # :176-178
        return [q[8], q[9], q[10]], [q[11], q[12], q[13]], [tw[0] / mass, tw[1] / mass, tw[2] / mass - g], "plan"   # :173-180
    return pt, vel, acc, "odom"


class Planner:
    def __init__(self, **kw):
        # NMPCManage's constructor and init (NM:9): INIT, every flag false, every counter 0
        self.state = INIT
        self.have_odom = self.have_target = self.have_traj = self.trigger = self.call_init_yaw = 0
        self.consider_force = self.replan_force_surpass = self.surpass_count = self.plan_fail_count = 0
        self.exec_mpc = 0
        self.end_pt, self.external_acc, self.last_external_acc = [0.0] * 3, [0.0] * 3, [0.0] * 3
        self.init_yaw = 0.0
        # the NMPCSolver members the FSM writes
        self.cmd_status, self.pub_end, self.mode = CMD_INIT_POSITION, 0, MODEL_NORMAL
        self.yaw_odom = [0.0] * 9
        self.change_yaw_time = self.kino_start_time = 0.0
        # what the last callback met (for the coverage test): a set of branch names
        self.met = set()
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, list(v) if isinstance(v, (list, tuple)) else v)

    def _go(self, new, who):
        self.met.add(("edge", who, self.state, new))
        self.state = new                                                   # changeFSMExecState, NM:102-107

    # ---- NM:481-493 ----
    def goal(self, goal, fresh=1):
        self.met = set()
        if not fresh:
            return
        if goal[2] < -0.1:                                                 # NM:484
            self.met.add("goal:ignored")
            return
        self.trigger = 1                                                   # NM:486
        self.have_target = 1                                               # NM:487
        self.end_pt = [float(goal[0]), float(goal[1]), 1.2]                # NM:489
        self.met.add("goal:taken")

    # ---- NM:366-418 ----
    def force(self, force, fresh=1, bound=0.5):
        self.met = set()
        if not fresh:
            return
        if not self.consider_force:                                        # NM:369
            self.met.add("force:not_considered")
            return
        fx, fy, fz = float(force[0]), float(force[1]), float(force[2])
        diverse = max_abs3(fx, fy, fz)                                     # NM:371
        if diverse <= bound:                                               # NM:372
            self.external_acc = [0.0, 0.0, 0.0]                            # NM:374
            self.last_external_acc = [fx, fy, fz]                          # NM:375
            self.surpass_count = 0                                         # NM:376
            self.met.add("force:quiet")
            return
        self.external_acc = [fx, fy, fz]                                   # NM:380
        diff = [self.last_external_acc[i] - self.external_acc[i] for i in range(3)]   # NM:382
        surpass = max_abs3(diff[0], diff[1], diff[2])                      # NM:383
        if surpass > bound:                                                # NM:385
            self.surpass_count += 1                                        # NM:391
            if self.surpass_count >= 1:                                    # NM:393
                self.replan_force_surpass = 1                              # NM:396
                self.last_external_acc = [fx, fy, fz]                      # NM:397
                self.met.add("force:loud_changed")
                if self.have_target:                                       # NM:399
                    self._go(REPLAN_TRAJ, "force")                         # NM:401
                    self.met.add("force:replan")
                if surpass > 10.0:                                         # NM:404
                    self.have_target = 0                                   # NM:407
                    self._go(WAIT_TARGET, "force")                         # NM:408
                    self.met.add("force:fierce")
        else:
            self.surpass_count = 0                                         # NM:414
            self.met.add("force:loud_steady")

    # ---- NM:60-97 ----
    def mpc(self, result):
        self.met = set()
        if result == 0:                                                    # NM:67-75
            self.exec_mpc = 0
            self.have_target = 0
            self._go(WAIT_TARGET, "mpc")
        elif result == -2:                                                 # NM:82-88
            self.exec_mpc = 0
            self._go(REPLAN_TRAJ, "mpc")
        elif result == -3:                                                 # NM:89-95
            self.exec_mpc = 0
            self._go(WAIT_TARGET, "mpc")
        self.met.add(("mpc", result))

    # ---- NM:318-325, :333-338 ----
    def safety(self, goal_blocked, first_hit):
        self.met = set()
        if self.have_target and goal_blocked:                              # NM:289-291
            if self.state == EXEC_TRAJ:                                    # NM:318
                self._go(REPLAN_TRAJ, "safety_goal")                       # NM:320
            else:
                self.have_target = 0                                       # NM:322
                self._go(WAIT_TARGET, "safety_goal")                       # NM:324
        if self.have_traj and first_hit >= 0:                              # NM:329-333
            self._go(REPLAN_TRAJ, "safety_path")                           # NM:336

    # ---- NM:127-259 up to getKinoPath, nmpc_solver.cpp:148-186 ----
    def exec_begin(self, state, pre_plan, exit_code, t_cur, now, N=20, Ts=0.05, mass=0.74, g=9.81):
        """Returns None, or the search's start: dict(start_pt, start_vel, start_acc, retry_pt, retry_vel, source)."""
        self.met = set()
        st = self.state
        if st == INIT:                                                     # NM:129-140
            if not self.have_odom:
                self.met.add("init:no_odom")
                return None
            if self.have_target:
                self._go(WAIT_TARGET, "exec")
            else:
                self.met.add("init:no_target")
        elif st == WAIT_TARGET:                                            # NM:142-155
            if not self.have_target:
                self.consider_force = 0                                    # NM:146
                self.met.add("wait:no_target")
            else:
                self._go(INIT_YAW, "exec")                                 # NM:151
                self.call_init_yaw = 1                                     # NM:152
        elif st == INIT_YAW:                                               # NM:157-180
            if self.call_init_yaw:
                d0, d1 = self.end_pt[0] - float(state[0]), self.end_pt[1] - float(state[1])   # NM:161
                self.init_yaw = math.atan2(d1, d0)                         # NM:162
                if abs(float(state[8]) - self.init_yaw) >= 0.8:            # NM:164
                    self.yaw_odom = [float(v) for v in state]              # callInitYaw, nmpc_solver.cpp:232
                    self.pub_end = 0                                       # :234
                    self.change_yaw_time = float(now)                      # :235
                    self.cmd_status = CMD_ROTATE_YAW                       # :261
                    self.met.add("yaw:rotate")
                else:
                    self.met.add("yaw:aligned")
                self.call_init_yaw = 0                                     # NM:168
            elif abs(float(state[8]) - self.init_yaw) < 0.8:               # NM:172
                self.consider_force = 1                                    # NM:174
                self._go(GEN_NEW_TRAJ, "exec")                             # NM:176
            else:
                self.met.add("yaw:turning")
        elif st in (GEN_NEW_TRAJ, REPLAN_TRAJ):                            # NM:182-245
            self.exec_mpc = 0                                              # NM:184, :218
            if self.plan_fail_count > 3:                                   # NM:187, :220
                self.have_target = 0
                self._go(WAIT_TARGET, "exec")
                self.plan_fail_count = 0
                self.met.add("plan:give_up")
                return None
            pt, vel, acc, source = start_state(st == REPLAN_TRAJ, exit_code, t_cur, pre_plan, state, N, Ts, mass, g)
            self.met.add("start:" + source)
            return dict(start_pt=pt, start_vel=vel, start_acc=acc, retry_pt=[float(v) for v in state[0:3]], retry_vel=[float(v) for v in state[3:6]],
                        source=source)
        elif st == EXEC_TRAJ:                                              # NM:247-257
            if self.trigger and self.exec_mpc:
                self._go(REPLAN_TRAJ, "exec")
            else:
                self.met.add("exec:steady")
        return None

    # ---- NM:194-210, :227-242, nmpc_solver.cpp:215-225 ----
    def exec_end(self, search, astar_status, now):
        if not search:
            return
        if astar_status != NO_PATH:
            self.mode = MODEL_NORMAL                                       # nmpc_solver.cpp:218
            self.kino_start_time = float(now)                              # :219
            self.cmd_status = CMD_PUB_TRAJ                                 # :222
            self.pub_end = 0                                               # :223
            self.have_traj = 1                                             # NM:197
            self.trigger = 0                                               # NM:198
            self.exec_mpc = 1                                              # NM:199
            self.replan_force_surpass = 0                                  # NM:200
            self.plan_fail_count = 0                                       # NM:203
            self._go(EXEC_TRAJ, "exec_end")                                # NM:204
        else:
            self.plan_fail_count += 1                                      # NM:208
            self._go(GEN_NEW_TRAJ, "exec_end")                             # NM:209

    def snapshot(self):
        out = {k: getattr(self, k) for k in INTS + SCALARS}
        out.update({k: list(getattr(self, k)) for k in VECS})
        return out
