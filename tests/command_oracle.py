"""Executable statement of the command timer (include/frp_nmpc_command.h): NMPCSolver::cmdTrajCallback
(plan_manage/src/nmpc_solver.cpp:865-987) with callInitYaw's rate (:237-257), eulerToRot (:554-564) and the snapshot
pre_mpc_output_ = mpc_output_ (:527-528), restated statement by statement on Python floats (IEEE doubles, one rounding per
operation, math.fmod exact).  Eigen's expressions are written out term by term: Quaternion(AngleAxis) (Geometry/Quaternion.h:
ha = 0.5 * angle; w = cos(ha); vec = sin(ha) * axis), the scalar quaternion product, Quaternion::toRotationMatrix, Matrix3d * Vector3d.

What the restatement adds to the reference, as the header states it:
  * (int)(t_cur / Ts_) is undefined for a NaN and for a quotient beyond int: such a t_cur takes the else branch (:948-952);
  * without odom / init_yaw / t_yaw a planner in ROTATE_YAW publishes nothing and is flagged: kind NO_YAW_INPUT;
  * a callback that publishes nothing writes 16 zeros; mav_msgs' message helper (:889) is not restated: a ROTATE_YAW sample is the
    position, the quaternion of a rotation about z by desired_yaw, and desired_yaw in slot 12.
Slots of a sample: position 0-2, quaternion x y z w 3-6, linear velocity 7-9, body rates 10-12, linear acceleration 13-15."""
import math

import numpy as np

INIT_POSITION, ROTATE_YAW, PUB_END, PUB_TRAJ, WAIT = range(5)   # enum CMD_STATUS, nmpc_utils.h:115-122
NONE, TRAJ, END, YAW, NO_YAW_INPUT = 0, 1, 2, 3, -1              # FRP_COMMAND_*
PI = 3.1415926                                                   # nmpc_solver.cpp:3
STRIDE = 16
DEFAULTS = dict(Ts=0.05, mass=0.74, g=9.81)


def axis_quat(angle, k):
    """Quaternion(AngleAxisd(angle, unit axis k)) as (w, x, y, z)."""
    ha = 0.5 * angle
    s = math.sin(ha)
    v = [0.0, 0.0, 0.0]
    v[k] = s
    return (math.cos(ha), v[0], v[1], v[2])


def qmul(a, b):
    """a * b, Eigen's scalar quat_product; (w, x, y, z)."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz,
            aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx)


def attitude(roll, pitch, yaw):
    """AngleAxisd(roll, X) * AngleAxisd(pitch, Y) * AngleAxisd(yaw, Z) (:933, :971) as the message stores it: (x, y, z, w)."""
    w, x, y, z = qmul(qmul(axis_quat(roll, 0), axis_quat(pitch, 1)), axis_quat(yaw, 2))
    return (x, y, z, w)


def to_rotation_matrix(q):
    """Quaternion::toRotationMatrix, (w, x, y, z) -> 3 x 3 list."""
    w, x, y, z = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def euler_to_rot(euler):
    """NMPCSolver::eulerToRot (:554-564): Matrix3d(qz * qy * qx)."""
    qx, qy, qz = axis_quat(euler[0], 0), axis_quat(euler[1], 1), axis_quat(euler[2], 2)
    return to_rotation_matrix(qmul(qmul(qz, qy), qx))


def init_yaw_dot(init_yaw, odom_yaw):
    """callInitYaw (:237-257)."""
    d = init_yaw - odom_yaw
    if d > PI:
        d = 2 * PI - d                 # :241, as written (not d - 2 PI)
    elif d < -PI:
        d = d + 2 * PI                 # :245
    max_yaw_dot = 0.4 * PI             # :248
    if d > max_yaw_dot:
        d = max_yaw_dot
    elif d < -max_yaw_dot:
        d = -max_yaw_dot
    return d


def std_min(a, b):
    return b if b < a else a


def std_max(a, b):
    return b if a < b else a


def cast_is_defined(q):
    """(int)q of a double is defined when the truncated value fits an int."""
    return not math.isnan(q) and -2147483649.0 < q < 2147483648.0


def interpolate(pre_plan, cur_index, t_cur, Ts):
    """mpcq (:911): pre.at(i) + fmod(t_cur, Ts_) / Ts_ * (pre.at(i + 1) - pre.at(i)), element by element."""
    w = math.fmod(t_cur, Ts) / Ts
    a, b = pre_plan[cur_index], pre_plan[cur_index + 1]
    return [float(a[j]) + w * (float(b[j]) - float(a[j])) for j in range(17)]


def trajectory_point(mpcq, mass, g):
    """:913-938 from mpcq."""
    o = [0.0] * STRIDE
    o[0:3] = mpcq[8:11]
    o[7:10] = mpcq[11:14]
    o[10:13] = mpcq[0:3]
    R = euler_to_rot(mpcq[14:17])                                           # :925, :927
    thrust_b = (0.0, 0.0, mpcq[3])                                          # :926
    thrust_w = [R[i][0] * thrust_b[0] + R[i][1] * thrust_b[1] + R[i][2] * thrust_b[2] for i in range(3)]
    o[13] = thrust_w[0] / mass
    o[14] = thrust_w[1] / mass
    o[15] = thrust_w[2] / mass - g                                          # :929-931
    o[3:7] = attitude(mpcq[14], mpcq[15], mpcq[16])                         # :933-938
    return o


class Planner:
    """The members cmdTrajCallback reads and writes."""

    def __init__(self, pre_plan, have_traj, status, pub_end, end_pt, odom=None, init_yaw=None, finish=None, Ts=0.05, mass=0.74, g=9.81):
        self.pre_plan = np.asarray(pre_plan, dtype=np.float64)
        self.N = self.pre_plan.shape[0]                                     # planning_horizon_
        self.have_traj, self.status, self.pub_end = bool(have_traj), int(status), bool(pub_end)
        self.end_pt = [float(v) for v in end_pt]
        self.odom = None if odom is None else [float(v) for v in odom]
        self.init_yaw = None if init_yaw is None else float(init_yaw)
        self.finish = finish            # finish_mpc_cmd_; None: not touched yet
        self.reset_output = False       # initialized_output_ = false happened
        self.Ts, self.mass, self.g = float(Ts), float(mass), float(g)

    def callback(self, t_cur, t_yaw=None):
        """One cmdTrajCallback; returns (kind, 16 doubles)."""
        zero = [0.0] * STRIDE
        st = self.status
        if st == ROTATE_YAW:                                                # :883-893
            if self.odom is None:
                return NO_YAW_INPUT, zero
            dot = init_yaw_dot(self.init_yaw, self.odom[8])
            yaw_temp = self.odom[8] + float(t_yaw) * dot                    # :885
            desired_yaw = std_min(yaw_temp, self.init_yaw) if self.init_yaw - self.odom[8] >= 0 else std_max(yaw_temp, self.init_yaw)  # :886
            o = list(zero)
            o[0:3] = self.odom[0:3]                                         # :888
            o[5] = math.sin(0.5 * desired_yaw)
            o[6] = math.cos(0.5 * desired_yaw)
            o[12] = desired_yaw
            return YAW, o
        if st == PUB_TRAJ:                                                  # :900-954
            if not self.have_traj:
                return NONE, zero                                           # :903
            t_cur = float(t_cur)
            q = t_cur / self.Ts
            if cast_is_defined(q):
                cur_index = int(q)                                          # :907 (truncation)
                publish = cur_index < self.N - 1 and t_cur >= 0.0           # :909
            else:
                publish = False
            if publish:
                o = trajectory_point(interpolate(self.pre_plan, cur_index, t_cur, self.Ts), self.mass, self.g)
                self.finish = 0                                             # :946
                return TRAJ, o
            self.finish = 1                                                 # :950
            if self.pub_end:
                self.status = PUB_END                                       # :951
            return NONE, zero
        if st == PUB_END:                                                   # :956-985
            o = list(zero)
            o[0:3] = self.end_pt
            last = self.pre_plan[self.N - 1]                                # .at(19)
            o[3:7] = attitude(float(last[14]), float(last[15]), float(last[16]))
            self.reset_output = True                                        # :981
            self.status = WAIT                                              # :983
            return END, o
        return NONE, zero                                                   # INIT_POSITION, WAIT (and anything else: no case)


def run_batch(pre_plan, have_traj, t_cur, status, pub_end, end_pt, odom=None, init_yaw=None, t_yaw=None, finish=None, reset_output=None,
              Ts=0.05, mass=0.74, g=9.81):
    """frp_nmpc_command_batch: S callbacks per planner.  Returns dict(cmd [B,S,16], kind [B,S], status [B], finish [B], reset_output [B]);
    finish / reset_output start from the arrays given (zeros when None) and change only where a callback wrote them."""
    pre_plan = np.asarray(pre_plan, dtype=np.float64)
    t_cur = np.asarray(t_cur, dtype=np.float64)
    B, S = t_cur.shape
    cmd = np.zeros((B, S, STRIDE)); kind = np.zeros((B, S), dtype=np.int32)
    st = np.array(status, dtype=np.int32).copy()
    fin = np.zeros(B, dtype=np.int32) if finish is None else np.array(finish, dtype=np.int32).copy()
    rst = np.zeros(B, dtype=np.int32) if reset_output is None else np.array(reset_output, dtype=np.int32).copy()
    for b in range(B):
        p = Planner(pre_plan[b], have_traj[b], st[b], pub_end[b], end_pt[b], None if odom is None else odom[b],
                    None if init_yaw is None else init_yaw[b], None, Ts, mass, g)
        for s in range(S):
            kind[b, s], cmd[b, s] = p.callback(t_cur[b, s], None if t_yaw is None else t_yaw[b][s])
        st[b] = p.status
        if p.finish is not None:
            fin[b] = p.finish
        if p.reset_output:
            rst[b] = 1
    return dict(cmd=cmd, kind=kind, status=st, finish=fin, reset_output=rst)


def snapshot(z, accept, pre_plan, have_traj):
    """frp_nmpc_command_snapshot: pre_mpc_output_ = mpc_output_; have_mpc_traj_ = true (:527-528) where accept != 0.  Returns copies."""
    pre_plan = np.array(pre_plan, dtype=np.float64); have_traj = np.array(have_traj, dtype=np.int32)
    m = np.asarray(accept) != 0
    pre_plan[m] = np.asarray(z, dtype=np.float64)[m]
    have_traj[m] = 1
    return pre_plan, have_traj
