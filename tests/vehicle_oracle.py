"""Executable statement of the vehicle (include/frp_nmpc_vehicle.h): the tracking plant that flies the command timer's samples, and the
reference's two odometry callbacks (plan_manage/src/nmpc_manage.cpp:421-478) with the message producer that feeds them.  Python floats
(IEEE doubles), one rounding per operation, written in the order the device code is written in.

  plant        the planner's own model: nonlinear_dynamics.m:21-40 as forces_resilient_planner_amd/csrc/frp_model.hpp's accel() holds it
               (mass, drag and gravity are THAT file's constants), integrated by Heun steps -- transit.m's scheme at another step size.
  controller   no reference counterpart (the reference flies RotorS' controller, which is not in its tree): a feed-forward + PD
               acceleration command, turned into a thrust and a desired roll / pitch by inverting the model's thrust direction, and a
               proportional attitude loop on the body rates.  Every bound is the planner's own stage bound (mpc_generator_normal.m:33-46).
  hold         what the vehicle tracks when the timer publishes nothing: the last published POSITION and YAW, with zero velocity, rate
               and acceleration feed-forward -- a position hold.  Slots 0-2 position, 3 yaw, 4-7 zero.
  odometry     the two callbacks statement by statement; mav_msgs is not in the reference tree, so getEulerAnglesFromQuaternion is the
               formula of its public header, restated (structurally unpinned)."""
import math

NONE, TRAJ, END, YAW, NO_YAW_INPUT = 0, 1, 2, 3, -1   # FRP_COMMAND_*
ODOM_WORLD, ODOM_BODY = 1, 2                          # FRP_ODOM_*: odometryCallback, odometryTransCallback
HOLD_STRIDE, MSG_STRIDE, CMD_STRIDE = 8, 13, 16

# frp_model.hpp
MASS, GRAV, DRAG = 0.745319, 9.81, 0.33
HALF_PI = 1.5707963267948966
PI = 3.14159265358979323846
THRUST_LO, THRUST_HI = 0.5 * GRAV * MASS, 2.0 * GRAV * MASS   # lower_bound(3), upper_bound(3)
RATE_LO, RATE_HI = -HALF_PI, HALF_PI                          # lower_bound(0..2), upper_bound(0..2)
ATT_LO, ATT_HI = -0.4 * PI, 0.4 * PI                          # lower_bound(14..15), upper_bound(14..15)

# sat[b][s]: which clamps engaged in sample s (FRP_VEHICLE_SAT_*)
SAT_THRUST_LO, SAT_THRUST_HI, SAT_ROLL, SAT_PITCH, SAT_RATE0, SAT_RATE1, SAT_RATE2, SAT_ZERO_ACC, SAT_YAW_WRAP = (1 << k for k in range(9))

DEFAULT_GAINS = dict(kp=(6.0, 6.0, 8.0), kv=(4.0, 4.0, 5.0), ka=(10.0, 10.0, 4.0))


def accel(v, e, T, f):
    """frp_model.hpp accel_t: zB T/m + f - g e3 - d (I - zB zB') v."""
    sr, cr, sp, cp, sy, cy = math.sin(e[0]), math.cos(e[0]), math.sin(e[1]), math.cos(e[1]), math.sin(e[2]), math.cos(e[2])
    zb0 = cy * sp * cr + sy * sr
    zb1 = sy * sp * cr - cy * sr
    zb2 = cp * cr
    zv = zb0 * v[0] + zb1 * v[1] + zb2 * v[2]
    a = T * (1.0 / MASS) + DRAG * zv
    return [a * zb0 - DRAG * v[0] + f[0], a * zb1 - DRAG * v[1] + f[1], a * zb2 - DRAG * v[2] + f[2] - GRAV]


def heun(x, w, T, f, h):
    """One Heun step of (p, v, e) with the rates w and the thrust T held: frp_model.hpp rk2 at step h."""
    v, e = x[3:6], x[6:9]
    a1 = accel(v, e, T, f)
    vt = [v[i] + h * a1[i] for i in range(3)]
    et = [e[i] + h * w[i] for i in range(3)]
    a2 = accel(vt, et, T, f)
    return [x[i] + 0.5 * h * (v[i] + vt[i]) for i in range(3)] + [v[i] + 0.5 * h * (a1[i] + a2[i]) for i in range(3)] + et


def clamp(v, lo, hi):
    """(value, -1 / 0 / +1: which bound engaged)"""
    if v < lo:
        return lo, -1
    if v > hi:
        return hi, 1
    return v, 0


def yaw_of_quaternion(x, y, z, w):
    """atan2(-R01, R00) of Quaternion::toRotationMatrix's entries, term by term: the yaw of the X * Y * Z product cmdTrajCallback composes."""
    ty, tz = 2.0 * y, 2.0 * z
    twz, txy, tyy, tzz = tz * w, ty * x, ty * y, tz * z
    return math.atan2(-(txy - twz), 1.0 - (tyy + tzz))


def setpoint(cmd, kind, hold):
    """(p_ref, v_ref, w_ff, a_ff, yaw_ref) of one sample; `hold` (8 floats) is updated where the sample published."""
    zero = [0.0, 0.0, 0.0]
    if kind == TRAJ or kind == END:
        p, v, w, a = list(cmd[0:3]), list(cmd[7:10]), list(cmd[10:13]), list(cmd[13:16])
        yaw = yaw_of_quaternion(cmd[3], cmd[4], cmd[5], cmd[6])
    elif kind == YAW:
        p, v, w, a = list(cmd[0:3]), zero, zero, zero
        yaw = cmd[12]
    else:
        return list(hold[0:3]), zero, zero, zero, hold[3]
    hold[0:3] = p
    hold[3] = yaw
    hold[4:8] = [0.0, 0.0, 0.0, 0.0]
    return p, v, w, a, yaw


def wrap_yaw(d):
    """d - 2 pi ceil((d - pi) / (2 pi)): into (-pi, pi].  Returns (wrapped, whether it moved)."""
    k = math.ceil((d - PI) / (2.0 * PI))
    return d - 2.0 * PI * k, k != 0.0


def control(x, sp, mass, g, kp, kv, ka):
    """(w [3], T, sat) from the state and a setpoint."""
    p_ref, v_ref, w_ff, a_ff, yaw = sp
    sat = 0
    a = [a_ff[i] + kp[i] * (p_ref[i] - x[i]) + kv[i] * (v_ref[i] - x[3 + i]) for i in range(3)]
    a[2] = a[2] + g
    na = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    T, c = clamp(mass * na, THRUST_LO, THRUST_HI)
    sat |= SAT_THRUST_LO if c < 0 else SAT_THRUST_HI if c > 0 else 0
    if na == 0.0:
        zb = [0.0, 0.0, 1.0]
        sat |= SAT_ZERO_ACC
    else:
        zb = [a[0] / na, a[1] / na, a[2] / na]
    sy, cy = math.sin(yaw), math.cos(yaw)
    cx = cy * zb[0] + sy * zb[1]
    cyy = cy * zb[1] - sy * zb[0]
    s, _ = clamp(-cyy, -1.0, 1.0)
    roll, c = clamp(math.asin(s), ATT_LO, ATT_HI)
    sat |= SAT_ROLL if c else 0
    pitch, c = clamp(math.atan2(cx, zb[2]), ATT_LO, ATT_HI)
    sat |= SAT_PITCH if c else 0
    dyaw, moved = wrap_yaw(yaw - x[8])
    sat |= SAT_YAW_WRAP if moved else 0
    err = [roll - x[6], pitch - x[7], dyaw]
    w = []
    for i in range(3):
        wi, c = clamp(w_ff[i] + ka[i] * err[i], RATE_LO, RATE_HI)
        sat |= (SAT_RATE0 << i) if c else 0
        w.append(wi)
    return w, T, sat


def step(x, hold, f_true, cmd, kind, mass=MASS, g=GRAV, dt_cmd=0.01, n_sub=4, kp=DEFAULT_GAINS["kp"], kv=DEFAULT_GAINS["kv"], ka=DEFAULT_GAINS["ka"]):
    """frp_nmpc_vehicle_step for one vehicle: S = len(kind) samples in order.  Returns (x, hold, trace [S][9], sat [S]); the inputs are
    not modified."""
    x, hold = [float(v) for v in x], [float(v) for v in hold]
    f = [float(v) for v in f_true]
    h = dt_cmd / n_sub
    trace, sats = [], []
    for s in range(len(kind)):
        sp = setpoint([float(v) for v in cmd[s]], int(kind[s]), hold)
        w, T, sat = control(x, sp, mass, g, kp, kv, ka)
        for _ in range(n_sub):
            x = heun(x, w, T, f, h)
        trace.append(list(x)); sats.append(sat)
    return x, hold, trace, sats


def reset(x0):
    """frp_nmpc_vehicle_reset for one vehicle: (x, hold) -- the vehicle holds its own position and yaw."""
    x0 = [float(v) for v in x0]
    return list(x0), [x0[0], x0[1], x0[2], x0[8], 0.0, 0.0, 0.0, 0.0]


# ---- the odometry link ----
def qmul(a, b):
    """a * b, Eigen's scalar quat_product; (w, x, y, z)."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz,
            aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx)


def euler_quaternion(e):
    """qz * qy * qx of NMPCSolver::eulerToRot (nmpc_solver.cpp:554-564) as (w, x, y, z)."""
    hr, hp, hy = 0.5 * e[0], 0.5 * e[1], 0.5 * e[2]
    qx = (math.cos(hr), math.sin(hr), 0.0, 0.0)
    qy = (math.cos(hp), 0.0, math.sin(hp), 0.0)
    qz = (math.cos(hy), 0.0, 0.0, math.sin(hy))
    return qmul(qmul(qz, qy), qx)


def rotation(q):
    """Quaternion::toRotationMatrix, (w, x, y, z) -> 3 x 3 list."""
    w, x, y, z = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def message(x, odom_type):
    """frp_nmpc_vehicle_message: position, quaternion x y z w, linear twist (world frame for ODOM_WORLD, body frame R' v for ODOM_BODY),
    angular twist 0 (the plant state carries none and the callbacks read none)."""
    x = [float(v) for v in x]
    q = euler_quaternion(x[6:9])
    v = x[3:6]
    if odom_type == ODOM_BODY:
        R = rotation(q)
        v = [R[0][i] * v[0] + R[1][i] * v[1] + R[2][i] * v[2] for i in range(3)]
    return x[0:3] + [q[1], q[2], q[3], q[0]] + v + [0.0, 0.0, 0.0]


def euler_of_quaternion(q):
    """mav_msgs::getEulerAnglesFromQuaternion, (w, x, y, z) -> (roll, pitch, yaw)."""
    w, x, y, z = q
    return [math.atan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + y * y)),
            math.asin(2.0 * (w * y - z * x)),
            math.atan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))]


def odometry(msg, fresh, odom_type, state, state_prev, have_odom):
    """odometryCallback (ODOM_WORLD, :421-448) / odometryTransCallback (ODOM_BODY, :456-478) for one planner; returns (state, state_prev,
    have_odom)."""
    if not fresh:
        return list(state), list(state_prev), have_odom
    m = [float(v) for v in msg]
    q = (m[6], m[3], m[4], m[5])
    v = m[7:10]
    if odom_type == ODOM_BODY:
        R = rotation(q)
        v = [R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2] for i in range(3)]
    return m[0:3] + v + euler_of_quaternion(q), list(state), 1
