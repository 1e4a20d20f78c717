"""Shared inputs of the vehicle tests (tests/test_vehicle_cpu.py, tests/test_gpu_vehicle.py, tests/tools/gen_vehicle_mp.py): the case list
of the multiprecision fixture, seeded, the same arrays on every run.  Only numpy: no device, no oracle.

A case is one vehicle and S = 5 command samples: x0 [9], hold0 [8], f_true [3], cmd [S][16], kind [S], n_sub.  The scalars are the same for
all: mass, g (the model's own), dt_cmd = 0.01, GAINS.  Cases 0 ... 31 run n_sub = 1, cases 32 ... 63 the same inputs at n_sub = 4.  Every
case sits well inside its branch (a clamp is missed or hit by a margin, a yaw error is not next to +-pi), so that the 50-digit
evaluation, the float64 restatement and the device take the same branches; the generator asserts it."""
import math

import numpy as np

S = 5
DT_CMD = 0.01
MASS, G = 0.745319, 9.81           # frp_model.hpp's: the controller is told the plant's mass
GAINS = dict(kp=(6.0, 6.0, 8.0), kv=(4.0, 4.0, 5.0), ka=(10.0, 10.0, 4.0))
NONE, TRAJ, END, YAW, NO_YAW_INPUT = 0, 1, 2, 3, -1
PER_N_SUB = 32
N_SUBS = (1, 4)
LABELS = ("traj",) * 10 + ("traj_then_none", "traj_then_none", "yaw", "yaw", "yaw_then_traj", "end", "end", "none", "no_yaw_input", "mixed", "mixed",
                           "thrust_high", "thrust_high", "thrust_low", "thrust_low", "rates", "rates", "rates_and_attitude", "yaw_wrap_up",
                           "yaw_wrap_down", "zero_acc", "zero_acc")


def _quat_xyz(roll, pitch, yaw):
    """(x, y, z, w) of q_x(roll) q_y(pitch) q_z(yaw): the order cmdTrajCallback publishes."""
    cr, sr, cp, sp, cy, sy = (math.cos(roll / 2), math.sin(roll / 2), math.cos(pitch / 2), math.sin(pitch / 2), math.cos(yaw / 2), math.sin(yaw / 2))
    return [sr * cp * cy + cr * sp * sy, cr * sp * cy - sr * cp * sy, cr * cp * sy + sr * sp * cy, cr * cp * cy - sr * sp * sy]


def _traj(rng, x, dp=0.05, yaw=None, t0=0.0):
    """S trajectory samples that start next to the state x and move on smoothly."""
    v = x[3:6] + rng.uniform(-0.2, 0.2, 3)
    a = rng.uniform(-1.0, 1.0, 3)
    p0 = x[0:3] + rng.uniform(-dp, dp, 3)
    yaw = x[8] + rng.uniform(-0.15, 0.15) if yaw is None else yaw
    rp = rng.uniform(-0.3, 0.3, 2)
    out = np.zeros((S, 16))
    for s in range(S):
        t = t0 + DT_CMD * s
        out[s, 0:3] = p0 + v * t + 0.5 * a * t * t
        out[s, 3:7] = _quat_xyz(rp[0], rp[1], yaw + 0.3 * t)
        out[s, 7:10] = v + a * t
        out[s, 10:13] = rng.uniform(-0.3, 0.3, 3)
        out[s, 13:16] = a
    return out


def _yaw(x, yaw):
    out = np.zeros(16)
    out[0:3] = x[0:3]
    out[5], out[6] = math.sin(0.5 * yaw), math.cos(0.5 * yaw)
    out[12] = yaw
    return out


def _end(p, rpy):
    out = np.zeros(16)
    out[0:3] = p
    out[3:7] = _quat_xyz(*rpy)
    return out


def _one(rng, label):
    x = np.zeros(9)
    x[0:3] = rng.uniform(-8, 8, 3); x[3:6] = rng.uniform(-1.5, 1.5, 3); x[6:8] = rng.uniform(-0.05, 0.05, 2); x[8] = rng.uniform(-2.5, 2.5)
    hold = np.zeros(8); hold[0:3] = x[0:3] + rng.uniform(-0.1, 0.1, 3); hold[3] = x[8] + rng.uniform(-0.2, 0.2)
    f = rng.uniform(-1.5, 1.5, 3)
    cmd = np.zeros((S, 16)); kind = np.zeros(S, dtype=np.int32)
    if label == "traj":
        cmd[:] = _traj(rng, x); kind[:] = TRAJ
    elif label == "traj_then_none":
        cmd[:] = _traj(rng, x); kind[:2] = TRAJ; cmd[2:] = 0.0
    elif label == "yaw":
        for s in range(S):
            cmd[s] = _yaw(x, x[8] + 0.3 + 0.01 * s)
        kind[:] = YAW
    elif label == "yaw_then_traj":
        cmd[:] = _traj(rng, x); kind[:] = TRAJ
        cmd[0] = _yaw(x, x[8] - 0.3); cmd[1] = _yaw(x, x[8] - 0.31); kind[:2] = YAW
    elif label == "end":
        cmd[:] = _traj(rng, x); kind[:] = TRAJ
        cmd[3] = _end(x[0:3] + rng.uniform(-0.1, 0.1, 3), (0.1, -0.2, x[8] + 0.1)); kind[3] = END; cmd[4] = 0.0; kind[4] = NONE
    elif label == "none":
        pass
    elif label == "no_yaw_input":
        kind[:] = NO_YAW_INPUT
    elif label == "mixed":
        cmd[:] = _traj(rng, x)
        kind[:] = (NONE, TRAJ, NO_YAW_INPUT, TRAJ, END)
        cmd[0] = 0.0; cmd[2] = 0.0; cmd[4, 7:16] = 0.0
    elif label == "thrust_high":
        cmd[:] = _traj(rng, x); kind[:] = TRAJ
        cmd[:, 2] += 4.0                      # kp_z * 4 m on top of g: far beyond 2 g m
    elif label == "thrust_low":
        cmd[:] = _traj(rng, x); kind[:] = TRAJ
        cmd[:, 13:16] = 0.0; cmd[:, 15] = -8.5   # |a| about 1.3 + the PD terms of a few centimetres: below g / 2
        cmd[:, 0:3] = x[0:3] + rng.uniform(-0.02, 0.02, 3); cmd[:, 7:10] = x[3:6]
    elif label == "rates":
        cmd[:] = _traj(rng, x); kind[:] = TRAJ
        cmd[:, 10:13] = (2.5, -2.5, 2.0)      # feed-forward rates beyond pi / 2
    elif label == "rates_and_attitude":
        cmd[:] = _traj(rng, x); kind[:] = TRAJ
        cmd[:, 0] += 30.0 * math.cos(x[8] + 0.5); cmd[:, 1] += 30.0 * math.sin(x[8] + 0.5)   # a sideways pull far beyond what 0.4 pi of tilt gives
    elif label == "yaw_wrap_up":
        x[8] = 3.0; hold[3] = 3.0
        cmd[:] = _traj(rng, x, yaw=-3.0); kind[:] = TRAJ
    elif label == "yaw_wrap_down":
        x[8] = -2.9; hold[3] = -2.9
        for s in range(S):
            cmd[s] = _yaw(x, 3.0)
        kind[:] = YAW
    elif label == "zero_acc":
        # the first sample's commanded acceleration is exactly 0: a_ff = (0, 0, -g) on the state itself; then nothing is published
        cmd[0, 0:3] = x[0:3]; cmd[0, 3:7] = _quat_xyz(0.0, 0.0, x[8]); cmd[0, 7:10] = x[3:6]; cmd[0, 15] = -G
        kind[0] = TRAJ
    else:
        raise ValueError(label)
    return dict(x0=x, hold0=hold, f_true=f, cmd=cmd, kind=kind, label=label)


def mp_cases():
    """The fixture's cases as arrays: x0 [C][9], hold0 [C][8], f_true [C][3], cmd [C][S][16], kind [C][S] int32, n_sub [C] int32, and the
    labels."""
    assert len(LABELS) == PER_N_SUB
    rng = np.random.default_rng(9200)
    base = [_one(rng, lb) for lb in LABELS]
    cases = [dict(c, n_sub=n) for n in N_SUBS for c in base]
    stack = lambda k, dt=np.float64: np.array([c[k] for c in cases], dtype=dt)
    return dict(x0=stack("x0"), hold0=stack("hold0"), f_true=stack("f_true"), cmd=stack("cmd"), kind=stack("kind", np.int32),
                n_sub=stack("n_sub", np.int32)), [c["label"] for c in cases]


# the smooth case of the order test: one sample of DT_ORDER seconds (long enough for the scheme's error to stand far above rounding),
# inputs held, nothing saturated
DT_ORDER = 0.05


def order_case():
    x = np.array([0.3, -0.2, 1.1, 0.8, -0.5, 0.2, 0.05, 0.05, 0.4])
    cmd = np.zeros((1, 16))
    cmd[0, 0:3] = x[0:3] + (0.05, 0.02, -0.03); cmd[0, 3:7] = _quat_xyz(0.0, 0.0, 0.6); cmd[0, 7:10] = (0.9, -0.4, 0.1)
    cmd[0, 10:13] = (0.4, -0.3, 0.2); cmd[0, 13:16] = (0.5, 0.3, -0.2)
    hold = np.zeros(8); hold[0:3] = x[0:3]; hold[3] = x[8]
    return dict(x0=x, hold0=hold, f_true=np.array([0.6, -0.4, 0.3]), cmd=cmd, kind=np.array([TRAJ], dtype=np.int32))


# frp_nmpc_vehicle_step's arguments: one good set (the addresses are placeholders: a test that launches replaces them) and every way to
# be refused with FRP_ERR_ARG
GOOD_STEP = dict(B=4, S=5, n_sub=4, mass=0.745319, g=9.81, dt_cmd=0.01, kp=(6.0, 6.0, 8.0), kv=(4.0, 4.0, 5.0), ka=(10.0, 10.0, 4.0),
                 x=0x1000, f_true=0x2000, cmd=0x3000, kind=0x4000, hold=0x5000, trace=0x6000, sat=0x7000)
BAD_STEP = [dict(B=0), dict(B=-3), dict(S=0), dict(n_sub=0), dict(n_sub=17), dict(B=1 << 20, S=1 << 12),
            dict(mass=0.0), dict(mass=-1.0), dict(mass=float("nan")), dict(mass=float("inf")), dict(dt_cmd=0.0), dict(dt_cmd=float("nan")),
            dict(dt_cmd=float("inf")), dict(g=float("nan")), dict(g=float("inf")),
            dict(kp=(6.0, -1e-300, 8.0)), dict(kv=(float("nan"), 4.0, 5.0)), dict(ka=(10.0, 10.0, float("inf"))), dict(ka=(-1.0, 0.0, 0.0)),
            dict(x=None), dict(f_true=None), dict(cmd=None), dict(kind=None), dict(hold=None)]
