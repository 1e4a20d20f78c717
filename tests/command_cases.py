"""Shared inputs of the command-timer tests (tests/test_command_cpu.py, tests/test_gpu_command.py, tests/tools/gen_command_mp.py):
seeded, the same arrays on every run.  Only numpy: no device, no oracle."""
import math

import numpy as np

TS = 0.05
MP_N = 4     # horizon of the multiprecision cases: rows 0..3, so that the index is 0, 1 or 2
SPECIAL_YAW = (math.pi, -math.pi, 3.1415926, 7.0, -9.5)            # +-pi as doubles, the file's PI, unwrapped yaws beyond +-pi
SPECIAL_PITCH = (0.4 * math.pi, -0.4 * math.pi)


def plans(rng, B, N):
    """[B][N][17] rows like the solver's: rates, thrust, previous input, position, velocity, roll / pitch inside their bounds, a yaw that
    keeps turning (NOT wrapped: pre_mpc_output_ holds the solver's own yaw)."""
    p = np.zeros((B, N, 17))
    p[..., 0:3] = rng.uniform(-1.5, 1.5, (B, N, 3))
    p[..., 3] = rng.uniform(4.0, 12.0, (B, N))
    p[..., 4:8] = rng.uniform(-1.0, 8.0, (B, N, 4))
    p[..., 8:11] = np.cumsum(rng.normal(0, 0.08, (B, N, 3)), axis=1) + rng.uniform(-8, 8, (B, 1, 3))
    p[..., 11:14] = rng.uniform(-2.0, 2.0, (B, N, 3))
    p[..., 14:16] = rng.uniform(-0.6, 0.6, (B, N, 2))
    p[..., 16] = rng.uniform(-7.0, 7.0, (B, 1)) + np.cumsum(rng.normal(0, 0.1, (B, N)), axis=1)
    return p


def special_times(N, Ts=TS):
    """t_cur values at which the index or the branch changes."""
    end = (N - 1) * Ts
    out = [-1e-3, -0.0, 0.0, 1e-9, float("nan"), 1e300, -1e300, float("inf"), end, np.nextafter(end, 0.0), np.nextafter(end, 1.0), end + 0.013]
    out += [k * 0.05 for k in range(N + 1)] if Ts == 0.05 else []          # the float k * 0.05 against Ts = 0.05: fmod is 0 or just below Ts
    out += [float(np.nextafter(k * Ts, 0.0)) for k in range(1, N)]
    return out


def mixed_batch(B, S, N, seed, yaw_inputs=True, Ts=TS):
    """B planners, S callbacks: neighbouring planners in different states, so that neighbouring lanes take different branches."""
    rng = np.random.default_rng(seed)
    sp = special_times(N, Ts)
    status = np.array([(3, 2, 1, 3, 4, 0, 3, 7)[b % 8] for b in range(B)], dtype=np.int32)   # PUB_TRAJ, PUB_END, ROTATE_YAW, .., WAIT, INIT_POSITION, .., no state
    have = np.array([0 if b % 11 == 6 else 1 for b in range(B)], dtype=np.int32)
    pub_end = np.array([1 if (b // 2) % 2 else 0 for b in range(B)], dtype=np.int32)
    start = rng.uniform(-0.03, (N - 1) * Ts + 0.02, B)
    start[::5] = (N - 1) * Ts - rng.uniform(0.0, 0.03, len(start[::5]))                   # some plans run out inside the S callbacks
    t_cur = start[:, None] + 0.01 * np.arange(S)[None, :]
    for b in range(0, B, 3):                                                              # a special time somewhere in every third planner
        t_cur[b, (b // 3) % S] = sp[(b // 3) % len(sp)]
    odom = rng.uniform(-3, 3, (B, 9)); odom[:, 8] = rng.uniform(-3.1, 3.1, B)
    init_yaw = odom[:, 8] + np.array([(0.3, -0.3, 3.5, -3.5, 2.0, -2.0, 0.0, 3.1415926, -3.1415926)[b % 9] for b in range(B)])
    t_yaw = rng.uniform(0.0, 4.0, (B, 1)) + 0.01 * np.arange(S)[None, :]
    d = dict(pre_plan=plans(rng, B, N), have_traj=have, t_cur=t_cur, status=status, pub_end=pub_end, end_pt=rng.uniform(-8, 8, (B, 3)))
    if yaw_inputs:
        d.update(odom=odom, init_yaw=init_yaw, t_yaw=t_yaw)
    return d


def mp_cases():
    """(plan [C][MP_N][17], t [C]) of the multiprecision fixture: generic rows at generic times, times on and next to the row
    boundaries, and rows held constant at yaw = +-pi / pitch = +-0.4 pi (constant: the interpolated angle is then that double itself)."""
    rng = np.random.default_rng(9100)
    C0 = 96
    plan = plans(rng, C0, MP_N)
    t = rng.uniform(0.0, (MP_N - 1) * TS, C0)
    edge = [0.0, 0.05, 0.1, float(np.nextafter(0.05, 0.0)), float(np.nextafter(0.1, 1.0)), float(np.nextafter(0.15, 0.0)), 2 * 0.05, 1e-12]
    t[:len(edge)] = edge
    extra, te = [], []
    for yaw in SPECIAL_YAW:
        for pitch in SPECIAL_PITCH + (0.0, 0.3):
            row = plans(rng, 1, MP_N)[0]
            row[:, 14] = rng.uniform(-0.6, 0.6); row[:, 15] = pitch; row[:, 16] = yaw
            extra.append(row); te.append(rng.uniform(0.0, (MP_N - 1) * TS))
    return np.concatenate([plan, np.stack(extra)]), np.concatenate([t, np.array(te)])


def mp_yaws():
    """desired_yaw values of the position + yaw sample in the fixture."""
    rng = np.random.default_rng(9101)
    return np.concatenate([np.array(SPECIAL_YAW + (0.0, 1e-9, -1e-9, 0.4 * 3.1415926)), rng.uniform(-10.0, 10.0, 32)])
