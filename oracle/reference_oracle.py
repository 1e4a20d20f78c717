"""ORACLE for SURVEY 8f row f-4, first half (stage references, mode switch) -- TEST INFRASTRUCTURE ONLY.

Only tests/ (including tests/tools/) and __graft_entry__.smoke() may import this file; the product path
(forces_resilient_planner_amd/csrc/frp_reference.hip) never does.

Plain-Python restatement of NMPCSolver::getCurTraj (plan_manage/src/nmpc_solver.cpp:109-142) and
NMPCSolver::calculate_yaw (:834-862) as called by setFORCESParams (:486, :493-495), and of switch_to_final
(:436-447), statement by statement.
PARITY UNPINNED: nmpc_solver.cpp needs ROS and Eigen and the reference holds no vectors for these functions; they
are two dozen lines of scalar arithmetic.  The arithmetic and every branch are pinned to a 50-digit evaluation
(tests/golden/reference_mp.npz, tests/test_reference_cpu.py); the transcription of the control flow is not.
"""
import math

import numpy as np

PI = 3.1415926  # nmpc_solver.cpp:3
INT_INDEFINITE = 0x80000000


def cvttsd2si(q):
    """(int)double as the reference's machine performs it (x86 CVTTSD2SI, 32-bit destination), as the bit pattern of
    the int: truncation towards zero when the truncated value fits (-2**31 - 1 < q < 2**31), otherwise -- NaN
    included -- the "integer indefinite" value 0x80000000."""
    if q == q and -2.0 ** 31 - 1.0 < q < 2.0 ** 31:
        return int(q) & 0xFFFFFFFF
    return INT_INDEFINITE


def cvt_i32_f64(q):
    """(int)double as the device performs it (V_CVT_I32_F64), as a Python int: truncation towards zero, values
    outside the int range (the infinities included) saturate to INT_MAX / INT_MIN, NaN gives 0."""
    if q != q:
        return 0
    if q >= 2.0 ** 31:
        return 2 ** 31 - 1
    if q <= -2.0 ** 31:
        return -2 ** 31
    return int(q)


def references_one(kino_path, kino_size, time_offset, mpc_output, N, Ts=0.05, trace=None):
    """kino_path [K,3]; mpc_output [N+1,17].  Returns (ref_pos [N,3], ref_yaw [N], replan flag).  `trace`: a list that receives, per
    stage, the decisions taken: (kino_index, interpolated, looked ahead, far, unwrap: -1 / 0 / +1 times 2 PI).

    The sample index is `unsigned int kino_index = (int)(index_time / Ts)` (nmpc_solver.cpp:112-115): cvttsd2si, then
    read as unsigned.  The reference compares `kino_index + 1 < kino_size_` with kino_size_ a double
    (nmpc_utils.h:220), but forms `kino_index + 1` / `+ 5` in 32-bit unsigned arithmetic first: a negative index
    (time_offset <= -Ts) wraps to a small one or reads kino_path_[0xFFFFFFFF], out of bounds.  Here `+ 1` and `+ 5`
    are Python's unbounded ones ON PURPOSE: every index the conversion makes negative or indefinite (time_offset
    <= -Ts, a quotient >= 2**31, NaN, +-inf) is past the end, and the stage gets the END OF THE PATH.  That is
    the kernel's documented deviation (frp_reference.hip), not the reference's out-of-bounds read.  Offsets in
    (-Ts, 0) truncate to sample 0 with a negative interpolation weight, as in the reference."""
    ref_pos = np.zeros((N, 3)); ref_yaw = np.zeros(N)
    last_yaw = float(mpc_output[1, 16])  # :486
    replan = False
    for index in range(N):
        index_time = index * Ts + time_offset
        kino_index = cvttsd2si(index_time / Ts)  # (unsigned int)(int)(...)
        if kino_index + 1 < kino_size:
            pos = kino_path[kino_index] + math.fmod(index_time, Ts) / Ts * (kino_path[kino_index + 1] - kino_path[kino_index])
        else:
            pos = kino_path[kino_size - 1]
        fwd = kino_path[kino_index + 5] if kino_index + 5 < kino_size else kino_path[kino_size - 1]
        # calculate_yaw
        d = fwd - pos
        far = np.linalg.norm(d) > 0.1
        yaw_temp = math.atan2(d[1], d[0]) if far else last_yaw
        unwrap = 0
        if abs(yaw_temp - last_yaw) > PI:
            yaw = yaw_temp - 2 * PI if yaw_temp > 0 else yaw_temp + 2 * PI
            unwrap = -1 if yaw_temp > 0 else 1
        else:
            yaw = yaw_temp
        if trace is not None:
            trace.append((kino_index, kino_index + 1 < kino_size, kino_index + 5 < kino_size, bool(far), unwrap))
        yaw = 0.2 * last_yaw + 0.8 * yaw
        last_yaw = yaw
        ref_pos[index] = pos; ref_yaw[index] = yaw
        if index == 0 and np.linalg.norm(pos - mpc_output[1, 8:11]) > 1.0:
            replan = True
    return ref_pos, ref_yaw, replan


def mode_one(plan, time_offset, kino_size, end_pt, N, Ts=0.05, radius=1.0):
    """switch_to_final (nmpc_solver.cpp:436-447) for one planner: plan [N+1,17], end_pt [3].  True when the planner
    switches to the final solver: its horizon runs past the path, `max_index >= kino_size_`, or the plan's stage
    N - 1 is closer than `radius` to end_pt.

    max_index = (int)((N Ts + time_offset) / Ts).  Within int range that is truncation towards zero.  Outside it C++
    leaves the conversion undefined; the two device copies (mode_kernel, tick_end_kernel) compile it to one
    V_CVT_I32_F64, which SATURATES: a quotient >= 2**31 (+inf included) gives INT_MAX, so the planner switches; a
    quotient <= -2**31 (-inf included) gives INT_MIN, so it does not switch by the index; NaN gives 0, so it
    switches by the index only for kino_size <= 0.  (The reference's x86 gives INT_MIN in all three cases.)"""
    max_index = cvt_i32_f64((N * Ts + time_offset) / Ts)
    d = np.asarray(plan, dtype=float)[N - 1, 8:11] - np.asarray(end_pt, dtype=float)
    return bool(max_index >= kino_size or math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < radius)
