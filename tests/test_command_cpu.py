"""CPU tests of the command timer (include/frp_nmpc_command.h): the restatement tests/command_oracle.py against a 50-digit evaluation
of the mathematics (tests/golden/command_mp.npz, tests/tools/gen_command_mp.py) and against known answers, one per arrow of the state
machine of NMPCSolver::cmdTrajCallback (plan_manage/src/nmpc_solver.cpp:865-987); and the boundary of the built library without a
device: the symbols, the struct, every FRP_ERR_ARG rule before any device call."""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from forces_resilient_planner_amd import solver

from . import command_cases as CC
from . import command_oracle as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, TS = 20, 0.05


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "command_mp.npz"))


def _err(got, pair):
    """max |got - (hi + lo)|, the subtraction of hi made first (exact for a got next to hi)."""
    got = np.asarray(got, dtype=np.float64)
    return float(np.max(np.abs((got - pair[..., 0]) - pair[..., 1])))


def oracle_on_fixture(fx):
    plan, t = fx["plan"], fx["t"]
    Ts, mass, g = float(fx["Ts"].reshape(-1)[0]), float(fx["mass"].reshape(-1)[0]), float(fx["g"].reshape(-1)[0])
    rows, out = [], []
    for c in range(len(t)):
        mpcq = CO.interpolate(plan[c], int(t[c] / Ts), float(t[c]), Ts)
        rows.append(mpcq); out.append(CO.trajectory_point(mpcq, mass, g))
    return np.array(rows), np.array(out)


def test_fixture_is_the_generators_case_list_and_is_consistent(fx):
    plan, t = CC.mp_cases()
    assert np.array_equal(fx["plan"], plan) and np.array_equal(fx["t"], t) and np.array_equal(fx["yaws"], CC.mp_yaws())
    assert int(fx["dps"].reshape(-1)[0]) == 50 and float(fx["tol_factor"].reshape(-1)[0]) == 8.0
    q = fx["quat"].sum(axis=-1)
    assert np.max(np.abs(np.linalg.norm(q, axis=1) - 1.0)) < 4e-16
    sc = fx["yaw_sc"].sum(axis=-1)
    assert np.max(np.abs(np.hypot(sc[:, 0], sc[:, 1]) - 1.0)) < 4e-16
    # the measured oracle errors are a few units in the last place of the quantities' size (|q| <= 1, |acc| <= 12 / 0.74 + 9.81 < 32, |pose| < 16)
    ulp = 2.0 ** -52
    assert 0 < float(fx["tol_quat"].reshape(-1)[0]) < 4 * ulp and 0 < float(fx["tol_yaw"].reshape(-1)[0]) < 2 * ulp
    assert 0 < float(fx["tol_acc"].reshape(-1)[0]) < 4 * 16 * ulp and 0 < float(fx["tol_pose"].reshape(-1)[0]) < 4 * 8 * ulp


def test_oracle_agrees_with_the_multiprecision_evaluation(fx):
    rows, out = oracle_on_fixture(fx)
    slots = list(range(0, 4)) + list(range(8, 17))
    e = dict(pose=_err(rows[:, slots], fx["pose"][:, slots]), quat=_err(out[:, 3:7], fx["quat"]), acc=_err(out[:, 13:16], fx["acc"]))
    ys = fx["yaws"]
    e["yaw"] = _err(np.c_[np.sin(0.5 * ys), np.cos(0.5 * ys)], fx["yaw_sc"])
    print("oracle against the 50-digit values:", e)
    # (the stored tolerances are this very measurement on the generating machine; another libm may differ in the last place)
    for k, v in e.items():
        assert v <= 2.0 * float(fx["tol_" + k].reshape(-1)[0]), (k, v, float(fx["tol_" + k].reshape(-1)[0]))
    # the published slots are the interpolated row's
    assert np.array_equal(out[:, 0:3], rows[:, 8:11]) and np.array_equal(out[:, 7:10], rows[:, 11:14]) and np.array_equal(out[:, 10:13], rows[:, 0:3])


def _Rx(a):
    return np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])


def _Ry(a):
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])


def _Rz(a):
    return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])


ANGLES = [(0.3, -0.2, 1.0), (0.0, 0.0, 0.0)] + [(0.1, p, y) for p in CC.SPECIAL_PITCH + (0.0,) for y in CC.SPECIAL_YAW] + [(-0.6, 0.6, -3.0)]


@pytest.mark.parametrize("roll,pitch,yaw", ANGLES)
def test_quaternion_is_unit_and_rotates_as_rx_ry_rz_while_the_thrust_turns_as_rz_ry_rx(roll, pitch, yaw):
    x, y, z, w = CO.attitude(roll, pitch, yaw)
    assert abs(math.sqrt(x * x + y * y + z * z + w * w) - 1.0) < 4e-16
    R = np.array(CO.to_rotation_matrix((w, x, y, z)))
    assert np.max(np.abs(R - _Rx(roll) @ _Ry(pitch) @ _Rz(yaw))) < 2e-15       # :933 -- X * Y * Z, the opposite order to eulerToRot
    E = np.array(CO.euler_to_rot([roll, pitch, yaw]))
    assert np.max(np.abs(E - _Rz(yaw) @ _Ry(pitch) @ _Rx(roll))) < 2e-15       # :561
    o = CO.trajectory_point([0, 0, 0, 7.3] + [0] * 10 + [roll, pitch, yaw], 0.74, 9.81)
    want = (_Rz(yaw) @ _Ry(pitch) @ _Rx(roll))[:, 2] * 7.3 / 0.74 - np.array([0, 0, 9.81])
    assert np.max(np.abs(np.array(o[13:16]) - want)) < 4e-14
    if roll == pitch == yaw == 0.0:
        assert o[3:7] == [0.0, 0.0, 0.0, 1.0] and o[13:16] == [0.0, 0.0, 7.3 / 0.74 - 9.81]   # hover: the thrust minus g


# ---- the state machine, one case per arrow ----
def ramp():
    """pre_plan whose row k, slot j is 100 j + k: every interpolated slot is 100 j + k + w."""
    return np.arange(17)[None, :] * 100.0 + np.arange(N)[:, None]


def planner(status=CO.PUB_TRAJ, have=True, pub_end=False, **kw):
    return CO.Planner(ramp(), have, status, pub_end, (1.0, 2.0, 3.0), **kw)


def test_no_trajectory_publishes_nothing_and_touches_nothing():
    p = planner(have=False, pub_end=True)
    assert p.callback(0.1) == (CO.NONE, [0.0] * 16) and p.status == CO.PUB_TRAJ and p.finish is None and not p.reset_output
    assert p.callback(99.0) == (CO.NONE, [0.0] * 16) and p.status == CO.PUB_TRAJ and p.finish is None   # not even the end of the plan


def test_negative_time_takes_the_else_branch():
    p = planner()
    k, o = p.callback(-1e-9)
    assert k == CO.NONE and o == [0.0] * 16 and p.finish == 1 and p.status == CO.PUB_TRAJ
    k, o = p.callback(-0.0)                                                     # -0.0 >= 0.0: published, row 0
    assert k == CO.TRAJ and o[0:3] == [800.0, 900.0, 1000.0] and p.finish == 0


@pytest.mark.parametrize("k", range(N + 1))
def test_time_exactly_k_ts_for_the_float_k_times_0_05(k):
    """t = the float k * 0.05 against Ts = the float 0.05: the quotient's truncation picks the row, fmod's exact remainder the fraction."""
    t = k * 0.05
    p = planner()
    kind, o = p.callback(t)
    i = int(t / TS)
    n = math.floor(Fraction(t) / Fraction(TS))                                  # the real quotient's floor
    assert Fraction(math.fmod(t, TS)) == Fraction(t) - n * Fraction(TS)         # fmod is exact
    assert i in (n, n + 1)                                                      # (the rounded quotient may reach the next integer)
    if i >= N - 1:
        assert kind == CO.NONE and p.finish == 1
        return
    w = math.fmod(t, TS) / TS
    assert kind == CO.TRAJ and p.finish == 0
    assert o[0:3] == [800.0 + i + w * 1.0, 900.0 + i + w * 1.0, 1000.0 + i + w * 1.0] and o[10] == i + w * 1.0 and o[7] == 1100.0 + i + w * 1.0
    assert i == k and (w < 1e-14 or w > 1 - 1e-14)                              # on these twenty the quotient is k; the fraction is 0 or one rounding away from it


def test_one_ulp_either_side_of_the_plans_end():
    end = (N - 1) * TS
    lo, hi = float(np.nextafter(end, 0.0)), float(np.nextafter(end, 1.0))
    assert int(lo / TS) == N - 2 and int(end / TS) == N - 1
    p = planner()
    assert p.callback(lo)[0] == CO.TRAJ and p.finish == 0
    assert p.callback(end)[0] == CO.NONE and p.finish == 1
    assert p.callback(hi)[0] == CO.NONE and p.finish == 1 and p.status == CO.PUB_TRAJ


@pytest.mark.parametrize("t", [float("nan"), 1e300, -1e300, float("inf"), float("-inf"), 2147483648.0 * TS * 2])
def test_times_whose_cast_is_undefined_take_the_else_branch(t):
    p = planner(pub_end=True)
    assert p.callback(t) == (CO.NONE, [0.0] * 16) and p.finish == 1 and p.status == CO.PUB_END


def test_pub_traj_to_pub_end_to_wait_inside_one_call():
    b = dict(pre_plan=ramp()[None], have_traj=[1], t_cur=[[0.93, 0.96, 0.97, 0.98]], status=[CO.PUB_TRAJ], pub_end=[1], end_pt=[[1.0, 2.0, 3.0]])
    r = CO.run_batch(**b)
    assert r["kind"].tolist() == [[CO.TRAJ, CO.NONE, CO.END, CO.NONE]] and r["status"].tolist() == [CO.WAIT]
    assert r["finish"].tolist() == [1] and r["reset_output"].tolist() == [1]
    end = r["cmd"][0, 2]
    assert end[0:3].tolist() == [1.0, 2.0, 3.0] and np.all(end[7:16] == 0.0)
    assert end[3:7].tolist() == list(CO.attitude(1419.0, 1519.0, 1619.0))       # the attitude of row N - 1 (.at(19))
    assert np.all(r["cmd"][0, 1] == 0.0) and np.all(r["cmd"][0, 3] == 0.0)
    three = CO.run_batch(**dict(b, t_cur=[[0.93, 0.96, 0.97]]))                   # S = 3: the arrow ends in WAIT all the same
    assert three["kind"].tolist() == [[CO.TRAJ, CO.NONE, CO.END]] and three["status"].tolist() == [CO.WAIT]


def test_pub_end_raised_before_the_plan_is_finished_keeps_publishing_the_trajectory():
    r = CO.run_batch(ramp()[None], [1], [[0.10, 0.11, 0.12]], [CO.PUB_TRAJ], [1], [[1.0, 2.0, 3.0]], finish=[1], reset_output=[0])
    assert r["kind"].tolist() == [[CO.TRAJ] * 3] and r["status"].tolist() == [CO.PUB_TRAJ] and r["finish"].tolist() == [0] and r["reset_output"].tolist() == [0]


def test_init_position_and_wait_publish_nothing_and_leave_finish_alone():
    for st in (CO.INIT_POSITION, CO.WAIT, 7):
        r = CO.run_batch(ramp()[None], [1], [[0.1, 0.2]], [st], [1], [[1.0, 2.0, 3.0]], finish=[5], reset_output=[9])
        assert np.all(r["kind"] == CO.NONE) and np.all(r["cmd"] == 0.0) and r["status"].tolist() == [st]
        assert r["finish"].tolist() == [5] and r["reset_output"].tolist() == [9]


PI = CO.PI
# (init_yaw - odom_yaw, the rate callInitYaw stores): the five regions of :239-257
YAW_REGIONS = [(6.0, 2 * PI - 6.0), (-6.0, -6.0 + 2 * PI), (2.0, 0.4 * PI), (-2.0, -0.4 * PI), (0.5, 0.5)]


@pytest.mark.parametrize("d,rate", YAW_REGIONS)
def test_rotate_yaw_in_each_region_of_call_init_yaw_runs_into_its_cap(d, rate):
    odom = [0.5, -0.5, 1.5, 0, 0, 0, 0, 0, 0.25]
    init = odom[8] + d
    assert CO.init_yaw_dot(init, odom[8]) == pytest.approx(rate, abs=1e-15)
    dot = CO.init_yaw_dot(init, odom[8])
    p = planner(status=CO.ROTATE_YAW, odom=odom, init_yaw=init)
    seen = []
    for t in (0.0, 0.5, 1.0, 2.0, 5.0, 50.0):
        k, o = p.callback(float("nan"), t)                                       # (t_cur is not read in this state)
        yaw_temp = odom[8] + t * dot
        want = (init if init < yaw_temp else yaw_temp) if init - odom[8] >= 0 else (init if yaw_temp < init else yaw_temp)
        assert k == CO.YAW and o[12] == want and o[0:3] == odom[0:3] and o[3:5] == [0.0, 0.0] and o[7:12] == [0.0] * 5 and o[13:16] == [0.0] * 3
        assert o[5] == math.sin(0.5 * want) and o[6] == math.cos(0.5 * want)
        seen.append(want)
    assert p.status == CO.ROTATE_YAW and p.finish is None
    if d == -6.0:      # folded to a POSITIVE rate although the target is below: max() lets the yaw run away from it (as written, :886)
        assert seen[-1] == odom[8] + 50.0 * dot and seen[-1] > init
    elif d == 6.0:     # the first fold yields 2 PI - d > 0: the long way round, capped at the target
        assert seen[0] == odom[8] and seen[-1] == init
    else:
        assert seen[0] == odom[8] and seen[-1] == init                           # the min / max cap


def test_rotate_yaw_without_its_inputs_is_flagged_per_sample():
    r = CO.run_batch(ramp()[None], [1], [[0.1, 0.2]], [CO.ROTATE_YAW], [0], [[1.0, 2.0, 3.0]])
    assert r["kind"].tolist() == [[CO.NO_YAW_INPUT] * 2] and np.all(r["cmd"] == 0.0) and r["status"].tolist() == [CO.ROTATE_YAW]


def test_snapshot_copies_only_accepted_planners():
    rng = np.random.default_rng(3)
    z = rng.normal(size=(5, N, 17)); pre = rng.normal(size=(5, N, 17)); have = np.array([0, 1, 0, 1, 0], dtype=np.int32)
    p2, h2 = CO.snapshot(z, [1, 0, 0, -3, 2], pre, have)
    assert np.array_equal(p2[[0, 3, 4]], z[[0, 3, 4]]) and np.array_equal(p2[[1, 2]], pre[[1, 2]]) and h2.tolist() == [1, 1, 0, 1, 1]


def test_mixed_batch_covers_every_kind_and_both_ends_of_the_plan():
    """The shared GPU case really mixes the branches (a case list that lost one would test less without failing)."""
    for n in (2, 4, 20, 64):
        c = CC.mixed_batch(70, 5, n, 100 + n)
        r = CO.run_batch(**c)
        assert set(np.unique(r["kind"])) == {CO.NONE, CO.TRAJ, CO.END, CO.YAW}, n
        assert set(np.unique(r["status"])) >= {CO.INIT_POSITION, CO.ROTATE_YAW, CO.PUB_TRAJ, CO.WAIT, 7}
        assert r["finish"].any() and r["reset_output"].any() and np.any(np.diff(r["kind"][:, :], axis=1) != 0)
        assert np.any(np.isnan(c["t_cur"])) and np.any(c["have_traj"] == 0)
        assert np.all(np.isfinite(r["cmd"]))


# ---- the boundary, without a device ----
FRP_ERR_NO_DEVICE, FRP_ERR_ARG = -1001, -1003
NAMES = ["frp_nmpc_command_snapshot", "frp_nmpc_command_batch"]


def _has_gpu():
    try:
        return solver.lib().frp_nmpc_device_count() > 0
    except Exception:
        return False


def test_the_two_calls_are_declared_and_exported_and_the_struct_is_the_headers(tmp_path):
    lib = solver.lib()
    assert solver.COMMAND_EXPORTS == NAMES
    for n in NAMES:
        assert hasattr(lib, n), n
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    assert '#include "frp_nmpc_command.h"' in hdr
    own = open(os.path.join(ROOT, "include", "frp_nmpc_command.h")).read()
    for n in NAMES:
        assert n + "(" in own
    lines = [f'_Static_assert(sizeof(frp_nmpc_command) == {ctypes.sizeof(solver.Command)}, "size");']
    for fld, _ in solver.Command._fields_:
        lines.append(f'_Static_assert(offsetof(frp_nmpc_command, {fld}) == {getattr(solver.Command, fld).offset}, "{fld}");')
    # the reference's enum (nmpc_utils.h:115-122) in its order, and the bindings' copies
    lines.append('_Static_assert(FRP_CMD_INIT_POSITION == 0 && FRP_CMD_ROTATE_YAW == 1 && FRP_CMD_PUB_END == 2 && FRP_CMD_PUB_TRAJ == 3 && FRP_CMD_WAIT == 4, "CMD_STATUS");')
    lines.append('_Static_assert(FRP_COMMAND_NONE == 0 && FRP_COMMAND_TRAJ == 1 && FRP_COMMAND_END == 2 && FRP_COMMAND_YAW == 3 && FRP_COMMAND_NO_YAW_INPUT == -1 && FRP_COMMAND_STRIDE == 16, "kinds");')
    assert (solver.CMD_INIT_POSITION, solver.CMD_ROTATE_YAW, solver.CMD_PUB_END, solver.CMD_PUB_TRAJ, solver.CMD_WAIT) == (0, 1, 2, 3, 4)
    assert (CO.INIT_POSITION, CO.ROTATE_YAW, CO.PUB_END, CO.PUB_TRAJ, CO.WAIT) == (0, 1, 2, 3, 4)
    assert (solver.COMMAND_NONE, solver.COMMAND_TRAJ, solver.COMMAND_END, solver.COMMAND_YAW, solver.COMMAND_NO_YAW_INPUT, solver.COMMAND_STRIDE) == (0, 1, 2, 3, -1, 16)
    for inc in ("frp_nmpc.h", "frp_nmpc_command.h"):   # through frp_nmpc.h, and on its own; strict C99 plus the C11 assertion
        src = tmp_path / ("layout_" + inc.replace(".", "_") + ".c")
        src.write_text('#include <stddef.h>\n#include "' + inc + '"\n' + "\n".join(lines) + "\nint main(void) { return 0; }\n")
        subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(src) + ".o"])


GOOD = dict(B=4, N=20, S=5, Ts=0.05, mass=0.74, g=9.81, pre_plan=0x1000, t_cur=0x2000, status=0x3000, have_traj=0x4000, pub_end=0x5000,
            end_pt=0x6000, odom=0x7000, init_yaw=0x8000, t_yaw=0x9000, cmd=0xa000, kind=0xb000, finish=0xc000, reset_output=0xd000)


def _batch(**kw):
    a = dict(GOOD); a.update(kw)
    c = solver.Command(*[a[f] for f, _ in solver.Command._fields_])   # the addresses are never dereferenced on the host; nothing is launched
    return solver.lib().frp_nmpc_command_batch(ctypes.byref(c), None)


BAD = ([dict(B=0), dict(B=-1), dict(N=1), dict(N=65), dict(N=0), dict(S=0), dict(S=-2), dict(B=1 << 20, S=1 << 12),
        dict(Ts=0.0), dict(Ts=-0.05), dict(Ts=float("nan")), dict(Ts=float("inf")), dict(mass=0.0), dict(mass=float("nan")), dict(mass=float("inf")),
        dict(g=float("nan")), dict(g=float("inf"))]
       + [{k: None} for k in ("pre_plan", "t_cur", "status", "have_traj", "pub_end", "end_pt", "cmd", "kind", "finish", "reset_output")]
       + [dict(odom=None), dict(init_yaw=None), dict(t_yaw=None), dict(odom=None, init_yaw=None), dict(odom=None, t_yaw=None), dict(init_yaw=None, t_yaw=None)])


@pytest.mark.parametrize("kw", BAD, ids=["-".join(f"{k}={v}" for k, v in kw.items()) for kw in BAD])
def test_batch_argument_errors_come_before_any_device_call(kw):
    assert _batch(**kw) == FRP_ERR_ARG


def test_null_struct_and_snapshot_argument_errors():
    lib = solver.lib()
    assert lib.frp_nmpc_command_batch(None, None) == FRP_ERR_ARG
    P = ctypes.c_void_p
    good = [4, 20, P(0x1000), P(0x2000), P(0x3000), P(0x4000), None]
    for i, bad in ((0, 0), (0, -1), (1, 1), (1, 65), (2, None), (3, None), (4, None), (5, None)):   # accept == NULL included: the policy is the caller's
        a = list(good); a[i] = bad
        assert lib.frp_nmpc_command_snapshot(*a) == FRP_ERR_ARG, (i, bad)


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_valid_arguments_without_a_device_fail_loudly():
    """Accepted arguments reach the device check and nothing else: no CPU path.  The yaw inputs may be absent as a set; g = 0 and a
    negative g are values, not errors."""
    P = ctypes.c_void_p
    assert _batch() == FRP_ERR_NO_DEVICE
    assert _batch(odom=None, init_yaw=None, t_yaw=None) == FRP_ERR_NO_DEVICE
    assert _batch(g=0.0) == FRP_ERR_NO_DEVICE and _batch(g=-9.81) == FRP_ERR_NO_DEVICE and _batch(N=2, S=1, B=1) == FRP_ERR_NO_DEVICE and _batch(N=64, S=1000) == FRP_ERR_NO_DEVICE
    assert solver.lib().frp_nmpc_command_snapshot(4, 20, P(0x1000), P(0x2000), P(0x3000), P(0x4000), None) == FRP_ERR_NO_DEVICE
