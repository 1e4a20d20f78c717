"""CPU tests of the vehicle (include/frp_nmpc_vehicle.h): the restatement tests/vehicle_oracle.py against the reference's model callbacks
(tests/golden/stage_vectors.npz), against the same discrete scheme in 50 digits and a 50-digit integration of the ODE
(tests/golden/vehicle_mp.npz, tests/tools/gen_vehicle_mp.py), and against known answers sample by sample; the odometry callbacks; and
the boundary of the built library without a device: the symbols, the struct, every FRP_ERR_ARG rule before any device call."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from forces_resilient_planner_amd import solver

from . import vehicle_cases as VC
from . import vehicle_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = dict(mass=VC.MASS, g=VC.G, dt_cmd=VC.DT_CMD, **VC.GAINS)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "vehicle_mp.npz"))


def _err(got, pair):
    """max |got - (hi + lo)|, the subtraction of hi made first (exact for a got next to hi)."""
    got = np.asarray(got, dtype=np.float64)
    return float(np.max(np.abs((got - pair[..., 0]) - pair[..., 1])))


def _case(fx, c):
    return [fx[k][c] for k in ("x0", "hold0", "f_true", "cmd", "kind")], int(fx["n_sub"][c])


# ---- the model ----
def test_heun_step_at_the_planners_step_equals_the_reference_model_fixtures(golden_dir):
    """The fixtures of tests/test_oracle.py::test_stage_functions_match_reference_golden (the reference's CasADi callbacks): rows 0-8 of c
    are the next state of z's state under z's input and p's external force.  Held to that test's tolerance."""
    g = np.load(os.path.join(golden_dir, "stage_vectors.npz"))
    n = 0
    for i in range(g["z"].shape[0]):
        if int(g["stage"][i]) == 19:          # the last stage has no dynamics
            continue
        z, p = g["z"][i], g["p"][i]
        xn = np.array(VO.heun([float(v) for v in z[8:17]], [float(v) for v in z[0:3]], float(z[3]), [float(v) for v in p[3:6]], 0.05))
        ref = g["c"][i][:9]
        assert np.max(np.abs(xn - ref) / (1 + np.abs(ref))) < 1e-12, i
        n += 1
    assert n >= 150


def test_bounds_and_constants_are_the_models():
    """The oracle's copies against csrc/frp_model.hpp's text (the device takes them from that file's functions)."""
    src = open(os.path.join(ROOT, "forces_resilient_planner_amd", "csrc", "frp_model.hpp")).read()
    val = lambda name: float(re.search(r"constexpr double " + name + r" = ([0-9.eE+-]+);", src).group(1))
    assert (VO.MASS, VO.GRAV, VO.DRAG, VO.HALF_PI, VO.PI) == (val("MASS"), val("GRAV"), val("DRAG"), val("HALF_PI"), val("PI"))
    assert "case 3: case 7: return 0.5 * GRAV * MASS;" in src and "case 3: case 7: return 2.0 * GRAV * MASS;" in src
    assert "case 0: case 1: case 2: case 4: case 5: case 6: return -HALF_PI;" in src and "case 14: case 15: return -0.4 * PI;" in src
    assert (VO.THRUST_LO, VO.THRUST_HI, VO.RATE_LO, VO.ATT_LO) == (0.5 * VO.GRAV * VO.MASS, 2.0 * VO.GRAV * VO.MASS, -VO.HALF_PI, -0.4 * VO.PI)
    assert (VC.MASS, VC.G) == (VO.MASS, VO.GRAV) and VC.GAINS == VO.DEFAULT_GAINS
    d = solver.VEHICLE_DEFAULTS
    assert (d["mass"], d["g"], d["dt_cmd"]) == (VO.MASS, VO.GRAV, 0.01) and {k: d[k] for k in ("kp", "kv", "ka")} == VO.DEFAULT_GAINS


# ---- the scheme in 50 digits ----
def test_fixture_is_the_generators_case_list_and_covers_every_branch(fx):
    cases, labels = VC.mp_cases()
    for k, v in cases.items():
        assert np.array_equal(fx[k], v), k
    C = len(labels)
    assert C == 64 and int(fx["dps"].reshape(-1)[0]) == 50 and float(fx["tol_factor"].reshape(-1)[0]) == 8.0
    assert set(fx["n_sub"].tolist()) == {1, 4} and set(np.unique(fx["kind"]).tolist()) == {VO.NO_YAW_INPUT, VO.NONE, VO.TRAJ, VO.END, VO.YAW}
    sat = fx["sat"]
    seen = np.bitwise_or.reduce(sat.reshape(-1))
    for bit in (VO.SAT_THRUST_LO, VO.SAT_THRUST_HI, VO.SAT_PITCH, VO.SAT_RATE0, VO.SAT_RATE1, VO.SAT_RATE2, VO.SAT_ZERO_ACC, VO.SAT_YAW_WRAP):
        assert seen & bit, bit
    assert np.any(np.all(sat == 0, axis=1))                                      # and cases where nothing engaged
    for n in (1, 4):
        m = fx["n_sub"] == n
        assert np.bitwise_or.reduce(sat[m].reshape(-1)) == seen                    # at both step counts
    # a few units in the last place of a state of size < 16, accumulated over S * n_sub <= 20 steps
    tol = fx["tol_case"]
    assert tol.shape == (C,) and np.all(tol > 0) and np.max(tol) < 20 * 4 * 16 * 2.0 ** -52


def test_oracle_agrees_with_the_scheme_in_50_digits(fx):
    worst = 0.0
    for c in range(len(fx["n_sub"])):
        a, n_sub = _case(fx, c)
        x, hold, trace, sat = VO.step(*a, n_sub=n_sub, **SCALARS)
        e = _err(trace, fx["trace"][c])
        worst = max(worst, e)
        # (the stored tolerance is this very measurement on the generating machine; another libm may differ in the last place)
        assert e <= 2.0 * float(fx["tol_case"][c]), (c, e, float(fx["tol_case"][c]))
        assert sat == fx["sat"][c].tolist(), (c, sat)
        assert hold[0:3] == fx["hold"][c, 0:3, 0].tolist() and hold[4:8] == [0.0] * 4 and _err(hold[3], fx["hold"][c, 3]) <= 2.0 * float(fx["tol_hold"].reshape(-1)[0]), c
        assert x == trace[-1]
    print("oracle against the 50-digit scheme, worst absolute error over all cases: %.3e" % worst)
    assert worst <= 2.0 * float(np.max(fx["tol_case"]))


def test_the_scheme_is_second_order(fx):
    """One smooth sample of DT_ORDER seconds: the error of n_sub = 1 over that of n_sub = 2, both against the 50-digit integration of the
    ODE with (w, T) held, lies in [3, 5] -- Heun's local error is O(h^3), two half steps leave a quarter of one whole step's."""
    c = VC.order_case()
    dt = float(fx["dt_order"].reshape(-1)[0])
    assert dt == VC.DT_ORDER
    k = dict(SCALARS, dt_cmd=dt)
    errs = []
    for n_sub in (1, 2):
        x, _, _, sat = VO.step(c["x0"], c["hold0"], c["f_true"], c["cmd"], c["kind"], n_sub=n_sub, **k)
        assert sat == [0]
        d = (np.array(x) - fx["ode_x"][:, 0]) - fx["ode_x"][:, 1]
        assert np.max(np.abs(d[6:9])) <= 2.0 ** -52                               # e' = w is integrated exactly up to rounding
        errs.append(float(np.linalg.norm(d[0:6])))
    print("error against the ODE: n_sub = 1 %.3e, n_sub = 2 %.3e, ratio %.3f" % (errs[0], errs[1], errs[0] / errs[1]))
    assert errs[1] > 1e-10                                                         # the scheme's error, not rounding
    assert 3.0 <= errs[0] / errs[1] <= 5.0


# ---- known answers ----
def test_hover_stays_at_rest():
    """At rest, on its own setpoint, f_true = 0: a = g e3, T = mass g, and the plant's T / m - g cancels up to rounding."""
    for n_sub in (1, 4):
        S = 5
        x0 = [1.5, -2.25, 1.2, 0.0, 0.0, 0.0, 0.0, 0.0, 0.7]
        x, hold = VO.reset(x0)
        x, hold, trace, sat = VO.step(x, hold, [0.0] * 3, np.zeros((S, 16)), [VO.NONE] * S, n_sub=n_sub, **SCALARS)
        h = VC.DT_CMD / n_sub
        assert math.sqrt(sum(v * v for v in x[3:6])) <= S * n_sub * h * VC.G * 2.0 ** -50
        assert sat == [0] * S and x[6:9] == x0[6:9] and hold == [1.5, -2.25, 1.2, 0.7, 0.0, 0.0, 0.0, 0.0]


def _yaw_cmd(p, yaw):
    o = [0.0] * 16
    o[0:3] = p
    o[5], o[6], o[12] = math.sin(0.5 * yaw), math.cos(0.5 * yaw), yaw
    return o


def test_per_sample_behaviour():
    x0 = [0.5, 0.25, 1.0, 0.3, -0.2, 0.1, 0.02, -0.03, 0.4]
    f = [0.3, -0.1, 0.2]
    run = lambda x, hold, cmd, kind: VO.step(x, hold, f, cmd, kind, n_sub=4, **SCALARS)
    _, hold0 = VO.reset(x0)
    hold0[0] += 0.5
    # NONE and NO_YAW_INPUT keep the hold, whatever the row holds, and track it
    junk = [7.0] * 16
    a = run(x0, hold0, [junk], [VO.NONE])
    b = run(x0, hold0, [[0.0] * 16], [VO.NO_YAW_INPUT])
    assert a[0] == b[0] and a[1] == b[1] == hold0
    c = run(x0, hold0, [_yaw_cmd(hold0[0:3], hold0[3])], [VO.YAW])
    assert c[0] == a[0]                                                            # the same setpoint, published
    # YAW reads the yaw from slot 12, not from the quaternion, and zeroes everything else
    y = _yaw_cmd([0.6, 0.2, 1.1], 0.9)
    y[5], y[6] = math.sin(-0.3), math.cos(-0.3)                                    # a quaternion that says something else
    y[7:10] = [5.0, 5.0, 5.0]; y[13:16] = [3.0, 3.0, 3.0]                          # and slots YAW does not read
    d = run(x0, hold0, [y], [VO.YAW])
    assert d[1] == [0.6, 0.2, 1.1, 0.9, 0.0, 0.0, 0.0, 0.0]
    assert d[0] == run(x0, hold0, [_yaw_cmd([0.6, 0.2, 1.1], 0.9)], [VO.YAW])[0]
    # END: the feed-forward of the sample is what the timer wrote -- zeros -- and the yaw comes from the quaternion like TRAJ's
    e = _yaw_cmd([0.6, 0.2, 1.1], 0.9); e[12] = 0.0
    t = run(x0, hold0, [e], [VO.TRAJ])
    assert run(x0, hold0, [e], [VO.END])[0] == t[0] and abs(t[1][3] - 0.9) <= 2.0 ** -52 and t[1][0:3] == [0.6, 0.2, 1.1]
    e_ff = list(e); e_ff[7:10] = [0.4, 0.0, 0.0]; e_ff[13:16] = [0.0, 0.5, 0.0]
    assert run(x0, hold0, [e_ff], [VO.TRAJ])[0] != t[0]                            # (a feed-forward does change the flight)
    # sample s + 1 sees the state and the hold sample s left
    two = run(x0, hold0, [y, junk], [VO.YAW, VO.NONE])
    first = run(x0, hold0, [y], [VO.YAW])
    second = run(first[0], first[1], [junk], [VO.NONE])
    assert two[0] == second[0] and two[1] == second[1] and two[2] == [first[0], second[0]]


# ---- the odometry link ----
def test_message_and_callback_return_the_multiprecision_angles_and_world_velocity(fx):
    worst = dict(msg=0.0, odo=0.0)
    for c in range(len(fx["n_sub"])):
        x = fx["x_link"][c]
        for t, key in ((VO.ODOM_WORLD, "msg_world"), (VO.ODOM_BODY, "msg_body")):
            m = VO.message(x, t)
            worst["msg"] = max(worst["msg"], _err(m, fx[key][c]))
            st, prev, have = VO.odometry(m, 1, t, [9.0] * 9, [8.0] * 9, 0)
            worst["odo"] = max(worst["odo"], _err(st, fx["odo"][c]))
            assert prev == [9.0] * 9 and have == 1 and st[0:3] == list(x[0:3])
            if t == VO.ODOM_WORLD:
                assert st[3:6] == list(x[3:6])                                      # copied
    print("message and callback against the 50-digit values:", worst)
    assert worst["msg"] <= 2.0 * float(fx["tol_msg"].reshape(-1)[0]) and worst["odo"] <= 2.0 * float(fx["tol_odo"].reshape(-1)[0])
    # the callback's angles and world velocity are the state's own, to a few units in the last place of quantities below 4
    assert float(np.max(np.abs(fx["odo"].sum(axis=-1) - fx["x_link"]))) < 8 * 4 * 2.0 ** -52


def test_a_stale_message_changes_nothing_and_the_two_types_differ_on_a_rolled_vehicle():
    x = [1.0, 2.0, 1.2, 0.8, -0.3, 0.1, 0.5, 0.0, 0.3]
    st, prev = [float(k) for k in range(9)], [float(-k) for k in range(9)]
    for t in (VO.ODOM_WORLD, VO.ODOM_BODY):
        assert VO.odometry(VO.message(x, t), 0, t, st, prev, 0) == (st, prev, 0)
    mw, mb = VO.message(x, VO.ODOM_WORLD), VO.message(x, VO.ODOM_BODY)
    assert mw[0:7] == mb[0:7] and max(abs(a - b) for a, b in zip(mw[7:10], mb[7:10])) > 0.1
    # the body-frame twist read as a world-frame one is a different velocity; read by its own callback it is the state's
    wrong = VO.odometry(mb, 1, VO.ODOM_WORLD, st, prev, 0)[0]
    right = VO.odometry(mb, 1, VO.ODOM_BODY, st, prev, 0)[0]
    assert max(abs(a - b) for a, b in zip(wrong[3:6], x[3:6])) > 0.1 and max(abs(a - b) for a, b in zip(right, x)) < 1e-15


# ---- the boundary, without a device ----
FRP_ERR_NO_DEVICE, FRP_ERR_ARG = -1001, -1003
NAMES = ["frp_nmpc_vehicle_step", "frp_nmpc_vehicle_reset", "frp_nmpc_vehicle_message", "frp_nmpc_vehicle_odometry"]


def _has_gpu():
    try:
        return solver.lib().frp_nmpc_device_count() > 0
    except Exception:
        return False


def test_the_four_calls_are_declared_and_exported_and_the_struct_is_the_headers(tmp_path):
    own = open(os.path.join(ROOT, "include", "frp_nmpc_vehicle.h")).read()
    declared = re.findall(r"^int (frp_nmpc_\w+)\(", own, flags=re.M)
    assert declared == NAMES == solver.VEHICLE_EXPORTS
    lib = solver.lib()
    for n in NAMES:
        assert hasattr(lib, n), n
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    assert hdr.count('#include "frp_nmpc_vehicle.h"') == 1 and "#define FRP_NMPC_ABI_VERSION 7" in hdr and solver.ABI_VERSION == 7
    assert "structurally unpinned" in own.lower()
    lines = [f'_Static_assert(sizeof(frp_nmpc_vehicle) == {ctypes.sizeof(solver.VehicleArgs)}, "size");']
    for fld, _ in solver.VehicleArgs._fields_:
        lines.append(f'_Static_assert(offsetof(frp_nmpc_vehicle, {fld}) == {getattr(solver.VehicleArgs, fld).offset}, "{fld}");')
    lines.append('_Static_assert(FRP_VEHICLE_STATE == 9 && FRP_VEHICLE_HOLD_STRIDE == 8 && FRP_VEHICLE_MSG_STRIDE == 13 && FRP_VEHICLE_MAX_SUB == 16, "strides");')
    lines.append('_Static_assert(FRP_ODOM_WORLD == 1 && FRP_ODOM_BODY == 2, "types");')
    lines.append('_Static_assert(FRP_VEHICLE_SAT_THRUST_LO == 1 && FRP_VEHICLE_SAT_THRUST_HI == 2 && FRP_VEHICLE_SAT_ROLL == 4 && FRP_VEHICLE_SAT_PITCH == 8 && '
                 'FRP_VEHICLE_SAT_RATE0 == 16 && FRP_VEHICLE_SAT_ZERO_ACC == 128 && FRP_VEHICLE_SAT_YAW_WRAP == 256, "sat");')
    assert (solver.VEHICLE_STATE, solver.VEHICLE_HOLD_STRIDE, solver.VEHICLE_MSG_STRIDE, solver.VEHICLE_MAX_SUB) == (9, 8, 13, 16)
    assert (solver.ODOM_WORLD, solver.ODOM_BODY) == (VO.ODOM_WORLD, VO.ODOM_BODY) == (1, 2)
    assert (VO.SAT_THRUST_LO, VO.SAT_THRUST_HI, VO.SAT_ROLL, VO.SAT_PITCH, VO.SAT_RATE0, VO.SAT_ZERO_ACC, VO.SAT_YAW_WRAP) == (1, 2, 4, 8, 16, 128, 256) == \
        (solver.VEHICLE_SAT_THRUST_LO, solver.VEHICLE_SAT_THRUST_HI, solver.VEHICLE_SAT_ROLL, solver.VEHICLE_SAT_PITCH, solver.VEHICLE_SAT_RATE0,
         solver.VEHICLE_SAT_ZERO_ACC, solver.VEHICLE_SAT_YAW_WRAP)
    for inc in ("frp_nmpc.h", "frp_nmpc_vehicle.h"):   # through frp_nmpc.h, and on its own; strict C99 plus the C11 assertion
        src = tmp_path / ("layout_" + inc.replace(".", "_") + ".c")
        src.write_text('#include <stddef.h>\n#include "' + inc + '"\n' + "\n".join(lines) + "\nint main(void) { return 0; }\n")
        subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(src) + ".o"])


def _step(**kw):
    a = dict(VC.GOOD_STEP); a.update(kw)
    vals = [(ctypes.c_double * 3)(*a[f]) if f in ("kp", "kv", "ka") else a[f] for f, _ in solver.VehicleArgs._fields_]
    v = solver.VehicleArgs(*vals)             # the addresses are never dereferenced on the host; nothing is launched
    return solver.lib().frp_nmpc_vehicle_step(ctypes.byref(v), None)


def test_every_bad_argument_is_refused_before_any_device_call():
    """Without a device a call that passes the argument checks answers FRP_ERR_NO_DEVICE, so FRP_ERR_ARG here was decided before any device
    call; with a device the same order holds and the good calls are not made here (their addresses are not memory)."""
    l = solver.lib()
    assert l.frp_nmpc_vehicle_step(None, None) == FRP_ERR_ARG
    for bad in VC.BAD_STEP:
        assert _step(**bad) == FRP_ERR_ARG, bad
    vp = ctypes.c_void_p
    a, b, c, d, e = vp(0x1000), vp(0x2000), vp(0x3000), vp(0x4000), vp(0x5000)
    assert l.frp_nmpc_vehicle_reset(0, a, None, b, c, None) == FRP_ERR_ARG
    for args in ((4, None, None, b, c), (4, a, None, None, c), (4, a, None, b, None)):
        assert l.frp_nmpc_vehicle_reset(*args, None) == FRP_ERR_ARG, args
    for args in ((0, 1, a, b), (4, 0, a, b), (4, 3, a, b), (4, 1, None, b), (4, 2, a, None)):
        assert l.frp_nmpc_vehicle_message(*args, None) == FRP_ERR_ARG, args
    for args in ((0, 1, a, b, c, d, e), (4, 0, a, b, c, d, e), (4, 3, a, b, c, d, e), (4, 1, None, b, c, d, e), (4, 1, a, None, c, d, e),
                 (4, 2, a, b, None, d, e), (4, 2, a, b, c, d, None)):
        assert l.frp_nmpc_vehicle_odometry(*args, None) == FRP_ERR_ARG, args
    if not _has_gpu():
        assert _step() == FRP_ERR_NO_DEVICE and _step(trace=None, sat=None) == FRP_ERR_NO_DEVICE and _step(kp=(0.0, 0.0, 0.0), n_sub=16) == FRP_ERR_NO_DEVICE
        assert l.frp_nmpc_vehicle_reset(4, a, None, b, c, None) == FRP_ERR_NO_DEVICE
        assert l.frp_nmpc_vehicle_message(4, 2, a, b, None) == FRP_ERR_NO_DEVICE
        assert l.frp_nmpc_vehicle_odometry(4, 1, a, b, c, None, e, None) == FRP_ERR_NO_DEVICE      # state_prev is optional


def test_period_without_a_vehicle_makes_the_calls_it_made_before():
    """FleetFSM.period's text: the vehicle's launches stand after the commands and under `if vehicle is not None` alone."""
    import inspect
    src = inspect.getsource(solver.FleetFSM.period)
    body = src[src.index('"""', src.index('"""') + 3):]
    assert body.count("vehicle.step(") == 1 and body.count("vehicle.odometry(") == 1
    tail = body[body.index("tk.reset_output = self.commands_out.reset_output"):]
    assert re.search(r"if vehicle is not None:\n\s+vehicle\.step\(self\.commands_out, s\)\n\s+vehicle\.odometry\(self, stream=s\)\n\s+return self\.commands_out", tail)
    assert inspect.signature(solver.FleetFSM.period).parameters["vehicle"].default is None
