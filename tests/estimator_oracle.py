"""Executable statement of the force estimator (include/frp_nmpc_estimator.h): a velocity-residual (momentum) observer on the planner's own
model.  NO reference counterpart -- the reference subscribes to a wrench that another node publishes
(plan_manage/src/nmpc_manage.cpp:366-418).  Python floats (IEEE doubles), one rounding per operation, written in the order the device code is
written in; the model is tests/vehicle_oracle.py's accel (frp_model.hpp's accel_t) with a zero force vector, and the thrust of a sample
is that file's control().

Per sample, with y the measured state after it and T the thrust it was flown with, the first that applies:
  not finite   count <- -1, SKIPPED, residual 0; f_hat and y_prev stay
  first        count == -1: y_prev <- y, count <- 0, FIRST, residual 0
  update       a0 = accel(v_prev, e_prev, T, 0), a1 = accel(v, e, T, 0); per axis dv = (v - v_prev) / dt, m = 0.5 * (a0 + a1), r = dv - m,
               f_hat <- f_hat + alpha * (r - f_hat); count <- min(count + 1, INT_MAX), y_prev <- y, ABSORBED
After the samples: force <- f_hat, fresh <- count >= min_samples."""
import math

from . import vehicle_oracle as VO

SKIPPED, FIRST, ABSORBED = 0, 1, 2   # FRP_EST_*
INT_MAX = 2 ** 31 - 1
ZERO = [0.0, 0.0, 0.0]


BREAKS = ("a0_alone", "next_thrust", "gain_complement", "fresh_strict", "nan_absorbed")


def update(meas, thrust, f_hat, y_prev, count, dt, alpha, min_samples, broken=None):
    """frp_nmpc_estimator_update for one vehicle: S = len(thrust) samples in order.  Returns (f_hat [3], y_prev [9], count, force [3],
    fresh, residual [S][3], status [S]); the inputs are not modified.
    broken: None, or one of BREAKS -- a deliberately WRONG scheme, for the tests that show the fixture tells them apart: a0 alone instead
    of the mean, the next sample's thrust, the gain 1 - alpha, fresh at count > min_samples, a non-finite sample absorbed."""
    assert broken is None or broken in BREAKS
    fh, yp, count = [float(v) for v in f_hat], [float(v) for v in y_prev], int(count)
    res, stat = [], []
    for s in range(len(thrust)):
        y, T = [float(v) for v in meas[s]], float(thrust[s])
        if broken == "next_thrust":
            T = float(thrust[min(s + 1, len(thrust) - 1)])
        r = [0.0, 0.0, 0.0]
        if broken != "nan_absorbed" and not (math.isfinite(T) and all(math.isfinite(v) for v in y)):
            count = -1
            st = SKIPPED
        elif count == -1:
            yp, count, st = list(y), 0, FIRST
        else:
            try:
                a0 = VO.accel(yp[3:6], yp[6:9], T, ZERO)
                a1 = VO.accel(y[3:6], y[6:9], T, ZERO)
            except ValueError:                       # (math.sin of an infinity: the broken "nan_absorbed" scheme alone gets here)
                a0 = a1 = [float("nan")] * 3
            for i in range(3):
                dv = (y[3 + i] - yp[3 + i]) / dt
                m = a0[i] if broken == "a0_alone" else 0.5 * (a0[i] + a1[i])
                r[i] = dv - m
                fh[i] = fh[i] + (1.0 - alpha if broken == "gain_complement" else alpha) * (r[i] - fh[i])
            count = min(count + 1, INT_MAX)
            yp, st = list(y), ABSORBED
        res.append(r); stat.append(st)
    return fh, yp, count, list(fh), int(count > min_samples if broken == "fresh_strict" else count >= min_samples), res, stat


def reset(f_hat, y_prev, count, force, fresh, mask=1):
    """frp_nmpc_estimator_reset for one vehicle: (f_hat, y_prev, count, force, fresh)."""
    if not mask:
        return list(f_hat), list(y_prev), count, list(force), fresh
    return [0.0] * 3, list(y_prev), -1, [0.0] * 3, 0


def thrusts(x, hold, cmd, kind, trace, mass=VO.MASS, g=VO.GRAV, kp=VO.DEFAULT_GAINS["kp"], kv=VO.DEFAULT_GAINS["kv"], ka=VO.DEFAULT_GAINS["ka"]):
    """frp_nmpc_vehicle_step_observed's thrust [S]: vehicle_oracle.control on the state and the hold BEFORE each sample -- x and hold before
    the first, trace[s - 1] and the hold the earlier samples left before sample s."""
    hold = [float(v) for v in hold]
    out = []
    for s in range(len(kind)):
        xs = [float(v) for v in (x if s == 0 else trace[s - 1])]
        sp = VO.setpoint([float(v) for v in cmd[s]], int(kind[s]), hold)
        out.append(VO.control(xs, sp, mass, g, kp, kv, ka)[1])
    return out


def fly(x, hold, f_true, cmd, kind, **kw):
    """vehicle_oracle.step with the thrust of every sample: (x, hold, trace, sat, thrust)."""
    xo, ho, trace, sat = VO.step(x, hold, f_true, cmd, kind, **kw)
    ctl = {k: kw[k] for k in ("mass", "g", "kp", "kv", "ka") if k in kw}
    return xo, ho, trace, sat, thrusts(x, hold, cmd, kind, trace, **ctl)
