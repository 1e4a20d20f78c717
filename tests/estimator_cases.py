"""Shared inputs of the estimator tests (tests/test_estimator_cpu.py, tests/test_gpu_estimator.py, tests/tools/gen_estimator_mp.py): the case
list of the multiprecision fixture, seeded, the same arrays on every run.  Only numpy: no device, no oracle.

A case is one estimator and one call of S = 1 or 5 samples: meas [5][9] and thrust [5] (rows beyond S are zero and unread), f_hat0 [3],
y_prev0 [9], count0, alpha, min_samples; dt = 0.01 for all.  The measurements are smooth synthetic states -- the update is a function of
its inputs, whatever flew them.  Which of the three branches a sample takes is decided by its inputs exactly (finite or not, count == -1 or
not), so the 50-digit evaluation, the float64 restatement and the device take the same ones; EXPECT holds the status sequence every label
must produce, and the generator asserts it.  Cases 0 ... PER_ALPHA - 1 run alpha = 1, the rest the same inputs at ALPHAS[1]."""
import math

import numpy as np

S_MAX = 5
DT = 0.01
MASS, G = 0.745319, 9.81                     # frp_model.hpp's
THRUST_LO, THRUST_HI = 0.5 * G * MASS, 2.0 * G * MASS
ALPHAS = (1.0, -math.expm1(-DT / 0.1))       # the whole residual, and the default filter (tau = 0.1 s at 100 Hz)
MIN_SAMPLES = 10
INT_MAX = 2 ** 31 - 1
SKIPPED, FIRST, ABSORBED = 0, 1, 2           # FRP_EST_*
NONFINITE = (float("nan"), float("inf"), float("-inf"))

A5, A1 = (ABSORBED,) * 5, (ABSORBED,)
NAN_AT_2 = (ABSORBED, ABSORBED, SKIPPED, FIRST, ABSORBED)
# label -> (S, count0, status of every sample, count after the call, fresh after the call)
EXPECT = dict([("smooth", (5, 3, A5, 8, 0)), ("smooth_s1", (1, 3, A1, 4, 0)),
               ("first_call", (5, -1, (FIRST,) + (ABSORBED,) * 4, 4, 0)), ("first_call_s1", (1, -1, (FIRST,), 0, 0)),
               ("crossing", (5, 8, A5, 13, 1)), ("not_yet", (5, 4, A5, 9, 0)), ("exactly", (5, 5, A5, 10, 1)), ("exactly_s1", (1, 9, A1, 10, 1)),
               ("nan_last", (5, 12, (ABSORBED,) * 4 + (SKIPPED,), -1, 0)), ("nan_s1", (1, 12, (SKIPPED,), -1, 0)),
               ("thrust_lo", (5, 3, A5, 8, 0)), ("thrust_hi", (5, 3, A5, 8, 0)),
               ("rolled", (5, 3, A5, 8, 0)), ("pitched", (5, 3, A5, 8, 0)), ("rolled_pitched", (5, 3, A5, 8, 0)),
               ("zero_residual", (5, 20, A5, 25, 1)), ("count_saturates", (5, INT_MAX - 2, A5, INT_MAX, 1))] +
              [("nan_pos_%d" % k, (5, 12, NAN_AT_2, 1, 0)) for k in range(10)])      # positions 0-8: the measurement's slots, 9: the thrust
LABELS = ("smooth",) * 4 + ("smooth_s1",) * 2 + ("first_call", "first_call_s1", "crossing", "not_yet", "exactly", "exactly_s1") + \
    tuple("nan_pos_%d" % k for k in range(10)) + ("nan_last", "nan_s1", "thrust_lo", "thrust_hi", "rolled", "pitched", "rolled_pitched",
                                                  "zero_residual", "count_saturates")
PER_ALPHA = len(LABELS)


def _one(rng, label):
    S, count0 = EXPECT[label][0], EXPECT[label][1]
    tilt = dict(rolled=(0.9, 0.05), pitched=(0.05, 0.9), rolled_pitched=(0.8, 0.8)).get(label, (0.3, 0.3))
    y = np.zeros(9)
    y[0:3] = rng.uniform(-8, 8, 3); y[3:6] = rng.uniform(-1.5, 1.5, 3)
    y[6] = rng.choice((-1.0, 1.0)) * rng.uniform(0.5, 1.0) * tilt[0]; y[7] = rng.choice((-1.0, 1.0)) * rng.uniform(0.5, 1.0) * tilt[1]
    y[8] = rng.uniform(-2.5, 2.5)
    f_hat0 = rng.uniform(-1.0, 1.0, 3)
    thrust = rng.uniform(THRUST_LO, THRUST_HI, S_MAX)
    if label == "thrust_lo":
        thrust[:] = THRUST_LO
    elif label == "thrust_hi":
        thrust[:] = THRUST_HI
    if label == "zero_residual":
        # a hover: level, at rest, T = m g as the controller forms it -- the model's acceleration and the velocity difference are both 0
        # up to the rounding of T / m - g; the residual is, and the estimate decays towards it
        y[3:8] = 0.0
        thrust[:] = MASS * G
    y_prev0 = y.copy()
    meas = np.zeros((S_MAX, 9))
    rate = rng.uniform(-1.0, 1.0, 3)
    acc = rng.uniform(-5.0, 5.0, 3)
    for s in range(S):
        if label != "zero_residual":
            y = y.copy()
            y[0:3] += DT * y[3:6]
            y[3:6] += DT * (acc + rng.uniform(-0.5, 0.5, 3))
            y[6:9] += DT * rate
        meas[s] = y
    if label.startswith("nan_pos_"):
        k = int(label[8:])
        bad = NONFINITE[k % 3]
        if k < 9:
            meas[2, k] = bad
        else:
            thrust[2] = bad
    elif label == "nan_last":
        meas[4, 4] = float("nan")
    elif label == "nan_s1":
        thrust[0] = float("inf")
    thrust[S:] = 0.0
    return dict(meas=meas, thrust=thrust, S=S, f_hat0=f_hat0, y_prev0=y_prev0, count0=count0, min_samples=MIN_SAMPLES, label=label)


def mp_cases():
    """The fixture's cases as arrays: meas [C][5][9], thrust [C][5], S [C] int32, f_hat0 [C][3], y_prev0 [C][9], count0 [C] int32,
    alpha [C], min_samples [C] int32, and the labels."""
    rng = np.random.default_rng(13100)
    base = [_one(rng, lb) for lb in LABELS]
    cases = [dict(c, alpha=a) for a in ALPHAS for c in base]
    stack = lambda k, dt=np.float64: np.array([c[k] for c in cases], dtype=dt)
    return dict(meas=stack("meas"), thrust=stack("thrust"), S=stack("S", np.int32), f_hat0=stack("f_hat0"), y_prev0=stack("y_prev0"),
                count0=stack("count0", np.int32), alpha=stack("alpha"), min_samples=stack("min_samples", np.int32)), [c["label"] for c in cases]


# which case every deliberately broken oracle (estimator_oracle.BREAKS) must fail, by label
BREAK_FAILS = dict(a0_alone="smooth", next_thrust="smooth", gain_complement="smooth", fresh_strict="exactly", nan_absorbed="nan_pos_4")

# frp_nmpc_estimator_update's arguments: one good set (the addresses are placeholders: a test that launches replaces them) and every way
# to be refused with FRP_ERR_ARG
GOOD_UPDATE = dict(B=4, S=5, min_samples=10, dt=0.01, alpha=0.1, meas=0x1000, thrust=0x2000, f_hat=0x3000, y_prev=0x4000, count=0x5000, force=0x6000,
                   fresh=0x7000, residual=0x8000, status=0x9000)
BAD_UPDATE = [dict(B=0), dict(B=-3), dict(S=0), dict(S=-1), dict(B=1 << 20, S=1 << 12), dict(min_samples=0), dict(min_samples=-2),
              dict(dt=0.0), dict(dt=-0.01), dict(dt=float("nan")), dict(dt=float("inf")),
              dict(alpha=0.0), dict(alpha=-0.1), dict(alpha=1.0000000000000002), dict(alpha=float("nan")), dict(alpha=float("inf")),
              dict(meas=None), dict(thrust=None), dict(f_hat=None), dict(y_prev=None), dict(count=None), dict(force=None), dict(fresh=None)]
