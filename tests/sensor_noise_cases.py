"""Shared inputs of the sensor-noise tests (tests/test_sensor_noise_cpu.py, tests/test_gpu_sensor_noise.py, tests/tools/gen_sensor_noise_mp.py),
built without random numbers: the same arrays on every run.  Only numpy and math: no device, no oracle.

States: B = 67 vehicles (one workgroup is 256 lanes: a partial wave and a partial workgroup), S = 5 samples each; lanes with a NaN or an
infinity in a position, a velocity or an angle, counters across 2^31 and near 2^63, a bias that starts away from zero, one sigma that is zero.
Depth: F = 3 frames of 37 x 53 (1961 pixels: seven full workgroups and a partial one per frame), frame 1 inactive; pixels 0, 1, 2, 65535 and
ranges between.  Scan: S = 2 scans of P = 131 points, count = (131, 70); NaN points, an infinite one, a point at the origin."""
import math

import numpy as np

DT = 0.01
SEED, ID0 = 20240917, -7
B, S = 67, 5
SIGMA_P, SIGMA_V, SIGMA_A = (0.02, 0.03, 0.05), (0.05, 0.05, 0.1), (0.01, 0.0, 0.02)      # (the pitch is measured exactly: a zero sigma)
SIGMA_BIAS, TAU_BIAS = (0.1, 0.1, 0.2), (5.0, 5.0, 2.0)
DEPTH = dict(sigma0=0.002, sigma2=0.0005, p_drop=0.1, depth_scale=1000.0)
SCAN = dict(sigma0=0.01, sigma1=0.002, p_drop=0.1)
F, ROWS, COLS = 3, 37, 53
DEPTH_ACTIVE = (1, 0, 1)
DEPTH_CALLS = 2                    # the fixture holds the images after the first and after the second call
SCANS, P = 2, 131
COUNT = (131, 70)
INF, NAN = float("inf"), float("nan")
# the lanes the state case was built around: (lane, sample, component, value)
BAD = ((3, 1, 0, NAN), (5, 2, 4, INF), (7, 2, 1, NAN), (7, 3, 1, NAN), (11, 0, 8, -INF), (13, 4, 2, INF), (66, 0, 0, NAN), (66, 0, 1, NAN), (66, 0, 2, NAN))


def coefficients():
    a = [math.exp(-DT / u) for u in TAU_BIAS]
    return a, [s * math.sqrt(1.0 - v * v) for s, v in zip(SIGMA_BIAS, a)]


def params(zero=False, id0=ID0):
    """The oracle's `par` of the case set; zero: every sigma and p_drop zero."""
    a, c = coefficients()
    z3 = [0.0, 0.0, 0.0]
    if zero:
        return dict(seed=SEED, id0=id0, sigma_p=z3, sigma_v=z3, sigma_a=z3, bias_a=a, bias_c=z3, depth_scale=DEPTH["depth_scale"], depth_sigma0=0.0, depth_sigma2=0.0,
                    depth_p_drop=0.0, scan_sigma0=0.0, scan_sigma1=0.0, scan_p_drop=0.0)
    return dict(seed=SEED, id0=id0, sigma_p=list(SIGMA_P), sigma_v=list(SIGMA_V), sigma_a=list(SIGMA_A), bias_a=a, bias_c=c, depth_scale=DEPTH["depth_scale"],
                depth_sigma0=DEPTH["sigma0"], depth_sigma2=DEPTH["sigma2"], depth_p_drop=DEPTH["p_drop"], scan_sigma0=SCAN["sigma0"], scan_sigma1=SCAN["sigma1"],
                scan_p_drop=SCAN["p_drop"])


def states_case():
    """x_true [B,S,9], bias0 [B,3], tick0 [B] int64."""
    b, s, j = np.meshgrid(np.arange(B), np.arange(S), np.arange(9), indexing="ij")
    x = 0.375 * b - 12.0 + 0.0625 * (j + 1) * np.sin(0.7 * b + 1.3 * j) + 0.01 * s * (j - 4)
    x[2, :, 3:6] = 0.0                       # a vehicle at rest
    x[4, :, 6:9] = -0.0                      # negative zeros keep their sign
    for lane, smp, comp, v in BAD:
        x[lane, smp, comp] = v
    bias0 = np.zeros((B, 3))
    bias0[1::4] = [0.05, -0.025, 0.125]
    tick0 = (np.arange(B, dtype=np.int64) * 13) % 50
    tick0[9], tick0[10], tick0[12] = 2 ** 31 - 2, 2 ** 40, 2 ** 63 - 3        # (the last: the counter wraps as the device's does)
    return x, bias0, tick0


def depth_case():
    """images [F,ROWS,COLS] uint16."""
    f, r, c = np.meshgrid(np.arange(F), np.arange(ROWS), np.arange(COLS), indexing="ij")
    idx = r * COLS + c
    img = 400 + (idx * 37 + f * 1013 + (idx * idx) % 911 * 7) % 9000         # 0.4 ... 9.4 m
    img[idx % 11 == 3] = 0                   # no return
    img[idx % 13 == 5] = 1                   # sigma0 is two units: the noise drives these below 1
    img[idx % 17 == 7] = 2
    img[idx % 19 == 9] = 65535               # sigma is 2.1 m there: the noise drives half of these beyond the uint16
    img[idx % 23 == 11] = 64000
    return img.astype(np.uint16)


def scan_case():
    """points [SCANS,P,3], origin [SCANS,3], count [SCANS] int32."""
    s, p = np.meshgrid(np.arange(SCANS), np.arange(P), indexing="ij")
    origin = np.array([[0.5, -1.25, 1.0], [-3.0, 2.0, 0.75]])
    az, el, rng = 0.37 * p + 0.9 * s, 0.4 * np.sin(0.11 * p), 1.0 + (p * 29 % 97) * 0.3
    d = np.stack([rng * np.cos(el) * np.cos(az), rng * np.cos(el) * np.sin(az), rng * np.sin(el)], axis=-1)
    pts = origin[:, None, :] + d
    pts[0, 5] = [NAN, NAN, NAN]              # a point another noise call already lost
    pts[0, 17, 1] = NAN
    pts[1, 3] = origin[1]                    # a point at the origin: r == 0
    pts[1, 8, 2] = INF
    pts[1, 100] = [NAN, 1.0, 2.0]            # beyond count: neither read nor written
    return pts, origin, np.array(COUNT, dtype=np.int32)
