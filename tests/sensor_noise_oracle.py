"""Executable statement of the sensor noise (include/frp_nmpc.h section 16): seeded errors of the states a fleet measures, of depth images
and of float64 point scans.  NO reference counterpart -- the reference flies RotorS, whose plugins add the noise.  Python floats (IEEE
doubles), one rounding per operation, written in the order the device code is written in; the integers are Python's, reduced mod 2^64
where the device's wrap.  The generator is tests/disturbance_oracle.py's (mix, stream_key), keyed per channel:
    h_sample = mix(stream_key(seed, id0 + i, k) + TAG)            i: the vehicle, frame or scan; k: its counter
    states: h = h_sample, normals j = 0 ... 11;   pixels and points: h = mix(h_sample + index), normal j = 0, uniform j = 2
CHOSEN, not derived: white Gaussian noise plus one Gauss-Markov position bias; sigma(z) = sigma0 + sigma2 z^2 per pixel, sigma(r) = sigma0 +
sigma1 r per point; independent pixels and points; no rolling shutter, no latency, no quantisation beyond the image's uint16.
A term that is zero is not added: with every sigma and p_drop zero the three functions return their input to the bit.

`brk`: a set of named ALTERATIONS of the statement, each of which tests/test_sensor_noise_cpu.py shows to fail a named check -- what the
checks can see.  () is the statement."""
import math

from .disturbance_oracle import MASK, TWO_PI, U1_DIV, U2_DIV, mix, stream_key

TAG_STATE, TAG_DEPTH, TAG_SCAN = 0x53544154, 0x44455054, 0x5343414E
NAN = float("nan")
BREAKS = ("tag_dropped", "tick_not_advanced", "bias_on_non_finite", "floor_without_half", "zero_pixel_redrawn", "count_ignored")


def sample_key(seed, ident, k, tag, brk=()):
    return mix((stream_key(seed, ident & MASK, k & MASK) + (0 if "tag_dropped" in brk else tag)) & MASK)


def normal_words(h, j):
    return mix((h + 2 * j) & MASK), mix((h + 2 * j + 1) & MASK)


def normal(h, j):
    r0, r1 = normal_words(h, j)
    u1, u2 = float((r0 >> 11) + 1) / U1_DIV, float(r1 >> 11) / U2_DIV
    return math.sqrt(-2.0 * math.log(u1)) * math.cos(TWO_PI * u2)


def uniform(h, j):
    return float(mix((h + j) & MASK) >> 11) / U2_DIV


def add_term(x, e):
    return x if e == 0.0 else x + e


def coefficients(sigma, tau, dt):
    """(a [3], c [3]) of the position bias as solver.SensorNoise computes them on the host (Disturbance's gust coefficients)."""
    a = [math.exp(-dt / u) for u in tau]
    return a, [s * math.sqrt(1.0 - v * v) for s, v in zip(sigma, a)]


def states(x, bias, tick, b, par, brk=()):
    """frp_nmpc_sensor_noise_states for vehicle b: x [S][9] -> (meas [S][9], y [9], bias [3], tick) as advance != 0 leaves them."""
    bias = [float(v) for v in bias]
    out = []
    for s, row in enumerate(x):
        row = [float(v) for v in row]
        h = sample_key(par["seed"], par["id0"] + b, tick + s, TAG_STATE, brk)
        m = list(row)
        for i in range(3):
            if math.isfinite(row[i]):
                bias[i] = par["bias_a"][i] * bias[i] + par["bias_c"][i] * normal(h, i)
                m[i] = add_term(add_term(row[i], bias[i]), par["sigma_p"][i] * normal(h, 3 + i))
            elif "bias_on_non_finite" in brk:
                bias[i] = par["bias_a"][i] * bias[i] + par["bias_c"][i] * normal(h, i)
            if math.isfinite(row[3 + i]):
                m[3 + i] = add_term(row[3 + i], par["sigma_v"][i] * normal(h, 6 + i))
            if math.isfinite(row[6 + i]):
                m[6 + i] = add_term(row[6 + i], par["sigma_a"][i] * normal(h, 9 + i))
        out.append(m)
    return out, list(out[-1]), bias, tick if "tick_not_advanced" in brk else tick + len(x)


def reset(bias, tick, y, x, mask=1):
    """frp_nmpc_sensor_noise_reset for one vehicle: (bias, tick, y)."""
    return ([0.0, 0.0, 0.0], 0, list(x)) if mask else (bias, tick, y)


def depth(img, f, tick, par, active=1, brk=(), detail=None):
    """frp_nmpc_sensor_noise_depth for frame f: img [rows][cols] of ints -> (out [rows][cols] of ints, tick).  detail: a list that receives
    (index, u, v + 0.5 or None for a dropped pixel) of every pixel that drew."""
    if not active:
        return [list(r) for r in img], tick
    cols = len(img[0])
    hs = sample_key(par["seed"], par["id0"] + f, tick, TAG_DEPTH, brk)
    scale, s0, s2, p_drop = par["depth_scale"], par["depth_sigma0"], par["depth_sigma2"], par["depth_p_drop"]
    out = []
    for r, row in enumerate(img):
        o = []
        for c, pix in enumerate(row):
            pix = int(pix)
            if pix == 0 and "zero_pixel_redrawn" not in brk:
                o.append(0)
                continue
            idx = r * cols + c
            h = mix((hs + idx) & MASK)
            u = uniform(h, 2)
            if u < p_drop:
                o.append(0)
                if detail is not None:
                    detail.append((idx, u, None))
                continue
            z = float(pix) / scale
            sigma = s0 + (s2 * z) * z
            v = float(pix) + (scale * sigma) * normal(h, 0)
            w = math.floor(v) if "floor_without_half" in brk else math.floor(v + 0.5)
            o.append(int(w) if 1.0 <= w <= 65535.0 else 0)
            if detail is not None:
                detail.append((idx, u, v + 0.5))
        out.append(o)
    return out, tick if "tick_not_advanced" in brk else tick + 1


def scan(points, origin, count, s, tick, par, active=1, brk=(), detail=None):
    """frp_nmpc_sensor_noise_scan for scan s: points [P][3] -> (out [P][3], tick); storage at index >= count is returned as it is.
    detail: a list that receives (index, u) of every point that drew."""
    out = [[float(v) for v in p] for p in points]
    if not active:
        return out, tick
    hs = sample_key(par["seed"], par["id0"] + s, tick, TAG_SCAN, brk)
    o = [float(v) for v in origin]
    s0, s1, p_drop = par["scan_sigma0"], par["scan_sigma1"], par["scan_p_drop"]
    for idx, p in enumerate(out):
        if idx >= count and "count_ignored" not in brk:
            break
        if not all(math.isfinite(v) for v in p):
            continue
        d = [p[i] - o[i] for i in range(3)]
        r = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        if not (r > 0.0 and math.isfinite(r)):
            continue
        h = mix((hs + idx) & MASK)
        u = uniform(h, 2)
        if detail is not None:
            detail.append((idx, u))
        if u < p_drop:
            out[idx] = [NAN, NAN, NAN]
            continue
        e = (s0 + s1 * r) * normal(h, 0)
        if e != 0.0:
            g = 1.0 + e / r
            out[idx] = [o[i] + d[i] * g for i in range(3)]
    return out, tick if "tick_not_advanced" in brk else tick + 1
