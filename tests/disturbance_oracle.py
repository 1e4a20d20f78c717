"""Executable statement of the disturbance model (include/frp_nmpc.h section 15): the TRUE mass-normalised force on a vehicle as a function of
its position, its time and a per-vehicle seeded stream.  NO reference counterpart -- the reference flies RotorS with a hand-driven wrench
(README.md:111-117).  Python floats (IEEE doubles), one rounding per operation, written in the order the device code is written in; the
integers are Python's, reduced mod 2^64 where the device's wrap.

Vehicle b keeps a sample counter tick.  For sample k = tick, at the plant's position p BEFORE the sample:
    t = t_epoch + float(k) * dt
    acc = base
    for every zone, in index order:    acc += w(p, t) * F          (w = 0 included)
    for every event, in index order:   if t_on <= t < t_off:  acc += F
    with gusts:                        g <- a o g + c o n(seed, id0 + b, k);  acc += g
CHOSEN, not derived: the force is held over the sample (zero-order hold), a zone's edge is a linear ramp, the gust an OU process."""
import math

MAX_ZONES, MAX_EVENTS, ZONE_STRIDE, EVENT_STRIDE = 16, 8, 12, 5
MASK = (1 << 64) - 1
U1_DIV = 9007199254740993.0    # written as 2^53 + 1 (distributed.monte_carlo_fext's literal); the double it denotes is 2^53: u1 in (0, 1]
U2_DIV = 9007199254740992.0    # 2^53: u2 in [0, 1)
TWO_PI = 6.283185307179586

# the branches sample() reports, for the tests that count them
ZONE_OFF, ZONE_OUT, ZONE_RAMP, ZONE_FULL, EVENT_ON, EVENT_OFF, GUST = "zone_off", "zone_out", "zone_ramp", "zone_full", "event_on", "event_off", "gust"


def mix(x):
    """The SplitMix64 finaliser, distributed._splitmix64's constants, on an unsigned 64-bit integer."""
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def stream_key(seed, ident, k):
    return mix((mix((mix(seed & MASK) + ident) & MASK) + k) & MASK)


def uniforms(seed, ident, k, axis):
    """(u1, u2) of one normal: u1 in (0, 1], u2 in [0, 1); both quotients are exact."""
    h = stream_key(seed, ident & MASK, k & MASK)
    r0, r1 = mix((h + 2 * axis) & MASK), mix((h + 2 * axis + 1) & MASK)
    return float((r0 >> 11) + 1) / U1_DIV, float(r1 >> 11) / U2_DIV


def normal(seed, ident, k, axis):
    u1, u2 = uniforms(seed, ident, k, axis)
    return math.sqrt(-2.0 * math.log(u1)) * math.cos(TWO_PI * u2)


def zone_weight(row, p, t):
    """(w, branch) of one zone row [12] at position p [3] and time t."""
    if not (row[10] <= t and t < row[11]):
        return 0.0, ZONE_OFF
    d = [p[i] - row[i] for i in range(3)] + [row[3 + i] - p[i] for i in range(3)]
    if not all(v >= 0.0 for v in d):              # (a NaN fails the comparison)
        return 0.0, ZONE_OUT
    m = d[0]
    for v in d[1:]:
        m = v if v < m else m
    ramp = row[9]
    return (1.0, ZONE_FULL) if m >= ramp else (m / ramp, ZONE_RAMP)


def time_of(k, t_epoch, dt):
    return t_epoch + float(k) * dt


def sample(p, k, b, base, zones, events, g, gust_a, gust_c, seed, id0, t_epoch, dt, branches=None):
    """One sample of vehicle b: (force [3], g [3]).  zones [Z][12]; events [E][5], the vehicle's own; g None: no gusts, nothing drawn.
    branches: a list that receives the branch names taken, or None."""
    t = time_of(k, t_epoch, dt)
    p = [float(v) for v in p]
    acc = [float(v) for v in base]
    note = branches.append if branches is not None else (lambda n: None)
    for row in zones:
        row = [float(v) for v in row]
        w, br = zone_weight(row, p, t)
        note(br)
        for i in range(3):
            acc[i] = acc[i] + w * row[6 + i]
    for row in events:
        row = [float(v) for v in row]
        if row[0] <= t and t < row[1]:
            note(EVENT_ON)
            for i in range(3):
                acc[i] = acc[i] + row[2 + i]
        else:
            note(EVENT_OFF)
    if g is not None:
        note(GUST)
        g = [float(v) for v in g]
        for i in range(3):
            g[i] = gust_a[i] * g[i] + gust_c[i] * normal(seed, id0 + b, k, i)
            acc[i] = acc[i] + g[i]
    return acc, g


def evaluate(pos, tick, b, base, zones, events, g, gust_a, gust_c, seed, id0, t_epoch, dt, branches=None):
    """frp_nmpc_disturbance_eval for one vehicle: S = len(pos) samples.  Returns (force [S][3], g, tick + S): what advance != 0 leaves; a
    pure query keeps the g and the tick it was given."""
    out = []
    for s in range(len(pos)):
        f, g = sample(pos[s], tick + s, b, base, zones, events, g, gust_a, gust_c, seed, id0, t_epoch, dt, branches)
        out.append(f)
    return out, g, tick + len(pos)


def reset(g, tick, mask=1):
    """frp_nmpc_disturbance_reset for one vehicle: (g, tick)."""
    if not mask:
        return g, tick
    return (None if g is None else [0.0, 0.0, 0.0]), 0


def gust_coefficients(sigma, tau, dt):
    """(a [3], c [3]) as solver.Disturbance computes them on the host."""
    a = [math.exp(-dt / u) for u in tau]
    return a, [s * math.sqrt(1.0 - v * v) for s, v in zip(sigma, a)]


def fly(x, hold, base, cmd, kind, tick, b, zones, events, gust, gust_a, gust_c, seed, id0, t_epoch, **kw):
    """frp_nmpc_vehicle_step_field for one vehicle through tests/vehicle_oracle.py: per sample the force at the position before it, then one
    S = 1 step under that force.  Returns (x, hold, trace, sat, force [S][3], gust, tick); gust is the OU state (None: no gusts; `g` is the vehicle's gravity, among kw)."""
    from . import vehicle_oracle as VO
    dt = kw.get("dt_cmd", 0.01)
    trace, sats, forces = [], [], []
    for s in range(len(kind)):
        f, gust = sample(x[0:3], tick + s, b, base, zones, events, gust, gust_a, gust_c, seed, id0, t_epoch, dt)
        x, hold, tr, sa = VO.step(x, hold, f, [cmd[s]], [kind[s]], **kw)
        trace.append(tr[0]); sats.append(sa[0]); forces.append(f)
    return x, hold, trace, sats, forces, gust, tick + len(kind)
