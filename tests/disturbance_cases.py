"""Shared inputs of the disturbance tests (tests/test_disturbance_cpu.py, tests/test_gpu_disturbance.py, tests/tools/gen_disturbance_mp.py): the
scene list of the multiprecision fixture, built without random numbers, the same arrays on every run.  Only numpy and math: no device, no
oracle.

A SCENE is what one launch shares: the zone table, E, the gust coefficients, seed, id0, t_epoch.  A CASE of a scene is one vehicle and
S_MAX = 5 samples: its lane b, pos [5][3], tick0, events [E][5], base [3], g0 [3] -- and `expect`, the branches its five samples are BUILT
to take, per sample a tuple of one name per zone followed by one per event.  The generator and the CPU test hold the oracle to them, so a
case that misses the branch it was written for fails there.  An S = 1 run takes a case's first sample alone."""
import math

import numpy as np

S_MAX = 5
DT = 0.01
B_GPU = 257                       # lanes of a GPU launch: one workgroup plus one lane
OFF, OUT, RAMP, FULL, EV_ON, EV_OFF = "zone_off", "zone_out", "zone_ramp", "zone_full", "event_on", "event_off"   # disturbance_oracle's names
INF, NAN = float("inf"), float("nan")
UNUSED = [INF, INF, 0.0, 0.0, 0.0]          # an unused event slot

up = lambda v: math.nextafter(v, INF)
down = lambda v: math.nextafter(v, -INF)


def t_of(k, t_epoch):
    return t_epoch + float(k) * DT


# ---- scene "box": Z = 1, E = 1 -- every face of a ramped box, the ramp's two ends, both ends of the time window ----
BOX_EPOCH = 0.25
BOX = dict(lo=(-1.0, 0.5, 0.75), hi=(2.0, 1.5, 3.0), F=(1.5, -0.5, 0.25), ramp=0.25, k_on=40, k_off=90)


def _box_scene():
    z = BOX
    zone = list(z["lo"]) + list(z["hi"]) + list(z["F"]) + [z["ramp"], t_of(z["k_on"], BOX_EPOCH), t_of(z["k_off"], BOX_EPOCH)]
    mid = [0.5 * (z["lo"][i] + z["hi"][i]) for i in range(3)]
    cases = []
    ev_on = [t_of(10, BOX_EPOCH), INF, 0.125, 0.0, -0.25]        # on from tick 10 for ever
    for face in range(6):
        i, low = face % 3, face < 3
        wall = z["lo"][i] if low else z["hi"][i]
        inward = (lambda v: up(v)) if low else (lambda v: down(v))
        outward = (lambda v: down(v)) if low else (lambda v: up(v))
        at_ramp = wall + z["ramp"] if low else wall - z["ramp"]              # exact in these numbers: d == ramp
        coords = [wall, inward(wall), outward(wall), at_ramp, outward(at_ramp)]
        pos = [[c if j == i else mid[j] for j in range(3)] for c in coords]
        # d = 0 and d = one ulp are on the ramp (w = 0 and w tiny), outside feels nothing, d == ramp is full, just below it is not
        expect = [(RAMP, EV_ON), (RAMP, EV_ON), (OUT, EV_ON), (FULL, EV_ON), (RAMP, EV_ON)]
        cases.append(dict(pos=pos, tick0=50 + face, events=[ev_on], base=[0.25 * face, -0.5, 0.0], expect=expect))
    # the time window: t == t_on is inside, t == t_off is outside; the event's own window ends exactly at a sample
    centre = [[0.5, 1.0, 2.0]] * 5
    cases.append(dict(pos=centre, tick0=z["k_on"] - 1, events=[[t_of(z["k_on"] + 1, BOX_EPOCH), t_of(z["k_on"] + 3, BOX_EPOCH), 1.0, 2.0, 3.0]], base=[0.0, 0.0, 0.0],
                      expect=[(OFF, EV_OFF), (FULL, EV_OFF), (FULL, EV_ON), (FULL, EV_ON), (FULL, EV_OFF)]))
    cases.append(dict(pos=centre, tick0=z["k_off"] - 2, events=[UNUSED], base=[1.0, 1.0, 1.0],
                      expect=[(FULL, EV_OFF), (FULL, EV_OFF), (OFF, EV_OFF), (OFF, EV_OFF), (OFF, EV_OFF)]))
    # positions that are not finite feel no zone (the window is open)
    bad = [[NAN, 1.0, 2.0], [0.5, INF, 2.0], [0.5, 1.0, -INF], [NAN, NAN, NAN], [0.5, 1.0, 2.0]]
    cases.append(dict(pos=bad, tick0=60, events=[ev_on], base=[0.5, 0.25, -0.125], expect=[(OUT, EV_ON)] * 4 + [(FULL, EV_ON)]))
    # an interior point of the ramp in every axis at once: the smallest difference decides
    cases.append(dict(pos=[[-0.9375, 0.625, 1.0], [1.9, 1.4375, 2.9], [0.0, 0.5625, 0.875], [1.875, 1.0, 2.9375], [-0.875, 1.375, 0.8125]], tick0=70,
                      events=[ev_on], base=[0.0, 0.0, 0.0], expect=[(RAMP, EV_ON)] * 5))
    return dict(name="box", zones=[zone], E=1, t_epoch=BOX_EPOCH, gust=None, seed=0, id0=0, cases=cases)


# ---- scene "many": Z = 16, E = 8 -- hard edges with closed faces, windows that never close, zones that never open, ticks across 2^31 ----
MANY_EPOCH = -1024.0
MANY_P = [0.5, -0.25, 1.5]
MANY_K = 2 ** 31 - 2


def _many_scene():
    zones, zexp = [], []
    for i in range(16):
        F = [0.0625 * (i + 1), -0.03125 * i, 0.125 * ((i % 3) - 1)]
        if i % 4 in (0, 2):        # a hard box with the vehicle ON a face (axis i % 3): closed faces, full weight
            lo, hi = [-2.0, -2.0, -2.0], [3.0, 3.0, 3.0]
            (lo if i % 4 == 0 else hi)[i % 3] = MANY_P[i % 3]
            zones.append(lo + hi + F + [0.0, -INF, INF]); zexp.append(FULL)
        elif i % 4 == 1:           # a box next to the vehicle
            zones.append([1.0, -2.0, -2.0, 3.0, 3.0, 3.0] + F + [0.5, -INF, INF]); zexp.append(OUT)
        else:                      # a box around it that never opens
            zones.append([-2.0, -2.0, -2.0, 3.0, 3.0, 3.0] + F + [0.5, INF, INF]); zexp.append(OFF)
    t = lambda k: t_of(k, MANY_EPOCH)
    k = MANY_K
    events = [[-INF, INF, 0.5, 0.0, 0.0], UNUSED, [t(k + 1), t(k + 3), 0.0, 0.25, 0.0], [t(k), t(k + 1), 0.0, 0.0, 1.0], [t(k + 4), INF, -2.0, 0.0, 0.0],
              [-INF, t(k + 2), 0.0, -0.75, 0.0], UNUSED, [t(k + 2), t(k + 2), 9.0, 9.0, 9.0]]         # (the last: an empty window)
    on = [(1, 0, 0, 1, 0, 1, 0, 0), (1, 0, 1, 0, 0, 1, 0, 0), (1, 0, 1, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 1, 0, 0, 0)]
    expect = [tuple(zexp) + tuple(EV_ON if v else EV_OFF for v in row) for row in on]
    cases = [dict(pos=[MANY_P] * 5, tick0=k, events=events, base=[0.0, 0.0, -0.5], expect=expect)]
    # the same vehicle one ulp off each face it sat on: zones 0, 2 ... lose it where the ulp points outward
    for axis in range(3):
        p_in = list(MANY_P); p_in[axis] = up(MANY_P[axis])
        p_out = list(MANY_P); p_out[axis] = down(MANY_P[axis])
        ex = []
        for p in (p_in, p_out, MANY_P, p_in, p_out):
            zz = []
            for i in range(16):
                if i % 4 in (0, 2) and i % 3 == axis and p is not MANY_P:
                    inside = (p is p_in) == (i % 4 == 0)      # lo faces keep what moved up, hi faces what moved down
                    zz.append(FULL if inside else OUT)
                else:
                    zz.append(zexp[i])
            ex.append(tuple(zz) + (EV_ON, EV_OFF) + (EV_OFF,) * 6)
        ev = [[-INF, INF, 0.5, 0.0, 0.0]] + [UNUSED] * 7
        cases.append(dict(pos=[p_in, p_out, MANY_P, p_in, p_out], tick0=7 + axis, events=ev, base=[0.0, 0.0, 0.0], expect=ex))
    return dict(name="many", zones=zones, E=8, t_epoch=MANY_EPOCH, gust=None, seed=0, id0=0, cases=cases)


# ---- scene "bare": Z = 0, E = 0 -- the force is the constant part ----
def _bare_scene():
    cases = [dict(pos=[[0.0, 0.0, 0.0]] * 5, tick0=0, events=[], base=[0.0, 0.0, 0.0], expect=[()] * 5),
             dict(pos=[[1.0, NAN, 2.0]] * 5, tick0=2 ** 40, events=[], base=[1.5, -2.25, 1e-300], expect=[()] * 5)]
    return dict(name="bare", zones=[], E=0, t_epoch=0.0, gust=None, seed=0, id0=0, cases=cases)


# ---- the gust scenes: the box scene and the bare scene once more with turbulence; lanes on both sides of the workgroup boundary ----
GUST_LANES = tuple(range(11)) + (255, 256)
GUST_SIGMA, GUST_TAU = (0.5, 0.3, 0.2), (0.5, 1.0, 0.25)


def _gusty(scene, name, seed, id0, tick_shift):
    src = scene["cases"]
    cases = []
    for j, lane in enumerate(GUST_LANES):
        c = dict(src[lane % len(src)])
        c["lane"] = lane
        c["tick0"] = c["tick0"] + tick_shift
        c["g0"] = [0.0, 0.0, 0.0] if j % 3 == 0 else [0.125 * j, -0.0625 * j, 0.03125 * (j - 5)]
        cases.append(c)
    return dict(scene, name=name, gust=dict(sigma=GUST_SIGMA, tau=GUST_TAU), seed=seed, id0=id0, cases=cases)


def gust_coefficients(sigma, tau, dt=DT):
    """solver.Disturbance's host computation, restated."""
    a = [math.exp(-dt / u) for u in tau]
    return a, [s * math.sqrt(1.0 - v * v) for s, v in zip(sigma, a)]


def scenes():
    box, many, bare = _box_scene(), _many_scene(), _bare_scene()
    for sc in (box, many, bare):
        for lane, c in enumerate(sc["cases"]):
            c["lane"] = lane
            c["g0"] = [0.0, 0.0, 0.0]
    # "box_gust": an ordinary stream.  "bare_gust": a negative seed, id0 + b crossing from -3 to 0 and on (the unsigned sum wraps), and the
    # second case's tick 2^40 moved to where the five samples cross 2^31
    return [box, many, bare, _gusty(box, "box_gust", 20261021, 1000, 0), _gusty(bare, "bare_gust", -7, -3, 0),
            _gusty(dict(bare, cases=[dict(bare["cases"][0], tick0=2 ** 31 - 3)]), "wrap_gust", 2 ** 63 - 1, -2 ** 63, 0)]


def arrays(sc):
    """A scene as the arrays the fixture stores and the GPU test uploads: zones [Z,12], lane [C], pos [C,5,3], tick0 [C] int64, events
    [C,E,5], base [C,3], g0 [C,3]."""
    C, E = len(sc["cases"]), sc["E"]
    return dict(zones=np.array(sc["zones"], dtype=np.float64).reshape(len(sc["zones"]), 12), lane=np.array([c["lane"] for c in sc["cases"]], dtype=np.int32),
                pos=np.array([c["pos"] for c in sc["cases"]], dtype=np.float64), tick0=np.array([c["tick0"] for c in sc["cases"]], dtype=np.int64),
                events=np.array([c["events"] for c in sc["cases"]], dtype=np.float64).reshape(C, E, 5),
                base=np.array([c["base"] for c in sc["cases"]], dtype=np.float64), g0=np.array([c["g0"] for c in sc["cases"]], dtype=np.float64))


# ---- the boundary: one good argument set, and every rule broken once ----
GOOD = dict(B=4, Z=2, E=1, t_epoch=0.0, dt=DT, gust_a=(0.5, 0.5, 0.5), gust_c=(0.1, 0.1, 0.1), seed=1, id0=0, zone=0x1000, event=0x2000, gust=0x3000, tick=0x4000)
BAD = [dict(B=0), dict(B=-1), dict(Z=-1), dict(Z=17), dict(E=-1), dict(E=9), dict(zone=None), dict(Z=0), dict(event=None), dict(E=0), dict(tick=None),
       dict(t_epoch=NAN), dict(t_epoch=INF), dict(dt=0.0), dict(dt=-DT), dict(dt=NAN), dict(dt=INF), dict(gust_a=(0.5, NAN, 0.5)), dict(gust_a=(1.5, 0.5, 0.5)),
       dict(gust_a=(0.5, 0.5, -0.1)), dict(gust_c=(0.1, -0.1, 0.1)), dict(gust_c=(0.1, 0.1, INF)), dict(gust_c=(NAN, 0.1, 0.1))]
GOOD_TOO = [dict(Z=0, zone=None), dict(E=0, event=None), dict(gust=None, gust_a=(NAN, NAN, NAN), gust_c=(-1.0, INF, NAN)), dict(Z=16, E=8), dict(gust_a=(0.0, 1.0, 0.5))]
