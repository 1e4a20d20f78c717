"""Case table of the stage references (frp_nmpc_reference_batch = getCurTraj + calculate_yaw) and of the mode switch
(frp_nmpc_mode_batch = switch_to_final).  Pure numpy and Python floats, no transcendental function: every number below is the same
double on every machine, so tests/golden/reference_mp.npz (tests/tools/gen_reference_mp.py) belongs to exactly these inputs.
Imported by tests/test_reference_cpu.py, tests/test_gpu_reference.py and the generator.

Stage references: `cases()` -> list of Case, each one planner (its path, size, offset, plan row 1) with a `family`; `launches()` groups
them into launches of B <= 64, one per (N, Ts, K, shared / per-planner) group, every case at blockIdx > 0 at least once;
`census()` counts, FROM THE ORACLE ALONE, how often each branch the families aim at is really taken.
Mode switch: `mode_groups()` -> launches with the expectation left to oracle.mode_one; MODE_TABLE is the hand-worked table mode_one
itself is checked against.

The kernel's own rules that the table relies on (frp_reference.hip): kino_size is clamped to [1, K]; a stage whose quotient
(i Ts + off) / Ts is <= -1, >= 2**31 - 1 or not finite gets the end of the path.
"""
import math

import numpy as np

TS_ALL = (0.05, 0.1, 0.02, 0.03)
N_ALL = (1, 2, 20, 63, 64)
PI = 3.1415926
NO_SIZE = -999          # "kino_size absent" in integer arrays
COS_A, SIN_A = 0.9968017063026194, 0.07991469396917269   # cos, sin of 0.08: literals, so that no libm decides the table


class Case:
    __slots__ = ("name", "family", "N", "Ts", "K", "path_id", "size", "off", "pos1", "yaw0", "shared", "index")

    def __init__(self, name, family, N, Ts, path_id, off, pos1=None, yaw0=0.0, size=None, shared=False):
        self.name, self.family, self.N, self.Ts, self.path_id, self.off, self.size, self.shared = name, family, N, Ts, path_id, float(off), size, shared
        self.K = len(PATHS[path_id])
        self.pos1 = np.array(PATHS[path_id][0] if pos1 is None else pos1, dtype=float)
        self.yaw0 = float(yaw0)
        self.index = -1

    @property
    def path(self):
        return PATHS[self.path_id]

    @property
    def eff_size(self):
        """The kernel's clamp of kino_size (frp_reference.hip): absent -> K, then to [1, K]."""
        s = self.K if self.size is None else self.size
        return max(1, min(s, self.K))

    def plan(self):
        p = np.zeros((self.N + 1, 17))
        p[1, 8:11] = self.pos1
        p[1, 16] = self.yaw0
        return p


PATHS = {}


def _reg(pid, rows):
    PATHS[pid] = np.array(rows, dtype=float).reshape(-1, 3)
    PATHS[pid].setflags(write=False)
    return pid


def spiral(K, radius=2.0, sign=1.0, centre=(0.0, 0.0, 1.0), dz=0.01):
    """K samples on a helix, 0.08 rad per sample (5 samples ahead: 0.8 m at radius 2), by a rotation recurrence of multiplies and adds
    only.  Starts at angle 0, so the direction of travel crosses +-pi after about 17 samples."""
    x, y, rows = radius, 0.0, []
    for k in range(K):
        rows.append((centre[0] + x, centre[1] + y, centre[2] + dz * k))
        x, y = COS_A * x - sign * SIN_A * y, sign * SIN_A * x + COS_A * y
    return rows


def line(K, step, start=(0.0, 0.0, 1.0)):
    return [(start[0] + step[0] * k, start[1] + step[1] * k, start[2] + step[2] * k) for k in range(K)]


def ulp_up(x):
    return float(np.nextafter(x, np.inf))


def ulp_down(x):
    return float(np.nextafter(x, -np.inf))


def direction_distinct(path, min_move=1e-3):
    """The property the on-grid and end-of-path cases lean on: reading sample ki + 4 or ki + 6 instead of ki + 5, or starting from sample
    ki - 1 or ki + 1 instead of ki, turns the look-ahead direction by more than min_move / 0.8, so ref_yaw (0.8 of it) moves by more
    than min_move.  Checked for the interpolation weights 0, 1/2 and 1."""
    path = np.asarray(path)
    K = len(path)

    def ang(pos, j):
        d = path[min(j, K - 1)] - pos
        return math.atan2(d[1], d[0])

    def wrap(a):
        return abs((a + math.pi) % (2 * math.pi) - math.pi)
    worst = math.inf
    for k in range(1, K - 7):
        for w in (0.0, 0.5, 1.0):
            pos = path[k] + w * (path[k + 1] - path[k])
            base = ang(pos, k + 5)
            worst = min(worst, wrap(ang(pos, k + 4) - base), wrap(ang(pos, k + 6) - base))
            for k2 in (k - 1, k + 1):
                pos2 = path[k2] + w * (path[k2 + 1] - path[k2])
                worst = min(worst, wrap(ang(pos2, k2 + 5) - base))
    return 0.8 * worst > min_move, 0.8 * worst


# ---- the paths -----------------------------------------------------------------------------------------------------------------
K_GRID = 48
_reg("grid", spiral(K_GRID))
_reg("grid_cw", spiral(K_GRID, sign=-1.0))
_reg("k40", spiral(40))
_reg("k30", spiral(30))
_reg("k30_cw", spiral(30, sign=-1.0, centre=(0.3, -0.2, 1.5)))
_reg("k80", spiral(80, radius=3.0))
_reg("k1", [(0.5, -0.25, 1.25)])
_reg("big", spiral(30, radius=1000.0, centre=(-250.0, 125.0, 500.0), dz=3.0))
_reg("far_small", spiral(30, radius=2.0, centre=(1000.0, -1000.0, 999.0)))
_reg("tiny", spiral(30, radius=1.0 / 1024, centre=(0.0, 0.0, 1.0 / 1024), dz=1.0 / 65536))
_reg("straight", line(40, (0.06, 0.08, 0.0)))                          # 0.1 m per sample along (0.6, 0.8)
_reg("hold_release", [(0.015 * k if k < 9 else 0.12 + 0.05 * (k - 8), 0.0 if k < 9 else -0.03 * (k - 8), 1.0) for k in range(24)])
_reg("jump", [(0.0, 0.0, 1.0)] + [(5.0 + 0.1 * k, 0.25, 1.0) for k in range(1, 12)])
_reg("hover", [(0.25, 0.5, 1.0)] * 12)

U1 = (1.0, 0.0, 0.0)
U3 = (2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0)                                 # unit to within rounding; margins are taken from the 50-digit norm
REL = (1e-9, -1e-9, 1e-3, -1e-3)


def _ahead(pid, d):
    """Samples 0-4 at the origin, samples 5-11 at d: stages 0-4 at offset 0 stand at the origin and look at d."""
    return _reg(pid, [(0.0, 0.0, 0.0)] * 5 + [tuple(d)] * 7)


for _u, _un in ((U1, "1"), (U3, "3")):
    for _r in REL:
        _ahead("dir%s_%+g" % (_un, _r), [0.1 * (1.0 + _r) * c for c in _u])
_ahead("dir_exact", (0.1, 0.0, 0.0))                                    # sqrt(fl(0.1 * 0.1)) is the double 0.1 again: exactly ON the threshold
_reg("origin", [(0.0, 0.0, 0.0)] * 12)
# unwrap: look-ahead at angle atan2(+-0.8, -0.6) = +-2.2142974355881810 rad from the origin, 0.5 m away
_ahead("turn_up", (-0.3, 0.4, 0.0))
_ahead("turn_dn", (-0.3, -0.4, 0.0))
THETA = 2.214297435588181                                               # atan2(0.8, -0.6), a literal; the generator measures the real margins
_reg("held_then_turn", [(0.0, 0.0, 0.0)] * 6 + [(-0.3, -0.4, 0.0)] * 6)  # stage 0 held, stage 1 sees the direction -THETA


def _build():
    out = []

    def add(*a, **k):
        out.append(Case(*a, **k))

    # on-grid offsets: off = k Ts, one ulp below and above, k = 0 .. K + 3; one shared path, size absent
    for Ts in TS_ALL:
        pid = "grid" if Ts in (0.05, 0.02) else "grid_cw"
        for k in range(K_GRID + 4):
            g = k * Ts
            for tag, off in (("", g), ("-", ulp_down(g)), ("+", ulp_up(g))):
                add("grid%s_%g_%d" % (tag, Ts, k), "grid" if tag == "" else "grid_ulp", 20, Ts, pid, off, pos1=(9.0, 9.0, 9.0), yaw0=1.7 if pid == "grid" else -1.7,
                    shared=True)
    for Ts in TS_ALL:
        s = "%g" % Ts
        # negative offsets
        for tag, off in (("in", -0.3 * Ts), ("near", -0.999 * Ts), ("ulp_in", ulp_up(-Ts)), ("at", -Ts), ("past", ulp_down(-Ts)), ("far", -3.7 * Ts)):
            add("neg_%s_%s" % (tag, s), "negative", 20, Ts, "k30", off, yaw0=1.5)
        # non-finite and huge offsets
        for tag, off in (("nan", math.nan), ("+inf", math.inf), ("-inf", -math.inf), ("2^31", 2.0 ** 31 * Ts), ("2^32+3", (2.0 ** 32 + 3) * Ts), ("1e300", 1e300),
                         ("2^31-2", (2.0 ** 31 - 2) * Ts), ("-1e300", -1e300)):
            add("hostile_%s_%s" % (tag, s), "hostile", 20, Ts, "k40", off, yaw0=0.4)
        # end of path: runs that start inside and end past it
        for m in range(4, 31):
            add("end_%s_%d" % (s, m), "end", 20, Ts, "k30", (m + 0.3) * Ts, yaw0=2.0)
        add("end_cw_%s" % s, "end", 20, Ts, "k30_cw", 14.6 * Ts, yaw0=-2.0)
        # path sizes, per-planner sizes that differ within a launch
        for size in (20, 30, 37, 1, 0, -5, 12):
            for off in (0.3 * Ts, 12.3 * Ts):
                add("size%d_%s_%g" % (size, s, off / Ts), "size", 20, Ts, "k30", off, size=size, yaw0=1.0)
    for size in (None, 17):                                             # a shared path with one size, and with none
        for j in range(6):
            add("shared_%s_%d" % (size, j), "size_shared", 20, 0.05, "k30_cw", (3 * j + 0.4) * 0.05, size=size, yaw0=-1.0, shared=True)
    for N in N_ALL:                                                     # every horizon; K == 1; K == 80
        Ts = TS_ALL[N % 4]
        add("k1_N%d" % N, "k1", N, Ts, "k1", 0.4 * Ts, pos1=(0.5, -0.25, 2.0))
        add("k1s_N%d" % N, "k1", N, Ts, "k1", 0.0, size=1, pos1=(0.5, 0.85, 1.25))
        for off in (0.25 * Ts, 30.5 * Ts, -0.5 * Ts):
            add("k80_N%d_%g" % (N, off / Ts), "horizon", N, Ts, "k80", off, yaw0=1.6)
            add("k80s_N%d_%g" % (N, off / Ts), "horizon", N, Ts, "k80", off, size=70, yaw0=-1.6)
    # direction threshold: distance 0.1 (1 +- 1e-9), 0.1 (1 +- 1e-3), from one component and from three; hover; hold, then release
    for un in "13":
        for r in REL:
            add("dir%s_%+g" % (un, r), "direction", 2, 0.05, "dir%s_%+g" % (un, r), 0.0, yaw0=0.7)
    # exactly 0.1: '>' holds the yaw, '>=' would turn it.  The one family with a zero margin: the distance IS the double 0.1 in exact
    # arithmetic, and a correctly rounded sqrt of the rounded square returns it (a theorem of binary floating point)
    add("dir_exact", "direction_exact", 2, 0.05, "dir_exact", 0.0, yaw0=0.7)
    add("hover", "direction", 20, 0.1, "hover", 0.03, yaw0=-2.5)
    for Ts in TS_ALL:
        add("hold_release_%g" % Ts, "hold", 20, Ts, "hold_release", 0.5 * Ts, yaw0=0.9)
    # unwrap: D = yaw_temp - last_yaw just above +PI, just below -PI, inside (PI, pi) on both signs, |D| < PI on both signs
    for tag, delta in (("above", PI + 2e-9), ("band", 3.14159263), ("below", PI - 2e-9), ("pi+", 3.1415927)):
        add("unwrap+_%s" % tag, "unwrap", 2, 0.05, "turn_up", 0.0, yaw0=THETA - delta)      # D = +delta, yaw_temp > 0
        add("unwrap-_%s" % tag, "unwrap", 2, 0.05, "turn_dn", 0.0, yaw0=-THETA + delta)     # D = -delta, yaw_temp < 0
    add("unwrap_after_hold", "unwrap_held", 3, 0.05, "held_then_turn", 0.0, yaw0=3.0)
    for Ts in TS_ALL:                                                   # seeds at +-3.1 and outside [-pi, pi]
        for y0 in (3.1, -3.1, 7.0, -9.5):
            add("seed_%g_%g" % (Ts, y0), "seed", 20, Ts, "k30" if y0 > 0 else "k30_cw", 1.5 * Ts, yaw0=y0)
    # replan flag: distance 1 (1 +- 1e-9), 1 (1 +- 1e-3); stage 0 near and stage 1 far; the reverse
    for u, un in ((U1, "1"), (U3, "3")):
        for r in REL:
            add("replan%s_%+g" % (un, r), "replan", 2, 0.05, "origin", 0.0, pos1=[(1.0 + r) * c for c in u])
    add("replan_stage0_near", "replan_stage0", 2, 0.05, "jump", 0.0, pos1=(0.0, 0.5, 1.0))
    add("replan_stage0_far", "replan_stage0", 2, 0.05, "jump", 0.0, pos1=(5.1, 0.25, 1.0))
    # coordinates: 1e3 m and 1e-3 m
    for Ts in TS_ALL:
        for pid in ("big", "far_small", "tiny"):
            for off in (0.37 * Ts, 7.73 * Ts):
                add("coord_%s_%g_%g" % (pid, Ts, off / Ts), "coord", 20, Ts, pid, off, yaw0=1.2)
    # closed form: the straight path of tests/test_oracle.py at every Ts
    for Ts in TS_ALL:
        add("straight_%g" % Ts, "straight", 20, Ts, "straight", 2.5 * Ts, yaw0=-0.4)
    for i, c in enumerate(out):
        c.index = i
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


class Launch:
    """One kernel launch: planners = the cases of `members` in order (a case may appear twice), one (N, Ts, K)."""

    def __init__(self, members):
        c0 = members[0]
        self.members, self.N, self.Ts, self.K, self.shared = members, c0.N, c0.Ts, c0.K, c0.shared
        self.B = len(members)
        self.path = c0.path.copy() if self.shared else np.stack([c.path for c in members])
        if c0.size is None:
            self.kino_size = None
        else:
            self.kino_size = np.array([c0.size] if self.shared else [c.size for c in members], dtype=np.int32)
        self.off = np.array([c.off for c in members])
        self.plans = np.stack([c.plan() for c in members])


def launches(case_list=None, chunk=63):
    """Groups of at most `chunk` cases with one (N, Ts, K, shared / per-planner, size absent or not) -- for a shared path also one path
    and one size -- each launched with its first case repeated behind the last: every case runs at blockIdx > 0."""
    groups = {}
    for c in (cases() if case_list is None else case_list):
        key = (c.N, c.Ts, c.K, c.shared, c.size is None) + ((c.path_id, c.size) if c.shared else ())
        groups.setdefault(key, []).append(c)
    out = []
    for key in sorted(groups, key=repr):
        g = groups[key]
        for s in range(0, len(g), chunk):
            part = g[s:s + chunk]
            out.append(Launch(part + part[:1]))
    return out


def oracle_case(R, c):
    """oracle.reference_oracle.references_one on a case, under the kernel's clamp of kino_size."""
    return R.references_one(c.path, c.eff_size, c.off, c.plan(), c.N, c.Ts)


def stage_quotients(c):
    """(index_time, quotient) per stage, as IEEE double operations (Python floats)."""
    it = [i * c.Ts + c.off for i in range(c.N)]
    return it, [t / c.Ts for t in it]


def in_range(q):
    return q == q and -1.0 < q < 2.0 ** 31 - 1.0


def census(R):
    """Counts per branch, from the oracle's own arithmetic (no kernel, no fixture).  Every count has to be positive; the two on-grid
    counts at least 50 per Ts."""
    n = {}

    def hit(key, k=1):
        n[key] = n.get(key, 0) + k
    for key in ("ki+1==size-1", "ki+1==size", "ki+5==size-1", "ki+5==size", "inside_then_past", "negative_weight", "hostile_stage", "hostile_then_in_range",
                "far", "held", "held_then_released", "unwrap_minus", "unwrap_plus", "unwrap_after_held", "band+", "band-", "no_unwrap+", "no_unwrap-",
                "replan", "no_replan", "replan_stage0_only_near", "replan_stage0_only_far", "size_absent", "size<K", "size==K", "size>K", "size==1", "size==0",
                "size<0", "K==1", "per_planner_sizes_differ", "shared_one_size", "coord>=1e3", "coord<=1e-3") + tuple("N==%d" % N for N in N_ALL):
        n[key] = 0
    for Ts in TS_ALL:
        n["grid_below_%g" % Ts] = n["grid_equal_%g" % Ts] = 0
    for c in cases():
        it, q = stage_quotients(c)
        size = c.eff_size
        hit("N==%d" % c.N)
        if c.family == "grid":
            k = int(c.name.rsplit("_", 1)[1])
            for i in range(c.N):
                if i + k < size:                                        # the side decides a sample that exists
                    t = int(q[i])
                    assert t in (i + k, i + k - 1), (c.name, i, q[i])
                    hit(("grid_below_%g" if t < i + k else "grid_equal_%g") % c.Ts)
        ok = [in_range(x) for x in q]
        ki = [int(x) if o else None for x, o in zip(q, ok)]
        hit("hostile_stage", sum(not o for o in ok))
        if not ok[0] and any(ok):
            hit("hostile_then_in_range")
        for i, k in enumerate(ki):
            if k is None:
                continue
            for d in (1, 5):
                hit("ki+%d==size-1" % d, k + d == size - 1)
                hit("ki+%d==size" % d, k + d == size)
            if k + 1 < size and math.fmod(it[i], c.Ts) < 0:
                hit("negative_weight")
        if ki[0] is not None and ki[-1] is not None and ki[0] + 1 < size <= ki[-1] + 1:
            hit("inside_then_past")
        pos, yaw, replan = oracle_case(R, c)
        last, held_before, branches = c.yaw0, False, []
        for i in range(c.N):                                            # the oracle's decisions, re-derived from what it returned
            k = ki[i]
            fwd = c.path[k + 5] if k is not None and k + 5 < size else c.path[size - 1]
            d = fwd - pos[i]
            far = np.linalg.norm(d) > 0.1
            yt = math.atan2(d[1], d[0]) if far else last
            D = yt - last
            br = ("far" if far else "held", "unwrap_minus" if D > PI else "unwrap_plus" if D < -PI else "none")
            branches.append(br)
            hit(br[0])
            if br[1] != "none":
                hit(br[1])
                hit("unwrap_after_held", held_before)
            elif far:
                hit("no_unwrap+", D > 0); hit("no_unwrap-", D < 0)
            hit("band+", PI < D < math.pi); hit("band-", -math.pi < D < -PI)
            hit("held_then_released", far and held_before)
            held_before = not far
            last = yaw[i]
        hit("replan" if replan else "no_replan")
        if c.family == "replan_stage0":
            hit("replan_stage0_only_far" if replan else "replan_stage0_only_near")
        s = c.size
        hit("size_absent", s is None)
        if s is not None:
            hit("size<K", 1 < s < c.K); hit("size==K", s == c.K and c.K > 1); hit("size>K", s > c.K); hit("size==1", s == 1); hit("size==0", s == 0); hit("size<0", s < 0)
        hit("K==1", c.K == 1)
        hit("coord>=1e3", float(np.max(np.abs(c.path))) >= 1e3)
        hit("coord<=1e-3", c.family == "coord" and float(np.max(np.abs(c.path))) <= 2e-3)
    for L in launches():
        if L.kino_size is not None:
            hit("per_planner_sizes_differ", (not L.shared) and len(set(L.kino_size.tolist())) > 1)
            hit("shared_one_size", L.shared)
    return {k: int(v) for k, v in n.items()}


# ---- mode switch ---------------------------------------------------------------------------------------------------------------
MODE_NORMAL, MODE_FINAL = 0, 1
MODE_N = (2, 20, 64)
MODE_TS = (0.05, 0.1, 0.03)
MODE_RADIUS = (1.0, 0.25)
MODE_B = (1, 255, 256, 257, 600)
CANARY = -7777

# hand-worked rows for mode_one: (N, Ts, radius, time_offset, kino_size, plan stage N-1 position, end_pt, switches, why)
# 0.05 and 0.1 are slightly ABOVE 1/20 and 1/10 as doubles, 0.03 slightly below 3/100; the rows marked * were worked through with exact
# fractions of those doubles (tests/test_reference_cpu.py re-derives their quotients with fractions.Fraction).
FAR = (50.0, 0.0, 0.0)
MODE_TABLE = [
    (20, 0.05, 1.0, 0.0, 21, FAR, (0, 0, 0), False, "max_index 20 < 21, 50 m away"),
    (20, 0.05, 1.0, 0.0, 20, FAR, (0, 0, 0), True, "max_index 20 == kino_size"),
    (20, 0.05, 1.0, 0.0, 19, FAR, (0, 0, 0), True, "max_index 20 > 19"),
    (20, 0.05, 1.0, 0.024, 21, FAR, (0, 0, 0), False, "(1 + 0.024) / 0.05 = 20.48 -> 20"),
    (20, 0.05, 1.0, 0.05, 21, FAR, (0, 0, 0), True, "* (1 + 0.05) / 0.05 = 21 exactly in doubles -> 21 == kino_size"),
    (20, 0.05, 1.0, 0.049, 21, FAR, (0, 0, 0), False, "20.98 -> 20"),
    (2, 0.1, 1.0, 0.25, 4, FAR, (0, 0, 0), True, "(0.2 + 0.25) / 0.1 = 4.5 -> 4 == kino_size"),
    (2, 0.1, 1.0, 0.15, 4, FAR, (0, 0, 0), False, "3.5 -> 3"),
    (64, 0.03, 0.25, 0.5, 81, FAR, (0, 0, 0), False, "(1.92 + 0.5) / 0.03 = 80.67 -> 80"),
    (64, 0.03, 0.25, 0.5, 80, FAR, (0, 0, 0), True, "80 == kino_size"),
    (20, 0.05, 1.0, -2.0, 5, FAR, (0, 0, 0), False, "(1 - 2) / 0.05 = -20: negative max_index, positive size"),
    (20, 0.05, 1.0, -2.0, 0, FAR, (0, 0, 0), False, "-20 < 0"),
    (20, 0.05, 1.0, -2.0, -20, FAR, (0, 0, 0), True, "* -1 / 0.05 = -20 exactly (the double 0.05 is above 1/20: -19.99.. rounds to -20) == kino_size -20"),
    (20, 0.05, 1.0, 0.0, 0, FAR, (0, 0, 0), True, "empty path: 20 >= 0"),
    (20, 0.05, 1.0, 0.0, 100, (0.0, 0.6, 0.0), (0, 0, 0), True, "0.6 m < 1.0"),
    (20, 0.05, 0.25, 0.0, 100, (0.0, 0.6, 0.0), (0, 0, 0), False, "0.6 m >= 0.25"),
    (20, 0.05, 1.0, 0.0, 100, (1.0, 0.0, 0.0), (0, 0, 0), False, "distance == radius: '<' is strict"),
    (20, 0.05, 1.0, 0.0, 100, (3.0, 4.0, 13.0), (3.0, 4.0, 12.0 + 2.0 ** -49), True, "1 - 2^-49 < 1"),
    (20, 0.05, 5.0, 0.0, 100, (3.0, 4.0, 0.0), (0, 0, 0), False, "3-4-5 triangle: exactly 5, not below"),
    (20, 0.05, 1.0, math.inf, 100, FAR, (0, 0, 0), True, "+inf saturates to INT_MAX"),
    (20, 0.05, 1.0, 1e300, 2 ** 31 - 1, FAR, (0, 0, 0), True, "INT_MAX >= INT_MAX"),
    (20, 0.05, 1.0, -math.inf, -100, FAR, (0, 0, 0), False, "-inf saturates to INT_MIN < -100"),
    (20, 0.05, 1.0, -1e300, -2 ** 31, FAR, (0, 0, 0), True, "INT_MIN >= INT_MIN"),
    (20, 0.05, 1.0, math.nan, 1, FAR, (0, 0, 0), False, "NaN converts to 0 < 1"),
    (20, 0.05, 1.0, math.nan, 0, FAR, (0, 0, 0), True, "NaN converts to 0 >= 0"),
    (20, 0.05, 1.0, math.nan, 100, (0.5, 0.0, 0.0), (0, 0, 0), True, "NaN offset, but 0.5 m from the goal"),
]


class ModeGroup:
    """One launch of frp_nmpc_mode_batch: plans [B,N+1,17], off [B], sizes [B] or [1], end_pt [B,3] or [3], mode_in [B]."""

    def __init__(self, N, Ts, radius, B, size_per, end_per, seed, shared_size=30):
        rng = np.random.default_rng(seed)
        self.N, self.Ts, self.radius, self.B, self.size_per, self.end_per = N, Ts, radius, B, size_per, end_per
        S = shared_size                                                 # the shared size
        self.sizes = np.full(B, S, dtype=np.int32) if size_per else np.array([S], dtype=np.int32)
        self.end_pt = rng.integers(-8, 9, (B, 3)).astype(float) if end_per else np.array([2.0, -1.0, 1.0])
        self.off = np.zeros(B)
        self.plans = rng.normal(0, 1, (B, N + 1, 17))
        self.plans[:, :, 8:11] += 40.0                                  # every stage far from every goal, until a row says otherwise
        self.mode_in = np.zeros(B, dtype=np.int32)
        unit = (U1, U3, (0.0, -1.0, 0.0))
        for b in range(B):
            r = (b * 7 + seed) % 29
            size = S
            if size_per:
                size = (S, S + 1, S - 1, 0, -3, 1, 2 ** 31 - 1, -2 ** 31)[(b // 29 + b) % 8]
                self.sizes[b] = size
            s = min(max(size, -100), 200)
            if r < 9:                                                   # max_index == size, one below, one above: on the grid, the truncation decides
                g = (s - N + (r % 3) - 1) * Ts
                self.off[b] = (g, ulp_down(g), ulp_up(g))[r // 3]
            elif r < 13:                                                # distance radius (1 +- 1e-9), (1 +- 1e-3); index far below the size
                self.off[b] = -(N + 150) * Ts
                e = self.end_pt[b] if end_per else self.end_pt
                self.plans[b, N - 1, 8:11] = e + radius * (1.0 + REL[r - 9]) * np.array(unit[b % 3])
            elif r < 15:                                                # negative offset, max_index < 0
                self.off[b] = -(N + 3 + r) * Ts
            elif r < 22:
                self.off[b] = (math.nan, math.inf, -math.inf, 2.0 ** 31 * Ts, (2.0 ** 32 + 3) * Ts, 1e300, -1e300)[r - 15]
            elif r < 24:                                                # already FINAL stays FINAL whatever the rule says
                self.off[b] = -(N + 150) * Ts
                self.mode_in[b] = MODE_FINAL
            else:
                self.off[b] = float(rng.uniform(-2, 3)) + (s - N) * Ts

    def expect(self, R):
        out = self.mode_in.copy()
        for b in range(self.B):
            size = int(self.sizes[b if self.size_per else 0])
            e = self.end_pt[b] if self.end_per else self.end_pt
            if R.mode_one(self.plans[b], self.off[b], size, e, self.N, self.Ts, self.radius):
                out[b] = MODE_FINAL
        return out


def mode_groups():
    out, seed = [], 0
    for N, Ts, radius in zip(MODE_N, MODE_TS, (1.0, 0.25, 1.0)):
        for B in MODE_B:
            seed += 1
            out.append(ModeGroup(N, Ts, radius, B, seed % 2, (seed // 2) % 2, seed))
    for size_per in (0, 1):                                             # both flags both ways at one shape, and the other radius / Ts pairings
        for end_per in (0, 1):
            seed += 1
            out.append(ModeGroup(20, 0.05, 0.25, 257, size_per, end_per, seed))
            out.append(ModeGroup(2, 0.03, 1.0, 64, size_per, end_per, seed + 100))
    for shared_size in (0, -3):                                         # kino_size[0] read at 0 and at a negative value
        seed += 1
        out.append(ModeGroup(20, 0.05, 1.0, 64, 0, seed % 2, seed, shared_size=shared_size))
    return out
