"""The synthetic cases of the mission (include/frp_nmpc.h section 17) that tests/test_mission_cpu.py and tests/test_gpu_mission.py share: for
each case the parameters, and a scripted world that answers every step the way a fleet would -- the goal callback takes an issued goal,
and a fixed script per vehicle lets go of targets near and far from the end point, moves an end point, loses the odometry, poisons a
position -- so that CALLS consecutive calls walk every branch of the step.  run() plays a case through tests/mission_oracle.py and returns
every call's inputs and the arrays expected after it; the script of a vehicle depends on its global id (id0 + b) alone, so a fleet and
its halves see the same world."""
import functools

import numpy as np

from . import mission_oracle as MO
from . import occmap_oracle as OO

CALLS = 8
T0, PERIOD, DT = 3.25, 0.05, 0.01
SEED = 20240918          # chosen on the CPU: every vehicle of random_r4_open that may fly gets a goal within its first four candidates

# the map of the random cases: 40 x 40 x 20 voxels of 0.1 m, a pillar and a solid block
MAP_ORIGIN, MAP_SIZE, MAP_RES = (-2.0, -2.0, 0.0), (4.0, 4.0, 2.0), 0.1
OPEN_BOX = (-1.4, 1.4, -1.4, 0.45)         # free but for the pillar: the inflated body (0.4 m) reaches neither the block nor the faces
WALLED_BOX = (-1.0, 1.0, 1.2, 1.7)         # inside the solid block y in [1.0, 2.0)
EDGE_BOX = (2.5, 6.0, -1.0, 1.0)           # beyond the map's x = 2 face: every probe is outside the map


def map_points():
    pts = []
    pts += [(0.25, -0.45, z) for z in np.arange(0.05, 2.0, 0.1)]
    pts += [(x, y, z) for x in np.arange(-1.95, 2.0, 0.1) for y in np.arange(1.05, 2.0, 0.1) for z in np.arange(0.05, 2.0, 0.1)]
    return np.array(pts, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def map_oracle():
    m = OO.OccMapOracle(MAP_ORIGIN, MAP_SIZE, MAP_RES)
    m.insert_cloud(map_points())
    return m


def _route(gid, W):
    """Waypoints of vehicle gid: a small polygon of its own."""
    x0, y0 = -1.0 + 0.125 * (gid % 17), -0.75 + 0.0625 * (gid % 23)
    return [[x0 + 0.5 * k, y0 + 0.25 * (k % 2), 1.0 + 0.125 * k] for k in range(W)]


def _route_len(gid, W):
    """Mostly W; some shorter; gid % 13 == 4: 0 and gid % 13 == 9: W + 1 -- the per-vehicle refusals."""
    r = gid % 13
    return 0 if r == 4 else W + 1 if r == 9 else 1 + (gid % W)


# name -> (mode arguments, uses the map)
CASES = {
    "route_w1": (dict(W=1, loop=False, dwell=0.0, leg_timeout=0.0, arrive_radius=0.25), False),
    "route_w3": (dict(W=3, loop=False, dwell=0.1, leg_timeout=0.075, arrive_radius=0.25), False),
    "route_w3_loop": (dict(W=3, loop=True, dwell=0.0, leg_timeout=0.0, arrive_radius=0.5), False),
    "random_r1": (dict(R=1, goal_box=OPEN_BOX, min_dist=0.5, max_dist=1.75, dwell=0.0, leg_timeout=0.075, arrive_radius=0.25), False),
    "random_r4": (dict(R=4, goal_box=OPEN_BOX, min_dist=0.5, max_dist=1.75, dwell=0.05, leg_timeout=0.0, arrive_radius=0.25), False),
    "random_r1_open": (dict(R=1, goal_box=OPEN_BOX, min_dist=0.25, max_dist=3.0, dwell=0.0, leg_timeout=0.0, arrive_radius=0.25), True),
    "random_r4_open": (dict(R=4, goal_box=OPEN_BOX, min_dist=0.25, max_dist=3.0, dwell=0.0, leg_timeout=0.0, arrive_radius=0.25), True),
    "random_r4_walled": (dict(R=4, goal_box=WALLED_BOX, min_dist=0.0, max_dist=10.0, dwell=0.0, leg_timeout=0.0, arrive_radius=0.25), True),
    "random_r4_edge": (dict(R=4, goal_box=EDGE_BOX, min_dist=0.0, max_dist=10.0, dwell=0.0, leg_timeout=0.0, arrive_radius=0.25), True),
}
SIZES = (1, 5, 260)      # one wave; a partly filled workgroup; more than one workgroup (65 workgroups of four waves)


def case_params(name, B, id0=0, R=None):
    a, with_map = CASES[name]
    a = dict(a)
    W = a.pop("W", 0)
    if R is not None and "R" in a:
        a["R"] = R
    if W:
        a["route"] = [_route(id0 + b, W) for b in range(B)]
        a["route_len"] = [_route_len(id0 + b, W) for b in range(B)]
    return MO.params(seed=SEED, id0=id0, **a), (map_oracle() if with_map else None)


def start_pos(gid):
    return [-1.25 + 0.03125 * (gid % 64), -1.0 + 0.0625 * (gid % 19), 1.2]


class World:
    """What the state machine and the vehicle of one mission vehicle show the step: have_odom, have_target, end_pt, pos."""

    def __init__(self, gid):
        self.gid, self.have_odom, self.have_target = gid, 0 if gid % 7 == 3 else 1, 0
        self.end_pt, self.pos = [0.0, 0.0, 0.0], start_pos(gid)

    def after_step(self, v, n):
        """The rest of period n: the goal callback, then this vehicle's script."""
        gid = self.gid
        self.have_target, self.end_pt = MO.goal_callback(self.have_target, self.end_pt, v["goal"], v["fresh"])
        if n >= 1:
            self.have_odom = 1                                  # the odometry of gid % 7 == 3 arrives after two calls
        e = (3 * gid + n) % 5
        if self.have_target and e == 0:                         # arrives: inside the radius, off the end point
            self.pos = [self.end_pt[0] + 0.125, self.end_pt[1] - 0.0625, self.end_pt[2] + 0.03125]
            self.have_target = 0
        elif self.have_target and e == 2:                       # dropped: the target is gone a metre from the end point
            self.pos = [self.end_pt[0] - 1.0, self.end_pt[1], self.end_pt[2]]
            self.have_target = 0
        elif self.have_target and e == 4 and gid % 4 == 1:      # the safety search moved the end point, the vehicle arrives THERE
            self.end_pt = [self.end_pt[0] + 0.75, self.end_pt[1] + 0.25, 1.4]
            self.pos = [self.end_pt[0], self.end_pt[1], self.end_pt[2] - 0.125]
            self.have_target = 0
        elif self.have_target:                                  # under way
            self.pos = [0.5 * (self.pos[0] + self.end_pt[0]), 0.5 * (self.pos[1] + self.end_pt[1]), self.pos[2]]
        if gid % 11 == 5 and n == 3:                            # a poisoned position: never `reached`, never within [min_dist, max_dist]
            self.pos = [float("nan"), self.pos[1], self.pos[2]]
        if gid % 11 == 5 and n == 5:
            self.pos = start_pos(gid)


def clock(k, n=3):
    return MO.clock(k, T0, PERIOD, DT, n)


@functools.lru_cache(maxsize=None)
def run(name, B, id0=0, R=None, calls=CALLS):
    """A case played through the oracle.  Returns (par, frames, met): frames[n] = (inputs, expected) of call n with inputs = dict(now,
    have_odom [B], have_target [B], end_pt [B,3], state [B,9]) and expected = dict of every state array and output after the call; met =
    the branches taken."""
    par, occ = case_params(name, B, id0, R)
    vs = [MO.new_vehicle() for _ in range(B)]
    ws = [World(id0 + b) for b in range(B)]
    frames, met = [], set()
    for n in range(calls):
        now = clock(n)[0]
        state = np.zeros((B, 9))
        state[:, 0:3] = [w.pos for w in ws]
        state[:, 3:] = 0.5                                      # (not read)
        inputs = dict(now=now, have_odom=np.array([w.have_odom for w in ws], dtype=np.int32), have_target=np.array([w.have_target for w in ws], dtype=np.int32),
                      end_pt=np.array([w.end_pt for w in ws], dtype=np.float64), state=state)
        for b, (v, w) in enumerate(zip(vs, ws)):
            met |= MO.step(v, par, b, now, w.have_odom, w.have_target, w.end_pt, w.pos, occ)
        frames.append((inputs, arrays(vs)))
        for v, w in zip(vs, ws):
            w.after_step(v, n)
    return par, frames, met


def arrays(vs):
    out = {n: np.array([v[n] for v in vs], dtype=np.int32) for n in MO.INT_FIELDS}
    out.update({n: np.array([v[n] for v in vs], dtype=np.float64) for n in MO.F64_FIELDS})
    return out


BRANCHES = ("done:leaves", "flying:reached", "flying:leg_time_max", "flying:dropped", "flying:abandoned", "flying:on_time", "idle:dwell", "idle:no_odom",
            "route:bad_len", "route:done", "route:wrap", "route:issue", "random:distance", "random:occupied", "random:issue", "random:issue_later", "random:blocked")
