"""The mission of include/frp_nmpc.h section 17, stated in numpy float64 and Python integers, one vehicle at a time: what
frp_nmpc_mission_step, _clock and _reset do.  There is no reference counterpart (in the reference a person clicks goals in rviz and ROS
owns the time): THIS FILE IS THE STATEMENT, pinned by the hand-worked scenarios of tests/test_mission_cpu.py, and the device agrees with it
to the bit -- every operation below is an IEEE one on doubles (Python floats), written in the order the header gives, or integer
arithmetic modulo 2^64.  checkPosSurround is tests/occmap_check_oracle.py's.

A vehicle is a dict of Python numbers (new_vehicle()); step() changes it in place and returns the names of the branches it took, which
the CPU test counts."""
from . import occmap_check_oracle as CO
from .disturbance_oracle import mix, stream_key

IDLE, FLYING, DONE = 0, 1, 2
TAG = 0x4D495353                        # "MISS"
M64 = (1 << 64) - 1
INT_FIELDS = ("phase", "leg", "tries", "issued", "reached", "dropped", "abandoned", "blocked", "fresh")
F64_FIELDS = ("t_mark", "leg_time_sum", "leg_time_max", "goal")


def new_vehicle():
    return dict(phase=IDLE, leg=-1, tries=0, t_mark=0.0, issued=0, reached=0, dropped=0, abandoned=0, blocked=0, leg_time_sum=0.0, leg_time_max=0.0,
                goal=[0.0, 0.0, 0.0], fresh=0)


def params(route=None, route_len=None, loop=False, goal_box=None, z_goal=1.2, min_dist=0.0, max_dist=1.0e6, R=0, inflate_ratio=1.2, arrive_radius=0.3,
           dwell=0.0, leg_timeout=0.0, seed=0, id0=0):
    """route: [B][W][3] nested lists (route mode) or None; goal_box (random mode) or None."""
    return dict(route=route, route_len=route_len, loop=bool(loop), goal_box=goal_box, z_goal=float(z_goal), min_dist=float(min_dist), max_dist=float(max_dist),
                R=int(R), inflate_ratio=float(inflate_ratio), arrive_radius=float(arrive_radius), dwell=float(dwell), leg_timeout=float(leg_timeout),
                seed=int(seed), id0=int(id0))


def uniform(h, j):
    """u(h, j) in [0, 1): section 16's; the quotient is exact."""
    return float(mix((h + j) & M64) >> 11) / 9007199254740992.0


def key(seed, ident, leg):
    return mix((stream_key(seed & M64, ident & M64, leg & M64) + TAG) & M64)


def candidate(par, b, leg, c):
    """Candidate c of leg `leg` of vehicle b: (x, y).  A function of (seed, id0 + b, leg, c) alone."""
    h = key(par["seed"], par["id0"] + b, leg)
    lo_x, hi_x, lo_y, hi_y = (float(v) for v in par["goal_box"])
    x = lo_x + uniform(h, 2 * c) * (hi_x - lo_x)
    y = lo_y + uniform(h, 2 * c + 1) * (hi_y - lo_y)
    return x, y


def step(v, par, b, now, have_odom, have_target, end_pt, pos, occ=None, body=(CO.EGO_R, CO.EGO_H)):
    """One frp_nmpc_mission_step for vehicle b.  end_pt, pos: three floats each (the state machine's end point; the odometry position).
    occ: a tests/occmap_oracle.OccMapOracle or None.  Returns the set of branch names taken."""
    met = set()
    now = float(now)
    v["fresh"] = 0
    due = False
    if v["phase"] not in (IDLE, FLYING):
        met.add("done:leaves")
        return met
    if v["phase"] == FLYING:
        if have_target == 0:
            dx, dy, dz = float(pos[0]) - float(end_pt[0]), float(pos[1]) - float(end_pt[1]), float(pos[2]) - float(end_pt[2])
            d2 = (dx * dx + dy * dy) + dz * dz
            if d2 <= par["arrive_radius"] * par["arrive_radius"]:
                lt = now - v["t_mark"]
                v["reached"] += 1
                v["leg_time_sum"] = v["leg_time_sum"] + lt
                if v["leg_time_max"] < lt:
                    v["leg_time_max"] = lt
                    met.add("flying:leg_time_max")
                met.add("flying:reached")
            else:
                v["dropped"] += 1
                met.add("flying:dropped")
            v["phase"], v["t_mark"] = IDLE, now
        elif par["leg_timeout"] > 0.0 and now - v["t_mark"] > par["leg_timeout"]:
            v["abandoned"] += 1
            v["phase"], v["t_mark"] = IDLE, now - par["dwell"]
            due = True
            met.add("flying:abandoned")
        else:
            met.add("flying:on_time")
    if v["phase"] != IDLE:
        return met
    if not (due or now - v["t_mark"] >= par["dwell"]):
        met.add("idle:dwell")
        return met
    if have_odom == 0:
        met.add("idle:no_odom")
        return met
    j = v["leg"] + 1
    point = None
    if par["route"] is not None:
        W = len(par["route"][b])
        n = int(par["route_len"][b])
        if n < 1 or n > W:
            v["phase"] = DONE
            met.add("route:bad_len")
        elif j < 0 or (not par["loop"] and j >= n):
            v["phase"] = DONE
            met.add("route:done")
        else:
            idx = j % n if par["loop"] else j
            if par["loop"] and j >= n:
                met.add("route:wrap")
            point = [float(u) for u in par["route"][b][idx]]
            met.add("route:issue")
    else:
        px, py = float(pos[0]), float(pos[1])
        min2, max2 = par["min_dist"] * par["min_dist"], par["max_dist"] * par["max_dist"]
        for i in range(par["R"]):
            c = v["tries"] + i
            x, y = candidate(par, b, j, c)
            dx, dy = x - px, y - py
            d2 = dx * dx + dy * dy
            if not (d2 >= min2 and d2 <= max2):
                met.add("random:distance")
                continue
            if occ is not None and not CO.check_pos_surround(occ, [x, y, par["z_goal"]], par["inflate_ratio"], None, body):
                met.add("random:occupied")
                continue
            point = [x, y, par["z_goal"]]
            met.add("random:issue" if c == 0 else "random:issue_later")
            break
        if point is None:
            v["blocked"] += 1
            v["tries"] += par["R"]
            met.add("random:blocked")
    if point is not None:
        v["leg"], v["tries"] = j, 0
        v["issued"] += 1
        v["phase"], v["t_mark"] = FLYING, now
        v["goal"], v["fresh"] = point, 1
    return met


def clock(k, t0, period, dt, n):
    """frp_nmpc_mission_clock's values for the counter k."""
    base = float(t0) + float(k) * float(period)
    return [base + float(dt) * float(j) for j in range(n)]


def reset(v):
    v.clear()
    v.update(new_vehicle())


def goal_callback(have_target, end_pt, goal, fresh):
    """goalCallback (NM:481-493) as far as the mission reads it back: (have_target, end_pt) afterwards."""
    if fresh and not goal[2] < -0.1:
        return 1, [goal[0], goal[1], 1.2]
    return have_target, end_pt
