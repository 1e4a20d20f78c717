"""The cases of the fleet peers (include/frp_nmpc.h section 18): seeded flights of B vehicles in the 18 x 12 x 5 m hall for the separation
record, and seeded scenes on the 40 x 40 x 20 map for the peer cloud.  Everything here is data: positions, masks, plans, boxes."""
import numpy as np

from . import peers_oracle as PO

R, D_WARN, D_HIT = 1.0, 0.5, 0.25
HALL_LO, HALL_HI = (-9.0, -6.0, 0.0), (9.0, 6.0, 5.0)
# the same hall under four grids: cell = R, cell = 3 R, and two other origins / dims
GRIDS = dict(unit=dict(origin=(-9.0, -6.0, 0.0), dims=(18, 12, 5), cell=1.0), coarse=dict(origin=(-9.0, -6.0, 0.0), dims=(6, 4, 2), cell=3.0),
             shifted=dict(origin=(-10.5, -7.25, -1.0), dims=(21, 15, 7), cell=1.0), wide=dict(origin=(-12.0, -8.0, -0.5), dims=(16, 11, 5), cell=1.5))
SIZES = (1, 2, 5, 70, 260)
CALLS = 3
CASES = ("clusters", "dense", "edges")


def flight(name, B, S, calls=CALLS, seed=0):
    """[(pos [B,S,3] f64, active [B] uint8 or None)] * calls.  clusters: a few groups about R wide that drift; dense: everybody in a
    1.5 m cube (many peers, ties among coincident vehicles); edges: the same with NaN and infinite coordinates, vehicles outside the box,
    inactive vehicles, coincident vehicles and vehicles on cell faces and corners."""
    rng = np.random.default_rng([seed, B, S, CASES.index(name)])
    lo, hi = np.array(HALL_LO), np.array(HALL_HI)
    n_c = max(1, B // 6)
    centre = lo + 1.5 + rng.random((n_c, 3)) * (hi - lo - 3.0)
    group = rng.integers(0, n_c, size=B)
    spread = 0.6 if name == "clusters" else 0.75
    if name != "clusters":
        centre[:] = np.array([1.0, -2.0, 2.0])
    p = centre[group] + (rng.random((B, 3)) - 0.5) * 2.0 * spread
    vel = (rng.random((B, 3)) - 0.5) * 0.2
    out = []
    for c in range(calls):
        pos = np.zeros((B, S, 3))
        for s in range(S):
            p = p + vel
            pos[:, s] = p
        pos = np.clip(pos, lo + 0.01, hi - 0.01)
        active = None
        if name in ("dense", "edges") and B >= 5:
            pos[1] = pos[0]                                   # coincident: d2 = 0, the lowest id wins
            pos[4] = pos[0]
        if name == "edges":
            pos[:] = np.round(pos * 4.0) / 4.0                # quarter metres: cell faces, corners, exact ties
            active = np.ones((B,), dtype=np.uint8)
            if B >= 5:
                pos[2, S - 1, 1] = np.nan
                pos[3, 0] = (50.0, 0.0, 1.0)                  # outside the box
                active[4] = 0 if c == 1 else 1
            if B >= 70:
                pos[10, :, 0] = np.inf
                pos[11, :, 2] = -3.0
                pos[12] = (1.0e300, -1.0e300, 1.0e300)        # far away: the quotient is beyond int
                pos[20] = (1.0, -2.0, 2.0); pos[21] = (2.0, -2.0, 2.0); pos[22] = (1.0, -1.0, 3.0)   # exactly R apart across a face; a corner
                active[30:34] = 0
        out.append((pos, active))
    return out


def replay(frames, grid, B, count=None):
    """The oracle over a flight: the arrays after every call, [(rec copy, outside [B] int32, tick)]."""
    rec, tick, out = PO.new_record(B, R), 0, []
    for pos, active in frames:
        ent = PO.entered(pos, grid["origin"], grid["dims"], grid["cell"], active, count)
        tick = PO.separation(rec, pos, ent, R, D_WARN, D_HIT, tick, 1, count)
        out.append(({k: v.copy() for k, v in rec.items()}, (~ent.all(axis=1)).astype(np.int32), tick))
    return out


# ---- the peer cloud: the 40 x 40 x 20 map of the mission's and the safety checks' tests ----
MAP_ORIGIN, MAP_SIZE, MAP_RES = (-2.0, -2.0, 0.0), (4.0, 4.0, 2.0), 0.1
MAP_POINTS = np.array([[0.05, 0.05, 0.55], [0.35, -0.25, 0.75], [-0.55, 0.45, 1.05], [1.05, 1.05, 0.35], [-1.25, -0.95, 1.45]])
CLOUD_GRID = dict(origin=(-2.0, -2.0, 0.0), dims=(8, 8, 4), cell=0.5)
CLOUD_R = 0.5
N_PLAN = 20


def cloud_scene(name, B, seed=0):
    """dict(state [B,9], pre_plan [B,N,17], have_traj [B], stages, r_body) of a named scene; the planners sit in the map's middle."""
    rng = np.random.default_rng([seed, B, len(name)])
    state = np.zeros((B, 9))
    state[:, :3] = np.array([0.0, 0.0, 1.0]) + (rng.random((B, 3)) - 0.5) * (0.6 if B <= 70 else 1.6)
    if name == "crowd":                                       # everybody within R of planner 0: 65, 70 or more peers of it
        state[:, :3] = np.array([0.0, 0.0, 1.0]) + (rng.random((B, 3)) - 0.5) * 0.3
        state[0, :3] = (0.0, 0.0, 1.0)
    pre_plan = rng.random((B, N_PLAN, 17))
    for k in range(N_PLAN):
        pre_plan[:, k, 8:11] = state[:, :3] + 0.03 * (k + 1) * (rng.random((B, 3)) - 0.3)
    have_traj = (rng.random(B) < 0.6).astype(np.int32)
    if B >= 2:
        have_traj[0], have_traj[1] = 1, 0
    if B >= 5:
        pre_plan[2, 3, 9] = np.nan                            # a non-finite point of a plan
        state[3, :3] = state[2, :3]                           # a tie in d2 for everybody else
    if name == "k3" and B >= 5:
        state[4, 2] = np.nan                                  # a planner that is not entered: no peers, nobody's peer
    stages = dict(k0=(), k8=(0, 2, 3, 5, 8, 12, 16, 19), k3=(3, 9, 19), crowd=(1,), alone=(3,))[name]
    r_body = dict(k0=0.2, k8=0.15, k3=0.0, crowd=0.0, alone=0.2)[name]
    if name == "alone":                                       # nobody within R of anybody
        state[:, 0] = -1.9 + 0.6 * (np.arange(B) % 6); state[:, 1] = -1.9 + 0.6 * ((np.arange(B) // 6) % 6); state[:, 2] = 0.2 + 0.6 * (np.arange(B) // 36)
    return dict(state=state, pre_plan=pre_plan, have_traj=have_traj, stages=stages, r_body=r_body)


CLOUD_CASES = ("k0", "k8", "k3", "crowd")
