"""The case table of the kinodynamic A*'s kernel routes (csrc/frp_astar.hip), shared by tests/test_astar_paths_cpu.py (no device: every
case really takes the route it is named after) and tests/test_gpu_astar_paths.py (the device against the oracle on that route).

workloads.astar_world at its defaults always takes ONE route through the kernel: the bit-packed map (grid z <= 64), the integer
cell -> voxel offset (`fast`), a staged window of radius 22 (below the clamp of 31), the eight-duration first expansion, no local box,
a pool that never runs out, K above every sample count, end_vel = start_acc = 0, everything far from the map's border.  Each case
below leaves that route by one switch.  A case is a list of RUNS -- two or three seeded worlds with B = 4 planners each --:

    dict(world, q, init, K, local_box [B,6] int32 or None, allocate_num or None, prior)

allocate_num, when given, is the pool of the plan under test, `prior` says that the device planner plans once with the world's own
pool first (so that a NO_PATH afterwards has a path to keep).  The switch conditions are restated here in Python from the kernel's
host code and formulas; nothing here imports the oracle except oracle_of() and the pool-exhaustion builder, which sizes its pool
from the oracle's own node counts."""
import math

import numpy as np

from forces_resilient_planner_amd import workloads

B = 4
WIN = 64                      # frp_astar.hip: window of staged occupancy columns
WIN_R_MAX = (WIN - 1) // 2    # ... and the clamp of its radius
CELL_SAFE = 4096              # ... and the range of ray cells the integer offset is verified for
POOL = 12000

STATUS_REACH_HORIZON, STATUS_REACH_END, STATUS_NO_PATH, STATUS_SHOT_FAILS = 1, 2, 3, 4


# ------------------------------------------------------------------ the switch conditions, restated from the kernel's host code
def fast_axis(origin_i, res):
    """The host loop of frp_nmpc_astar_batch for one axis: True when floor(((c res + res / 2) - origin) (1 / res)) == c + off for
    every ray cell |c| <= CELL_SAFE, off being that expression at c = 0.  (Python floats are IEEE doubles, evaluated without
    contraction: the same operations.)"""
    res_inv = 1.0 / res
    off = math.floor(((0.0 * res + res / 2.0) - origin_i) * res_inv)
    for c in range(-CELL_SAFE, CELL_SAFE + 1):
        if math.floor(((float(c) * res + res / 2.0) - origin_i) * res_inv) != c + off:
            return False
    return True


def fast_flag(world):
    return all(fast_axis(world["origin"][i], world["resolution"]) for i in range(3))


def win_r_wanted(world, f_ext_row):
    """The radius astar_kernel asks for before it clamps it to WIN_R_MAX: reach of a primitive per axis + the inflated ego radius, in
    cells, plus two."""
    tau = max(world["max_tau"], world["init_max_tau"])
    fm = max(abs(f_ext_row[0]), abs(f_ext_row[1]))
    reach = world["max_vel"] * tau + 0.5 * (world["max_acc"] + fm) * tau * tau + 1.5 * world["ego_r"]
    return int(math.ceil(reach / world["resolution"])) + 2


def grid_z(world):
    return world["occ"].shape[2]


# ------------------------------------------------------------------ builders
def _run(world, q, init=True, K=2048, local_box=None, allocate_num=None, prior=False):
    return dict(world=world, q=q, init=init, K=K, local_box=local_box, allocate_num=allocate_num, prior=prior)


def _world(seed, kind, **kw):
    kw.setdefault("allocate_num", POOL)
    kw.setdefault("n_obstacles", 30)
    return workloads.astar_world(seed, kind, **kw)


KINDS = ("pillars", "wall_gap", "pillars")


def byte_map():
    return [_run(_world(300 + i, KINDS[i], map_size=(20.0, 20.0, 8.0), origin=(-10.0, -10.0, -4.0)), workloads.astar_queries(B, 300 + i)) for i in range(2)]


def fast_off():
    """x, then y, then both shifted by half a voxel.  map_size stays 20: the last 5 cm before +10 are outside the grid and read -1."""
    org = [(-10.05, -10.0, -1.0), (-10.0, -10.05, -1.0), (-10.05, -10.05, -1.0)]
    return [_run(_world(310 + i, KINDS[i], origin=org[i]), workloads.astar_queries(B, 310 + i)) for i in range(3)]


def byte_map_fast_off():
    org = [(-10.05, -10.0, -4.0), (-10.0, -10.05, -4.0)]
    return [_run(_world(320 + i, KINDS[i], map_size=(20.0, 20.0, 8.0), origin=org[i]), workloads.astar_queries(B, 320 + i)) for i in range(2)]


def clamp_tau():
    return [_run(_world(330 + i, KINDS[i], max_tau=0.8), workloads.astar_queries(B, 330 + i)) for i in range(2)]


def clamp_res():
    """Resolution 0.05 with grid z = 60 <= 64: the packed map, a window that wants 42 columns either way."""
    runs = []
    for i in range(2):
        w = _world(340 + i, KINDS[i], resolution=0.05, map_size=(20.0, 20.0, 3.0), origin=(-10.0, -10.0, -1.5))
        q = workloads.astar_queries(B, 340 + i, goal_dist=(3.0, 7.0))
        q["start_pt"][:, 2] = np.clip(q["start_pt"][:, 2], 0.3, 1.3); q["end_pt"][:, 2] = np.clip(q["end_pt"][:, 2], 0.3, 1.3)
        runs.append(_run(w, q))
    return runs


def init_false():
    runs = [_run(_world(350 + i, KINDS[i]), workloads.astar_queries(B, 350 + i), init=False) for i in range(2)]
    # one planner starts inside a pillar: NO_PATH without a retry
    w, q = runs[0]["world"], runs[0]["q"]
    ix, iy, iz = np.argwhere(w["occ"][:, :, 15:25] > 0)[0]
    q["start_pt"][3] = np.array(w["origin"]) + (np.array([ix, iy, iz + 15]) + 0.5) * w["resolution"]
    return runs


def _to_idx(w, p, i):
    return int(np.floor((p - w["origin"][i]) / w["resolution"]))


def local_box():
    """Boxes of the occupancy map's local view (tests/occmap_oracle.py) with a radius shorter than the searches; in the first world
    planner 3 gets a hand-made box instead that cuts a pillar across its path in half: the half at y >= 0 reads as free."""
    from . import occmap_oracle as OO
    runs = []
    for i in range(2):
        w = _world(360 + i, "pillars", n_obstacles=25)
        q = workloads.astar_queries(B, 360 + i)
        om = OO.OccMapOracle(w["origin"], w["map_size"], w["resolution"], local_radius=(4.0, 4.0, 3.0))
        box = np.array([om.local_box(x) for x in q["start_pt"]], dtype=np.int32)
        if i == 0:
            occ = w["occ"]
            occ[_to_idx(w, -1.2, 0):_to_idx(w, -0.6, 0) + 1, _to_idx(w, -1.5, 1):_to_idx(w, 1.5, 1) + 1, :] = 1
            q["start_pt"][3] = (-4.0, 0.55, 1.0); q["end_pt"][3] = (2.5, 0.55, 1.0); q["start_v"][3] = 0.0; q["f_ext"][3] = 0.0
            gx, gy, gz = occ.shape
            box[3] = (0, 0, 0, gx, _to_idx(w, -0.05, 1), gz)
        runs.append(_run(w, q, local_box=box))
    return runs


def without_box(run):
    r = dict(run)
    r["local_box"] = None
    return r


def pool_exhaustion():
    """allocate_num from the oracle's own node counts of an unconstrained run (pool 12000): U1[b] nodes with the continuous start
    (init), U2[b] from the full primitive set (what the retry runs).  A search whose unconstrained run creates U nodes runs out of a
    pool of A <= U.  The pool is chosen so that one planner's first search AND its retry run out (A <= min(U1, U2)) and another's first
    search runs out while its retry fits (U2 < A <= U1)."""
    from . import astar_lib as AL
    runs = []
    for seed in range(370, 400):
        w = _world(seed, "pillars")
        q = workloads.astar_queries(B, seed)
        o1 = AL.plan_batch(w, q["start_pt"], q["start_v"], q["start_a"], q["end_pt"], q["end_v"], q["f_ext"], init=True, nthreads=4)
        o2 = AL.plan_batch(w, q["start_pt"], q["start_v"], q["start_a"], q["end_pt"], q["end_v"], q["f_ext"], init=False, nthreads=4)
        ok = [b for b in range(B) if o1["retried"][b] == 0 and o1["status"][b] != STATUS_NO_PATH and o2["status"][b] != STATUS_NO_PATH]
        U1 = {b: o1["results"][b].use_node_num for b in ok}; U2 = {b: o2["results"][b].use_node_num for b in ok}
        best = None
        for y in ok:            # the planner whose retry succeeds
            A = U2[y] + 1       # the smallest pool its retry still fits
            for x in ok:        # the planner whose retry runs out as well
                if x != y and A <= U1[y] and A <= min(U1[x], U2[x]) and A >= 64 and (best is None or A < best[0]):
                    best = (A, x, y)
        if best is None:
            continue
        r = _run(w, q, allocate_num=best[0], prior=True)
        r["both_out"], r["retry_fits"] = best[1], best[2]
        runs.append(r)
        if len(runs) == 2:
            break
    assert len(runs) == 2
    return runs


def truncation():
    """K = 32 (every path is longer) and K = exactly the sample count of one planner of the world (found by the CPU test / set by
    exact_K below from the oracle's untruncated count)."""
    runs = [_run(_world(380 + i, KINDS[i]), workloads.astar_queries(B, 380 + i, goal_dist=(3.0, 12.0)), K=32) for i in range(2)]
    # an empty world, starts two primitives short of the goal's neighbourhood: 22 samples of search, and the SHOT crosses K = 32
    a = lambda *rows: np.asarray(rows, dtype=float)
    z = np.zeros((B, 3))
    q = dict(start_pt=a((-1.5, 0.05, 1.05), (-1.2, 0.05, 1.05), (-1.0, 0.05, 1.05), (-1.5, -2.0, 1.05)), start_v=a((0, 0, 0), (0, 0, 0), (0, 0, 0), (1.0, 0, 0)),
             start_a=z.copy(), end_pt=a((0.6, 0.05, 1.05), (0.6, 0.05, 1.05), (0.6, 0.05, 1.05), (0.6, -2.0, 1.05)), end_v=z.copy(), f_ext=z.copy())
    runs.append(_run(_world(0, "empty"), q, K=32))
    return runs


def exact_K(run, counts, status):
    """The same run with K = the smallest untruncated sample count among the planners that found a path."""
    r = dict(run)
    r["K"] = int(min(int(n) for n, s in zip(counts, status) if s != STATUS_NO_PATH))
    return r


def end_vel_start_acc():
    runs = []
    for i in range(3):
        w = _world(390 + i, KINDS[i])
        q = workloads.astar_queries(B, 390 + i, goal_dist=(2.0, 12.0))
        rng = np.random.default_rng(3900 + i)
        q["end_v"] = rng.uniform(-1.0, 1.0, (B, 3)); q["start_a"] = rng.uniform(-2.0, 2.0, (B, 3))
        runs.append(_run(w, q))
    return runs


def map_border():
    """Starts and goals within 0.3 m of an x / y bound and z within 0.15 of the floor of the range (0.1): the staged window hangs over
    the grid's edge, the ego cross reaches cells outside the map (-1: not free) and in_range rejects primitives.  The inflated ego
    cross of a planner at rest reaches 1.5 ego_r / sqrt(2) = 0.2864 m along x and y, so planners 0, 1 and 3 start 0.288 .. 0.3 m
    from one bound and head for a goal at the opposite bound, across the map (REACH_HORIZON on the way); planner 2 starts in a
    corner, within reach of both bounds, and can only fail."""
    runs = []
    for i in range(2):
        w = _world(400 + i, ("empty", "pillars")[i])
        rng = np.random.default_rng(4000 + i)
        u = lambda lo, hi: float(rng.uniform(lo, hi))
        near, far = (lambda: 10.0 - u(0.288, 0.3)), (lambda: 10.0 - u(0.05, 0.3))
        start = np.array([(-near(), u(-6.0, 6.0), 0.0), (u(-4.0, 4.0), -near(), 0.0), (-far(), far(), 0.0), (near(), u(-6.0, 6.0), 0.0)])
        end = np.array([(far(), start[0, 1] + u(-2.0, 2.0), 0.0), (start[1, 0] + u(-2.0, 2.0), far(), 0.0), (far(), -far(), 0.0),
                        (-far(), start[3, 1] + u(-2.0, 2.0), 0.0)])
        start[:, 2] = 0.1 + rng.uniform(0.02, 0.15, B); end[:, 2] = 0.1 + rng.uniform(0.02, 0.15, B)
        q = dict(start_pt=start, start_v=np.zeros((B, 3)), start_a=np.zeros((B, 3)), end_pt=end, end_v=np.zeros((B, 3)),
                 f_ext=rng.uniform(-0.5, 0.5, (B, 3)) * np.array([1.0, 1.0, 0.3]))
        runs.append(_run(w, q))
    return runs


CASES = dict(byte_map=byte_map, fast_off=fast_off, byte_map_fast_off=byte_map_fast_off, clamp_tau=clamp_tau, clamp_res=clamp_res,
             init_false=init_false, local_box=local_box, pool_exhaustion=pool_exhaustion, truncation=truncation,
             end_vel_start_acc=end_vel_start_acc, map_border=map_border)

_runs, _oracle = {}, {}


def runs_of(name):
    """The runs of a case, built once per process (the worlds and the oracle's answers are shared by the tests and never modified)."""
    if name not in _runs:
        _runs[name] = CASES[name]()
    return _runs[name]


def oracle_of(run, cap=2048):
    """The oracle's answer for a run: UNTRUNCATED (cap = 2048 rows, kino_size the full count), with the run's pool, box and init."""
    from . import astar_lib as AL
    key = (id(run), cap)
    if key not in _oracle:
        w = run["world"]
        if run["allocate_num"] is not None:
            w = dict(w); w["allocate_num"] = run["allocate_num"]
        q = run["q"]
        _oracle[key] = (run, AL.plan_batch(w, q["start_pt"], q["start_v"], q["start_a"], q["end_pt"], q["end_v"], q["f_ext"], init=run["init"], cap=cap,
                                           nthreads=4, local_box=run["local_box"]))
    return _oracle[key][1]
