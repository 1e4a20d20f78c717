"""-m gpu: every route through the kinodynamic A* kernel (csrc/frp_astar.hip) against the CPU oracle, to the bit, and the device's own
result against the referee written from the mathematics (tests/astar_referee.py).

tests/test_gpu_astar.py runs the kernel on workloads.astar_world's defaults only, which always take the same route.  The cases of
tests/astar_path_cases.py leave it by one switch each -- the byte map, the general cell -> voxel path, both, the clamped window (two
ways), init_search = 0, a local box, an exhausted node pool, truncated samples, non-zero end velocity / start acceleration, the
map's border -- and tests/test_astar_paths_cpu.py proves without a device that each case takes its route.  Compared per planner:
status, nodes created, expansions, the retry flag, path-node ids, states, inputs, durations, kino_size and the samples."""
import numpy as np
import pytest

from forces_resilient_planner_amd import solver

from . import astar_gpu_lib as AG
from . import astar_path_cases as C
from . import astar_referee as R

pytestmark = pytest.mark.gpu


def _referee_on_the_device_result(run, pl, o):
    st = pl.status.cpu().numpy(); sz = pl.kino_size.cpu().numpy(); stats = pl.stats.cpu().numpy()
    kp = pl.kino_path.cpu().numpy(); pn = pl.path_nodes.cpu().numpy()
    q = run["q"]
    judged = 0
    for b in range(C.B):
        if st[b] == solver.ASTAR_NO_PATH:
            continue
        n = abs(int(stats[b, 3]))
        s = R.check(run["world"], q["start_pt"][b], q["start_v"][b], q["start_a"][b], q["end_pt"][b], q["end_v"][b], q["f_ext"][b], run["init"],
                    bool(stats[b, 2]), int(st[b]), pn[b, :n, :10], kp[b, :sz[b]], Ts=pl.Ts, local_box=None if run["local_box"] is None else run["local_box"][b])
        judged += s["nodes"]
    return judged


def _one(run, K=None):
    w = run["world"]
    pl = AG.run_gpu(w, run["q"], C.B, K=K or run["K"], init=run["init"], local_box=run["local_box"])
    o = C.oracle_of(run)
    AG.compare(pl, o, C.B)
    _referee_on_the_device_result(run, pl, o)
    return pl, o


@pytest.mark.parametrize("name", ["byte_map", "fast_off", "byte_map_fast_off", "clamp_tau", "clamp_res", "end_vel_start_acc", "map_border"])
def test_route_equals_the_oracle(name):
    """The routes that need nothing but their world and queries: the byte map (grid z = 80 > 64: no packed map, no staged window, an
    empty cell box), the general cell_state path (an origin half a voxel off: fast == 0), both at once, the window clamped to radius
    31 (max_tau = 0.8; resolution 0.05) with lookups beyond it falling back to the packed map in HBM, end_vel / start_acc != 0, and
    starts at the map's border (the window hangs over the grid's edge, cells outside the map)."""
    st = []
    for run in C.runs_of(name):
        w = run["world"]
        assert (C.grid_z(w) > 64) == (name in ("byte_map", "byte_map_fast_off"))
        assert (not C.fast_flag(w)) == (name in ("fast_off", "byte_map_fast_off"))
        assert (min(C.win_r_wanted(w, f) for f in run["q"]["f_ext"]) > C.WIN_R_MAX) == (name in ("clamp_tau", "clamp_res"))
        pl, o = _one(run)
        assert tuple(pl.occ.shape)[2] == C.grid_z(w)
        st += pl.status.cpu().tolist()
    assert any(s != solver.ASTAR_NO_PATH for s in st)
    if name == "end_vel_start_acc":
        assert solver.ASTAR_REACH_END in st and solver.ASTAR_REACH_HORIZON in st


def test_init_false_uses_the_full_primitive_set_and_never_retries():
    st, rt = [], []
    for run in C.runs_of("init_false"):
        pl, o = _one(run)
        st += pl.status.cpu().tolist(); rt += pl.stats.cpu().numpy()[:, 2].tolist()
    assert not any(rt) and solver.ASTAR_NO_PATH in st  # stats[:, 2] == 0 everywhere, also for the NO_PATH planner


def test_local_box_equals_the_oracles_local_map():
    """The oracle's use_local / local_min / local_max against the kernel's local_box, per planner (boxes of the map's local view with
    a radius shorter than the search, and one hand-made box that cuts a pillar in half); the box changes at least one result."""
    changed = 0
    for run in C.runs_of("local_box"):
        pl, o = _one(run)
        free = AG.run_gpu(run["world"], run["q"], C.B, K=run["K"])
        AG.compare(free, C.oracle_of(C.without_box(run)), C.B)
        changed += sum(1 for b in range(C.B) if not np.array_equal(free.kino_path[b].cpu().numpy(), pl.kino_path[b].cpu().numpy()) or
                       not np.array_equal(free.stats[b].cpu().numpy(), pl.stats[b].cpu().numpy()))
    assert changed >= 1


def test_pool_exhaustion_ends_in_no_path_and_the_retry():
    """allocate_num sized from the oracle's node counts so that one planner's first search and its retry both run out of nodes
    (NO_PATH: it keeps the path and size of an earlier, unconstrained plan) and another's first search runs out while its retry fits.
    From the code of run_search (read before this first ran on a device): the commit walk of the first wavefront gives a new node the
    number `use`, increments it and sets out_of_memory at use == allocate_num; the walk's loop condition (`m && !out_of_memory`)
    stops it there, as the oracle's `goto done` does -- the largest node number written is allocate_num - 1, the largest heap hole
    likewise.  The second wavefront's hash inserts count the same new nodes in the same order and stop at the same count (`full`); the
    node records are written afterwards for walked voxel groups only (c_winner stays -1 for the rest).  The hash has >= 2 allocate_num
    slots and cannot fill."""
    import torch
    for run in C.runs_of("pool_exhaustion"):
        w, q, A = run["world"], run["q"], run["allocate_num"]
        pl = AG.run_gpu(w, q, C.B, K=run["K"])                       # unconstrained: every planner gets a path
        path0 = pl.kino_path.clone(); size0 = pl.kino_size.clone()
        assert (size0 > 0).all() and pl.allocate_num == w["allocate_num"] > A
        pl.allocate_num = A                                            # (the workspace was sized for the larger pool)
        pl = AG.run_gpu(w, q, C.B, planner=pl)
        o = C.oracle_of(run)
        st = pl.status.cpu().numpy(); stats = pl.stats.cpu().numpy()
        AG.compare(pl, o, C.B)
        assert np.array_equal(st, o["status"]) and np.array_equal(stats[:, 2], o["retried"])
        x, y = run["both_out"], run["retry_fits"]
        assert st[x] == solver.ASTAR_NO_PATH and stats[x, 2] == 1 and stats[x, 0] == A
        assert st[y] != solver.ASTAR_NO_PATH and stats[y, 2] == 1 and stats[y, 0] < A
        for b in range(C.B):
            if st[b] == solver.ASTAR_NO_PATH:
                assert torch.equal(pl.kino_path[b], path0[b]) and int(pl.kino_size[b]) == int(size0[b])
        _referee_on_the_device_result(run, pl, o)


def test_truncation_keeps_the_first_K_samples():
    """More samples than K: kino_path[b, :K] is the first K rows of the oracle's untruncated path, kino_size == K and stats[b, 3] ==
    -n_path (AG.compare asserts all three for every planner whose count exceeds K) -- in the search part and, in the third world,
    in the shot part.  With K = the exact sample count of a planner nothing is negated and its last row is intact."""
    for run in C.runs_of("truncation"):
        pl, o = _one(run)
        sz = pl.kino_size.cpu().numpy(); stats = pl.stats.cpu().numpy(); st = pl.status.cpu().numpy()
        found = st != solver.ASTAR_NO_PATH
        assert found.any() and np.all(sz[found] == 32) and np.all(stats[found, 3] < 0)
        assert np.array_equal(pl.kino_path.cpu().numpy()[found], o["kino_path"][found, :32])
        e = C.exact_K(run, o["kino_size"], o["status"])
        K = e["K"]
        pe, _ = _one(e)
        sz = pe.kino_size.cpu().numpy(); stats = pe.stats.cpu().numpy()
        exact = [b for b in range(C.B) if found[b] and o["kino_size"][b] == K]
        assert exact
        for b in exact:
            assert sz[b] == K and stats[b, 3] == o["results"][b].n_path > 0
            assert np.array_equal(pe.kino_path[b, K - 1].cpu().numpy(), o["kino_path"][b, K - 1])
        for b in range(C.B):
            if found[b] and o["kino_size"][b] > K:
                assert sz[b] == K and stats[b, 3] == -o["results"][b].n_path
