"""GPU tests of the fleet state machine (include/frp_nmpc_fsm.h, csrc/frp_fsm.hip, solver.FleetFSM) against tests/fsm_oracle.py: the scripted
sequence of tests/fsm_cases.py callback by callback (the script's fleet, one planner, a tail workgroup), the replan start state at the
edges of its plan test and at both horizon limits, the A* buffers and paths of planners that do not search, FleetFSM.period on a small
map with the oracle fed the read-back verdicts, and that period replayed from a hipGraph.
The layer is structurally unpinned (the reference holds no test vectors for it): the oracle is a restatement."""
import numpy as np
import pytest

from forces_resilient_planner_amd import layout as L, solver, workloads

from . import fsm_cases as FC
from . import fsm_oracle as FO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WEIGHTS = (15.0, 3.0, 80.0, 15.0, 0.0)
TRIG_TOL = 1e-12          # device trigonometry against libm: the bound of tests/test_gpu_command.py
EXACT = ("end_pt", "external_acc", "last_external_acc", "kino_start_time", "change_yaw_time", "yaw_odom")
SENTINEL = -777.25


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _fleet(B, N=20, M=30, F=6, **kw):
    return solver.DeviceFleet(B, N, M, F, L.MODEL_NORMAL, WEIGHTS, weights_final=WEIGHTS, **kw)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def _compare(fsm, want, where):
    got = fsm.arrays()
    got["mode"] = fsm.mode.cpu().numpy()
    for k in FO.INTS:
        assert np.array_equal(got[k], want[k]), (where, k, np.nonzero(got[k] != want[k])[0][:8], got[k][got[k] != want[k]][:8], want[k][got[k] != want[k]][:8])
    for k in EXACT:
        assert _same_bits(got[k], want[k]), (where, k)
    assert np.all(np.abs(got["init_yaw"] - want["init_yaw"]) <= TRIG_TOL), (where, "init_yaw", np.max(np.abs(got["init_yaw"] - want["init_yaw"])))


def _compare_start(bufs, search, starts, where):
    sp, sv, sa, rp, rv = [x.cpu().numpy() for x in bufs]
    for b, s in enumerate(starts):
        if s is None:
            assert search[b] == 0 and all(np.all(x[b] == SENTINEL) for x in (sp, sv, sa, rp, rv)), (where, b)
            continue
        assert search[b] == 1
        assert _same_bits(sp[b], s["start_pt"]) and _same_bits(sv[b], s["start_vel"]), (where, b, s["source"], sp[b], s["start_pt"])
        assert _same_bits(rp[b], s["retry_pt"]) and _same_bits(rv[b], s["retry_vel"]), (where, b)
        assert np.all(np.abs(sa[b] - np.array(s["start_acc"])) <= TRIG_TOL), (where, b, sa[b], s["start_acc"])
        if s["source"] == "odom":
            assert _same_bits(sa[b], [0.0, 0.0, 0.0])


def run_script(B):
    """The scripted sequence through the six entry points, callback by callback, every array compared after every call."""
    import torch
    events = FC.sequence(B)
    _, after, _ = FC.run_oracle(events, B)
    fleet = _fleet(B, FC.N)
    fsm = solver.FleetFSM(fleet, ext_noise_bound=FC.BOUND)
    bufs = [torch.zeros((B, 3), dtype=torch.float64, device=DEV) for _ in range(5)]
    n_search = 0
    for i, (e, a) in enumerate(zip(events, after)):
        kind = e["kind"]
        if kind == "host":
            if len(e["idx"]):
                getattr(fsm, e["name"])[torch.from_numpy(e["idx"]).to(DEV)] = int(e["value"])
            continue
        if kind == "goal":
            fsm.goal(_dev(e["goal"], np.float64), _dev(e["fresh"], np.int32))
        elif kind == "force":
            fsm.force(_dev(e["force"], np.float64), _dev(e["fresh"], np.int32))
        elif kind == "safety":
            fsm.safety_verdict(_dev(e["goal_blocked"], np.int32), _dev(e["first_hit"], np.int32))
        elif kind == "mpc":
            fsm.mpc_result(_dev(e["result"], np.int32))
        elif kind == "exec":
            fleet.pre_plan.copy_(_dev(e["pre_plan"], np.float64)); fsm.tick.exit_code.copy_(_dev(e["exit_code"], np.int32))
            for x in bufs:
                x.fill_(SENTINEL)
            fsm.search.fill_(-99)
            now = _dev([e["now"]], np.float64)
            fsm.exec_begin(_dev(e["state"], np.float64), _dev(e["t_cur"], np.float64), now, *bufs, Ts=FC.TS, mass=FC.MASS, g=FC.G)
            torch.cuda.synchronize()
            search = fsm.search.cpu().numpy()
            assert np.array_equal(search, a["search"]), (i, "search")
            _compare(fsm, a["after_begin"], (i, "exec_begin"))
            _compare_start(bufs, search, a["start"], i)
            n_search += int(search.sum())
            fsm.exec_end(_dev(e["astar_status"], np.int32), now)
        torch.cuda.synchronize()
        _compare(fsm, a, (i, kind))
    return n_search


def test_a_scripted_sequence_equals_the_oracle_callback_by_callback():
    assert run_script(FC.B) >= 40


@pytest.mark.parametrize("B", [1, 257])
def test_b_one_planner_and_one_more_than_a_whole_workgroup(B):
    """(frp_fsm.hip launches 256 threads per workgroup)"""
    run_script(B)


@pytest.mark.parametrize("N", [2, 20, 64])
def test_c_start_state_at_the_edges_of_the_plan_test(N):
    """Every planner in REPLAN_TRAJ (a few in GEN_NEW_TRAJ, a few executing) with t_cur on a stage boundary, below zero, exactly (N - 1) Ts,
    NaN, beyond int, just inside the last stage, and seeded draws; yaw inputs play no part here."""
    import torch
    B, Ts = 96, FC.TS
    rng = np.random.default_rng(N)
    fleet = _fleet(B, N)
    fsm = solver.FleetFSM(fleet)
    t_cur = rng.uniform(0.0, (N - 1) * Ts, B)
    special = [0.0, Ts * (N - 1), -1e-9, float("nan"), 1e300, float("inf"), (N - 1) * Ts * (1 - 1e-12), -0.0] + [Ts * k for k in range(1, min(N - 1, 6))]
    t_cur[:len(special)] = special
    state = np.full(B, FO.REPLAN_TRAJ, dtype=np.int32); state[60:70] = FO.GEN_NEW_TRAJ; state[70:80] = FO.EXEC_TRAJ
    exit_code = np.ones(B, dtype=np.int32); exit_code[50:60] = rng.choice([0, -7, 2], 10)
    pre_plan = rng.normal(size=(B, N, 17)); pre_plan[:, :, 3] = 7.3 + pre_plan[:, :, 3]
    odom = rng.normal(size=(B, 9))
    fsm.state.copy_(_dev(state, np.int32)); fleet.pre_plan.copy_(_dev(pre_plan, np.float64)); fsm.tick.exit_code.copy_(_dev(exit_code, np.int32))
    bufs = [torch.full((B, 3), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(5)]
    fsm.exec_begin(_dev(odom, np.float64), _dev(t_cur, np.float64), _dev([1.5], np.float64), *bufs, Ts=Ts, mass=FC.MASS, g=FC.G)
    torch.cuda.synchronize()
    starts, n_plan = [], 0
    for b in range(B):
        p = FO.Planner(state=int(state[b]))
        starts.append(p.exec_begin(odom[b], pre_plan[b], int(exit_code[b]), float(t_cur[b]), 1.5, N, Ts, FC.MASS, FC.G))
        n_plan += starts[-1] is not None and starts[-1]["source"] == "plan"
    _compare_start(bufs, fsm.search.cpu().numpy(), starts, N)
    assert starts[0]["source"] == "plan" and all(starts[k]["source"] == "odom" for k in (1, 2, 3, 4, 5)) and starts[6]["source"] == "plan" and starts[7]["source"] == "plan"
    assert all(s is None for s in starts[70:80]) and all(s["source"] == "odom" for s in starts[50:70])
    assert n_plan >= 50


def test_c_replan_start_state_is_the_command_timers_sample():
    """The two users of csrc/frp_fleet.hpp's plan sampling on one plan at one time: a planner in REPLAN_TRAJ with exit_code 1 starts its
    search where the command timer, in PUB_TRAJ with a trajectory, publishes its sample -- position, velocity and acceleration bit for bit.
    B = 257 (one more than a workgroup), N = 20, S = 1; t_cur on a stage boundary, inside the first and the last stage, 0.0 and seeded
    draws in [0, (N - 1) Ts): every planner is inside its plan, in both kernels.  The acceleration goes through the device library's sin
    and cos of the same half angles, called from a function of its own in one kernel and inline in the other: the same bits (measured
    on an MI355X, before and after the header: max |difference| = 0)."""
    import torch
    B, N, Ts = 257, 20, FC.TS
    rng = np.random.default_rng(2057)
    t_cur = rng.uniform(0.0, (N - 1) * Ts, B)
    t_cur[:5] = [3 * Ts, 0.3 * Ts, (N - 2 + 0.6) * Ts, 0.0, 0.999 * Ts]
    assert np.all(t_cur >= 0.0) and np.all(t_cur / Ts < N - 1)
    pre_plan = rng.normal(size=(B, N, 17)); pre_plan[:, :, 3] = 7.3 + pre_plan[:, :, 3]
    odom = rng.normal(size=(B, 9))
    fleet = _fleet(B, N)
    fsm = solver.FleetFSM(fleet)
    fsm.state.fill_(FO.REPLAN_TRAJ); fsm.tick.exit_code.fill_(1); fleet.pre_plan.copy_(_dev(pre_plan, np.float64))
    bufs = [torch.full((B, 3), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(5)]
    fsm.exec_begin(_dev(odom, np.float64), _dev(t_cur, np.float64), _dev([1.5], np.float64), *bufs, Ts=Ts, mass=FC.MASS, g=FC.G)
    ones, zeros = _dev(np.ones(B), np.int32), _dev(np.zeros(B), np.int32)
    status = _dev(np.full(B, solver.CMD_PUB_TRAJ), np.int32)
    c = solver.command_batch_device(fleet.pre_plan, ones, _dev(t_cur.reshape(B, 1), np.float64), status, zeros, _dev(np.zeros((B, 3)), np.float64),
                                    Ts=Ts, mass=FC.MASS, g=FC.G)
    torch.cuda.synchronize()
    assert np.all(c.kind.cpu().numpy() == solver.COMMAND_TRAJ) and np.all(fsm.search.cpu().numpy() == 1)   # the sampled branch, in both, for everyone
    cmd = c.cmd.cpu().numpy()
    sp, sv, sa = [x.cpu().numpy() for x in bufs[:3]]
    print("start_acc against the published acceleration: max |difference| = %.3e" % float(np.max(np.abs(sa - cmd[:, 0, 13:16]))))
    assert _same_bits(sp, cmd[:, 0, 0:3])
    assert _same_bits(sv, cmd[:, 0, 7:10])
    assert _same_bits(sa, cmd[:, 0, 13:16])


def _world():
    """The empty 20 x 20 x 4 m world of tests/test_gpu_astar.py (origin (-10, -10, -1), 0.1 m voxels) with one pillar at the origin."""
    w = workloads.astar_world(0, "empty", allocate_num=12000)
    dm = solver.OccupancyMap(w)
    pillar = np.array([(x, y, z) for x in np.arange(-0.25, 0.26, 0.1) for y in np.arange(-0.25, 0.26, 0.1) for z in np.arange(-0.95, 2.96, 0.1)], dtype=np.float32)
    dm.insert_cloud(pillar)
    return w, dm, pillar


def test_d_planners_that_do_not_search_keep_their_astar_buffers_and_their_path():
    import torch
    B = 8
    w, dm, _ = _world()
    fleet = _fleet(B)
    fsm = solver.FleetFSM(fleet)
    pl = solver.AstarPlanner(dm, B, K=256)
    fsm.bind(pl)
    for x in pl._q[:3] + pl._retry + [pl.kino_path]:
        x.fill_(SENTINEL)
    pl.kino_size.fill_(123); pl.status.fill_(solver.ASTAR_NO_PATH)
    # planner 2 searches (GEN_NEW_TRAJ), everybody else does not: executing, waiting, aligning, INIT
    states = [FO.EXEC_TRAJ, FO.WAIT_TARGET, FO.GEN_NEW_TRAJ, FO.INIT_YAW, FO.INIT, FO.EXEC_TRAJ, FO.WAIT_TARGET, FO.EXEC_TRAJ]
    fsm.state.copy_(_dev(states, np.int32)); fsm.have_target.fill_(1); fsm.exec_mpc.fill_(1)
    end = np.tile([-4.05, -4.05, 1.2], (B, 1)); fsm.end_pt.copy_(_dev(end, np.float64))
    odom = np.zeros((B, 9)); odom[:, 0:3] = (-6.05, -6.05, 1.05); odom[:, 8] = 3.0
    fsm.exec_step(pl, _dev(odom, np.float64), _dev(np.zeros(B), np.float64), _dev([2.0], np.float64))
    torch.cuda.synchronize()
    search = fsm.search.cpu().numpy()
    assert search.tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    for b in range(B):
        kept = all(bool((x[b] == SENTINEL).all()) for x in pl._q[:3] + pl._retry + [pl.kino_path])
        if b == 2:
            assert not kept and int(pl.status[b]) != solver.ASTAR_NO_PATH and 0 < int(pl.kino_size[b]) != 123
            assert int(fsm.state[b]) == FO.EXEC_TRAJ and float(fsm.kino_start_time[b]) == 2.0 and int(fsm.cmd_status[b]) == solver.CMD_PUB_TRAJ
            assert _same_bits(pl._q[0][b].cpu().numpy(), odom[b, 0:3]) and _same_bits(pl._q[2][b].cpu().numpy(), [0.0, 0.0, 0.0])
        else:
            assert kept and int(pl.kino_size[b]) == 123 and int(pl.status[b]) == solver.ASTAR_NO_PATH and float(fsm.kino_start_time[b]) == 0.0
    assert int(fsm.state[1]) == FO.INIT_YAW and int(fsm.state[3]) == FO.INIT_YAW and int(fsm.state[4]) == FO.INIT


# ---- FleetFSM.period on a map ----
STEPS = 2
START = np.array([(-6.05, -6.05), (-6.05, -3.05), (-6.05, 0.05), (-6.05, 3.05), (-6.05, 6.05), (2.05, -6.05), (2.05, 6.05), (4.05, -3.05)])
GOAL1 = np.array([(-4.55, -6.05), (5.95, -3.05), (5.95, 0.05), (-3.05, 3.05), (0.0, 0.0), (6.05, -6.05), (6.05, 6.05), (8.05, -3.05)])


def _box_around(c, half=1.0, thick=0.3):
    """A closed box of obstacle points around c: four walls, a roof and a floor, `thick` metres thick, `half` metres from c."""
    g = np.arange(-half - thick, half + thick + 0.01, 0.1)
    pts = [(x, y, z) for x in g for y in g for z in g if max(abs(x), abs(y), abs(z)) > half]
    return (np.array(pts) + np.asarray(c)).astype(np.float32)


class Harness:
    """The fleet, its map, its state machine, and the oracle that follows them: the oracle is fed what the device's period read back (safety
    verdicts, A* statuses, tick results) and has to hold the same state after it."""

    def __init__(self, B=8, steps=STEPS):
        import torch
        self.torch, self.B, self.steps = torch, B, steps
        self.w, self.dm, pillar = _world()
        self.dm.insert_cloud(_box_around((GOAL1[3][0], GOAL1[3][1], 1.2)))          # planner 3's goal is enclosed
        self.fleet = _fleet(B, F=64)
        self.fleet.poly_index = torch.zeros((B, 20), dtype=torch.int32, device=DEV)
        self.fsm = solver.FleetFSM(self.fleet)
        self.pl = solver.AstarPlanner(self.dm, B, K=512)
        self.fsm.bind(self.pl)
        self.cloud = _dev(pillar.astype(np.float64), np.float64)                      # the corridor's cloud: the pillar (shared by all planners)
        self.odom = np.zeros((B, 9)); self.odom[:, 0:2] = START; self.odom[:, 2] = 1.2
        d = GOAL1 - START
        self.odom[:, 8] = np.arctan2(d[:, 1], d[:, 0])                                # everybody faces its first goal
        self.state = _dev(self.odom, np.float64)
        self.goal = torch.zeros((B, 3), dtype=torch.float64, device=DEV); self.goal_fresh = torch.zeros((B,), dtype=torch.int32, device=DEV)
        self.force = torch.zeros((B, 3), dtype=torch.float64, device=DEV); self.force_fresh = torch.zeros((B,), dtype=torch.int32, device=DEV)
        self.clock = torch.zeros((steps + 2,), dtype=torch.float64, device=DEV)
        self.oracle = [FO.Planner() for _ in range(B)]
        self.period = 0
        self.cmd = None

    def inputs(self, goal=None, force=None):
        """goal / force: {planner: xyz} of this period's messages."""
        g = np.zeros((self.B, 3)); gf = np.zeros(self.B, dtype=np.int32); f = np.zeros((self.B, 3)); ff = np.zeros(self.B, dtype=np.int32)
        for b, v in (goal or {}).items():
            g[b] = v; gf[b] = 1
        for b, v in (force or {}).items():
            f[b] = v; ff[b] = 1
        self.goal.copy_(_dev(g, np.float64)); self.goal_fresh.copy_(_dev(gf, np.int32)); self.force.copy_(_dev(f, np.float64)); self.force_fresh.copy_(_dev(ff, np.int32))
        self.state.copy_(_dev(self.odom, np.float64))
        self.times = solver.FleetFSM.clock_for(0.05 * self.period, self.steps)
        self.clock.copy_(_dev(self.times, np.float64))
        return g, gf, f, ff

    def call(self, stream=None):
        self.cmd = self.fsm.period(self.pl, self.dm, self.state, self.clock, self.cloud, goal=self.goal, goal_fresh=self.goal_fresh, force=self.force,
                                   force_fresh=self.force_fresh, fsm_steps=self.steps, stream=stream)

    def vehicle(self):
        """The odometry of the next period (a perfect vehicle; odometry is an input of this layer): a planner that executes sits on its
        plan's stage 1; a planner that rotates takes the yaw the command timer published last."""
        t = self.torch
        plan = self.fleet.mpc_output[:, 1, 8:17].cpu().numpy()
        run = self.fsm.tick.accept.cpu().numpy() != 0
        self.odom[run] = plan[run]
        kind = self.cmd.kind[:, -1].cpu().numpy(); yaw = self.cmd.cmd[:, -1, 12].cpu().numpy()
        rot = kind == solver.COMMAND_YAW
        self.odom[rot, 8] = yaw[rot]
        t.cuda.synchronize()


def test_e_periods_on_a_map_follow_the_oracle_through_goal_force_collision_and_give_up():
    """FleetFSM.period with one exec step per period, so that every search's status can be read back after it.  The oracle gets the
    messages, then what the device read back: the safety verdicts (and a goal the search moved), the A* statuses, what the tick and the
    command timer wrote into the shared arrays (they have their own tests), and the tick results."""
    import torch
    h = Harness(steps=1)
    B, fsm, pl = h.B, h.fsm, h.pl
    fsm.have_odom.fill_(1); fsm.have_odom[6] = 0                     # planner 6 never hears its odometry
    for b, p in enumerate(h.oracle):
        p.have_odom = int(b != 6)
    seen = dict(second_goal=-1, reached=-1, force_replan=False, block_replan=False, gave_up=False)
    EVENT = 14
    for period in range(90):
        h.period = period
        goal, force = {}, {}
        if period == 0:
            goal = {b: (GOAL1[b][0], GOAL1[b][1], 0.0) for b in range(B) if b != 4}
            goal[5] = (GOAL1[5][0], GOAL1[5][1], -1.0)               # planner 5's goal lies below the floor: ignored; planner 4 gets none
        if period == EVENT:
            force[1] = (2.0, 0.0, 0.0)                               # a force step on an executing planner
            # a slab across planner 2's path, short of the pillar, low enough and narrow enough to fly around
            block = np.array([(x, y, z) for x in np.arange(-3.05, -2.74, 0.1) for y in np.arange(-0.35, 0.46, 0.1) for z in np.arange(0.55, 1.86, 0.1)], dtype=np.float32)
            h.dm.insert_cloud(block)
        if seen["reached"] >= 0 and seen["second_goal"] < 0:
            goal[0] = (-4.55, -4.75, 0.0)                            # the second goal, about a radian and a half to the left
            seen["second_goal"] = period
        g, gf, f, ff = h.inputs(goal, force)
        states0 = fsm.state.cpu().numpy().copy()
        pre_plan = h.fleet.pre_plan.cpu().numpy(); exit_code = fsm.tick.exit_code.cpu().numpy(); mpc_start = fsm.mpc_start.cpu().numpy()
        h.call()
        torch.cuda.synchronize()
        sc = fsm.safety_out
        blocked, hit, end_after = sc.goal_blocked.cpu().numpy(), sc.first_hit.cpu().numpy(), fsm.end_pt.cpu().numpy()
        search, status, result = fsm.search.cpu().numpy(), pl.status.cpu().numpy(), fsm.tick.result.cpu().numpy()
        shared = {k: getattr(fsm, k).cpu().numpy() for k in ("exec_mpc", "cmd_status", "pub_end", "mode")}
        for b, p in enumerate(h.oracle):
            p.goal(g[b], gf[b]); p.force(f[b], ff[b], solver.FSM_EXT_NOISE_BOUND)
            if p.have_target and blocked[b]:
                p.end_pt = [float(v) for v in end_after[b]]          # the goal search may have moved it: the map's part, read back
            p.safety(blocked[b], hit[b])
            after_safety = p.state
            start = p.exec_begin(h.odom[b], pre_plan[b], int(exit_code[b]), h.times[0] - mpc_start[b], h.times[0])
            gave_up = "plan:give_up" in p.met
            assert (start is not None) == bool(search[b]), (period, b, p.state, search[b])
            p.exec_end(start is not None, int(status[b]), h.times[0])
            if period >= EVENT and start is not None and after_safety == FO.REPLAN_TRAJ and status[b] != FO.NO_PATH and b in (1, 2):
                seen["force_replan" if b == 1 else "block_replan"] = True
            if b == 3 and gave_up:
                seen["gave_up"] = True
            if period == EVENT and b in (1, 2):
                assert states0[b] == FO.EXEC_TRAJ and after_safety == FO.REPLAN_TRAJ and (b == 1 or hit[b] >= 0), (b, states0[b], after_safety, hit[b])
            for k, v in shared.items():                               # the tick's and the command timer's stores
                setattr(p, k, int(v[b]))
            p.mpc(int(result[b]))
            for k, v in shared.items():
                setattr(p, k, int(v[b]))
        _compare(fsm, FC.arrays(h.oracle), period)
        if result[0] == 0 and seen["reached"] < 0:
            seen["reached"] = period
        h.vehicle()
        if seen["second_goal"] >= 0 and int(fsm.state[0]) == FO.EXEC_TRAJ and seen["gave_up"] and seen["force_replan"] and seen["block_replan"]:
            break
    assert seen["reached"] >= 0 and seen["second_goal"] > seen["reached"] and int(fsm.state[0]) == FO.EXEC_TRAJ, seen    # reached its goal, took a second one
    assert seen["force_replan"] and seen["block_replan"] and seen["gave_up"], seen
    assert int(fsm.have_target[3]) == 0 and int(fsm.state[3]) == FO.WAIT_TARGET
    assert int(fsm.state[4]) == FO.INIT and int(fsm.state[5]) == FO.INIT and int(fsm.state[6]) == FO.INIT and int(fsm.have_target[6]) == 1
    assert int(fsm.state[7]) == FO.EXEC_TRAJ


def _bits(x):
    import torch
    return x.view(torch.int64) if x.dtype == torch.float64 else x


def test_f_period_replayed_from_a_hipgraph_equals_eager_launches():
    """FleetFSM.period captured once on one stream with the default queue count and replayed with new goal / force / odometry / clock
    buffers; the state is reset before every run."""
    import torch
    T = 7

    def run(h, fn):
        res = []
        for period in range(T):
            h.period = period
            goal = {b: (GOAL1[b][0], GOAL1[b][1], 0.0) for b in range(h.B)} if period == 0 else ({7: (8.05, -1.05, 0.0)} if period == 5 else {})
            h.inputs(goal, {1: (2.0, 0.0, 0.0)} if period == 4 else {})
            fn()
            torch.cuda.synchronize()
            f = h.fsm
            res.append([x.clone() for x in [getattr(f, n) for n in f.INT_FIELDS + ("search", "exec_mpc", "cmd_status", "pub_end", "mode") + tuple(n for n, _ in f.F64_FIELDS)]
                        + [f.tick.result, f.mpc_start, h.pl.kino_size, h.pl.status, h.fleet.mpc_output, h.fleet.pre_plan, h.cmd.cmd, h.cmd.kind]])
            h.vehicle()
        return res

    eager = Harness()
    eager.fsm.have_odom.fill_(1)
    ref = run(eager, eager.call)
    assert int((eager.fsm.state == FO.EXEC_TRAJ).sum()) >= 6 and int(eager.fsm.tick.result.eq(1).sum()) >= 4

    h = Harness()
    h.fsm.have_odom.fill_(1)
    h.inputs()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        h.call(side)                                                   # warm-up: every lazy allocation happens here
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        h.call(torch.cuda.current_stream())
    torch.cuda.synchronize()
    # back to the constructor's state: the warm-up and the capture ran nothing that matters with have_target == 0, but the tick state moved
    fresh = Harness()
    fresh.fsm.have_odom.fill_(1)
    for n in h.fsm.INT_FIELDS + ("search",) + tuple(n for n, _ in h.fsm.F64_FIELDS) + ("mpc_start",):
        getattr(h.fsm, n).copy_(getattr(fresh.fsm, n))
    for n in solver.TickState.INT_FIELDS:
        getattr(h.fsm.tick, n).copy_(getattr(fresh.fsm.tick, n))
    h.fsm.tick.cmd_end_pt.zero_(); h.fleet.mode.copy_(fresh.fleet.mode); h.fleet.mpc_output.copy_(fresh.fleet.mpc_output)
    h.fleet.pre_plan.copy_(fresh.fleet.pre_plan); h.fleet.have_traj.copy_(fresh.fleet.have_traj)
    h.fleet.solver.iters.copy_(fresh.fleet.solver.iters)
    for x in (h.cmd.cmd, h.cmd.kind, h.cmd.finish, h.cmd.reset_output):
        x.zero_()
    h.pl.kino_path.zero_(); h.pl.kino_size.zero_(); h.pl.status.zero_()
    got = run(h, g.replay)
    for t, (a, b) in enumerate(zip(got, ref)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(_bits(x), _bits(y)), (t, i)
