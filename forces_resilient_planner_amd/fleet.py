"""B planners whose receding-horizon loop lives in HBM: DeviceFleet strings the planning stages and the solve into a tick, TickState keeps
what solveNMPC decides about it (frp_nmpc_pack_batch, _update_batch, _coldstart_batch, _mode_batch, _tick_*)."""
import ctypes
import os

import numpy as np

from . import layout as L
from .batch import DeviceSolver
from .capi import ASTAR_NO_PATH, CMD_INIT_POSITION, CMD_PUB_TRAJ, Pack, Tick, TickIn, _check, lib, stream_ptr, tensor_ptr
from .planning import command_batch_device, command_snapshot_device, corridor_batch_device, reference_batch_device, tube_batch_device


class TickState:
    """The per-planner state the tick outcome keeps on the device (frp_nmpc_tick, include/frp_nmpc_outcome.h), all [B] int32 unless noted:
    fail_count, replan_count, kino_replan, exit_code (the last solve that RAN for the planner, not solver.exitflag), initialized, cmd_status
    (CMD_*: the tensor DeviceFleet.commands walks), pub_end, cmd_end_pt [B,3] f64, exec_mpc; the outputs gate (TICK_*), keep, accept, result,
    replan of tick_begin / tick_end; and ref_replan, which receives the references' replan flag inside DeviceFleet.full_tick.
    As the reference's constructor leaves them: counters 0, exit_code 0, initialized 0, cmd_status INIT_POSITION, pub_end 0; exec_mpc 1.
    Constructing it also makes fleet.pre_plan / fleet.have_traj exist (DeviceFleet.snapshot_commands allocates them on first use otherwise),
    so that a capture of full_tick(tick=...) allocates nothing.
    The loop without a host: DeviceFleet.full_tick(..., tick=ts) -> DeviceFleet.commands(t_cur, ts.cmd_status, ts.pub_end, ts.cmd_end_pt, ...)
    with ts.reset_output = the returned Commands.reset_output -> DeviceFleet.replan(..., replan=ts.replan, tick=ts)."""

    INT_FIELDS = ("fail_count", "replan_count", "kino_replan", "exit_code", "initialized", "cmd_status", "pub_end", "exec_mpc",
                  "gate", "keep", "accept", "result", "replan", "ref_replan")

    def __init__(self, fleet):
        t = fleet.torch
        dev = fleet.solver.device
        self.B = fleet.B
        for n in self.INT_FIELDS:
            setattr(self, n, t.zeros((self.B,), dtype=t.int32, device=dev))
        self.cmd_status.fill_(CMD_INIT_POSITION)
        self.exec_mpc.fill_(1)
        self.cmd_end_pt = t.zeros((self.B, 3), dtype=t.float64, device=dev)
        self._sizes = {}
        self.reset_output = None  # set it to Commands.reset_output of DeviceFleet.commands: every DeviceFleet.full_tick(tick=self) consumes and clears it
        fleet._command_buffers()

    def struct(self):
        p = lambda n: getattr(self, n).data_ptr()
        return Tick(self.B, *[p(n) for n, _ in Tick._fields_[1:]])

    def path_size(self, K):
        """kino_size [1] = K for a caller that passes whole paths (allocated on first use per K: call once outside a graph capture)."""
        if K not in self._sizes:
            self._sizes[K] = self.gate.new_full((1,), K)
        return self._sizes[K]

    def begin(self, reset_output=None, stream=None):
        """frp_nmpc_tick_begin: gate and keep of this tick; reset_output [B] int32 (Commands.reset_output) is consumed and cleared."""
        import torch
        if reset_output is not None:
            assert reset_output.dtype == torch.int32 and tuple(reset_output.shape) == (self.B,) and reset_output.is_contiguous()
        t = self.struct()
        _check(lib().frp_nmpc_tick_begin(ctypes.byref(t), tensor_ptr(reset_output),
                                         stream_ptr(stream, self.gate.device)), "frp_nmpc_tick_begin")

    def end(self, z, exitflag, mpc_output, state, end_pt, kino_path, kino_size, time_offset, ref_replan=None, Ts=0.05, mode=None, stream=None):
        """frp_nmpc_tick_end on device tensors: z [B,N,17], exitflag [B] int32, mpc_output [B,N+1,17] (before the update), state [B,9],
        end_pt [3] or [B,3], kino_path [K,3] or [B,K,3], kino_size int32 [1] or [B], time_offset [B], ref_replan [B] int32 (None: this
        object's own), mode [B] int32 or None."""
        import torch
        B, N, nz = z.shape
        K = kino_path.shape[-2]
        ref_replan = self.ref_replan if ref_replan is None else ref_replan
        per_end, per_path, per_size = end_pt.dim() == 2, kino_path.dim() == 3, kino_size.numel() > 1
        f64 = [(z, (B, N, L.NZ)), (mpc_output, (B, N + 1, L.NZ)), (state, (B, 9)), (end_pt, (B, 3) if per_end else (3,)),
               (kino_path, (B, K, 3) if per_path else (K, 3)), (time_offset, (B,))]
        i32 = [(exitflag, (B,)), (kino_size, (B,) if per_size else (1,)), (ref_replan, (B,))] + ([(mode, (B,))] if mode is not None else [])
        assert B == self.B
        for a, shape in f64:
            assert a.dtype == torch.float64 and tuple(a.shape) == shape and a.is_contiguous(), (tuple(a.shape), shape, a.dtype)
        for a, shape in i32:
            assert a.dtype == torch.int32 and tuple(a.shape) == shape and a.is_contiguous(), (tuple(a.shape), shape, a.dtype)
        t = self.struct()
        i = TickIn(N, K, float(Ts), z.data_ptr(), exitflag.data_ptr(), mpc_output.data_ptr(), state.data_ptr(), end_pt.data_ptr(), int(per_end),
                   kino_path.data_ptr(), int(per_path), kino_size.data_ptr(), int(per_size), time_offset.data_ptr(), ref_replan.data_ptr(),
                   mode.data_ptr() if mode is not None else None)
        _check(lib().frp_nmpc_tick_end(ctypes.byref(t), ctypes.byref(i), stream_ptr(stream, z.device)), "frp_nmpc_tick_end")


class DeviceFleet:
    """B planners whose receding-horizon loop lives in HBM: per tick
        pack (forces_normal.cpp:55-136 on the device)  ->  solve  ->  update (forces_normal.cpp:142-168,
        nmpc_solver.cpp:524-543 on the device).
    Host data is uploaded once (plans, polytopes, tube matrices); references / external forces per tick are device
    tensors handed to tick()."""

    def __init__(self, B, N, M, F, model, weights, device="cuda:0", npoly=None, weights_final=None):
        """weights_final: setParasFinal's five weights.  When given, every planner carries its own mode
        (self.mode [B], all FRP_MODEL_NORMAL at first): pack() picks its weights and solve() its objective by it, and
        update_mode() applies the reference's switch rule (nmpc_solver.cpp:436-447)."""
        import torch
        self.torch = torch
        self.B, self.N, self.M, self.F, self.model = B, N, M, F, model
        self.NPOLY = N if npoly is None else npoly
        self.weights = tuple(float(x) for x in weights)  # (w_stage_wp, w_stage_input, w_input_rate, w_terminal_wp, w_terminal_input)
        self.solver = DeviceSolver(B, N, M, min(M, F), model, device)
        # a fleet ticks: this tick's problem is the previous one shifted by a stage, and its iteration count is the best predictor of
        # this one's (frp_nmpc_batch.order_hint; zero before the first solve = "typical").  Saves the key kernel's pass over the
        # parameters as well (27 of a tick's 1590 us at 4096 planners).  FRP_FLEET_ORDER_HINT=0: the key of the initial guess, as before
        self.solver.order_by_last_iters = os.environ.get("FRP_FLEET_ORDER_HINT", "1") != "0"
        dev = self.solver.device
        f64 = dict(dtype=torch.float64, device=dev)
        self.mpc_output = torch.zeros((B, N + 1, L.NZ), **f64)
        self.ellipsoid = torch.zeros((B, N, 3, 3), **f64)
        self.poly_A = torch.zeros((B, self.NPOLY, F, 3), **f64)
        self.poly_b = torch.zeros((B, self.NPOLY, F), **f64)
        self.poly_nfaces = torch.zeros((B, self.NPOLY), dtype=torch.int32, device=dev)
        self.poly_index = None
        # per planner: polytopes produced by the last corridor() (>= 1), negated when one of them needed more than F rows and
        # was truncated (getSikangConst tests all rows; callers that size F below FRP_CORRIDOR_MAX_F should check overflowed())
        self.poly_count = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.weights_final = None if weights_final is None else tuple(float(x) for x in weights_final)
        self.mode = None
        if self.weights_final is not None:
            self.mode = torch.full((B,), int(model), dtype=torch.int32, device=dev)
            self.solver.models = self.mode

    def update_mode(self, time_offset, kino_size, end_pt, Ts=0.05, radius=1.0, stream=None):
        """switch_to_final for every planner (nmpc_solver.cpp:436-447): time_offset [B] f64, kino_size int32 [1] or [B],
        end_pt f64 [3] or [B,3] (device tensors).  Sticky until reset_mode()."""
        assert self.mode is not None, "construct the fleet with weights_final"
        _check(lib().frp_nmpc_mode_batch(self.B, self.N, tensor_ptr(self.mpc_output), tensor_ptr(time_offset), tensor_ptr(kino_size),
                                         1 if kino_size.numel() > 1 else 0, tensor_ptr(end_pt), 1 if end_pt.dim() == 2 else 0, float(Ts), float(radius),
                                         tensor_ptr(self.mode), stream_ptr(stream, self.solver.device)), "frp_nmpc_mode_batch")

    def reset_mode(self):
        """A new kinodynamic path puts every planner back on the normal solver (nmpc_solver.cpp:218)."""
        self.mode.fill_(L.MODEL_NORMAL)

    def to_device(self, a, dtype=None):
        t = self.torch
        return t.from_numpy(np.ascontiguousarray(a)).to(self.solver.device, dtype=dtype)

    def pack(self, external_acc, ref_pos, ref_yaw, stream=None):
        ds = self.solver
        pk = Pack(self.B, self.N, self.M, self.NPOLY, self.F, 1 if external_acc.dim() == 3 else 0,
                  self.mpc_output.data_ptr(), external_acc.data_ptr(),
                  ref_pos.data_ptr(), ref_yaw.data_ptr(), self.ellipsoid.data_ptr(), self.poly_A.data_ptr(),
                  self.poly_b.data_ptr(), self.poly_nfaces.data_ptr(),
                  self.poly_index.data_ptr() if self.poly_index is not None else None, *self.weights,
                  ds.xinit.data_ptr(), ds.x0.data_ptr(), ds.params.data_ptr(), ds.nfaces.data_ptr(),
                  self.mode.data_ptr() if self.mode is not None else None, *(self.weights_final or (0.0,) * 5),
                  # (from the second pack on: this fleet's solver buffers are as its own previous pack left them -- DeviceSolver.upload takes the promise back)
                  1 if getattr(ds, "_packed_by", None) is self else 0)
        _check(lib().frp_nmpc_pack_batch(ctypes.byref(pk), stream_ptr(stream, self.solver.device)), "frp_nmpc_pack_batch")
        ds._packed_by = self

    def update(self, stream=None, keep_failed=True, accept=None):
        """accept [B] int32: the planners whose result is taken over are those with accept == 1 (TickState.accept, the reference's whole
        rule) instead of those with solver.exitflag == 1 (its first branch)."""
        ds = self.solver
        flags = accept if accept is not None else ds.exitflag
        _check(lib().frp_nmpc_update_batch(self.B, self.N, tensor_ptr(ds.z), tensor_ptr(flags) if keep_failed else None,
                                           tensor_ptr(self.mpc_output), stream_ptr(stream, self.solver.device)), "frp_nmpc_update_batch")

    def tube(self, consts=None, stream=None):
        """ellipsoid_matrices_ of all B planners from their current plans
        (NMPCSolver::setFORCESParams, nmpc_solver.cpp:484-521) -> self.ellipsoid, on the device."""
        s = stream if stream is not None else self.torch.cuda.current_stream(self.solver.device)
        tube_batch_device(self.mpc_output, self.ellipsoid, consts, s)

    def corridor(self, cloud, ref_pos, ref_yaw, consts=None, stream=None, cloud_count=None, grid=None, cut=None, view=None):
        """polytopes and poly_indices of all B planners from the obstacle cloud, the stage
        references and the current tube (getSikangConst, nmpc_solver.cpp:288-332) -> self.poly_*, on the device.
        cut: OccupancyMap.cut(local_box) with the shared cloud and grid of OccupancyMap.shared_view().
        view: a SharedView in place of cloud / grid / cloud_count (cloud = None); combines with cut."""
        t = self.torch
        assert self.NPOLY == self.N
        if self.poly_index is None:
            self.poly_index = t.zeros((self.B, self.N), dtype=t.int32, device=self.solver.device)
        corridor_batch_device(cloud, ref_pos, ref_yaw, self.ellipsoid, self.poly_A, self.poly_b, self.poly_nfaces,
                              self.poly_index, self.poly_count, cloud_count, consts, stream, grid, cut, view)

    def overflowed(self):
        """Planners whose last corridor() truncated a polytope to F rows (device tensor of bool; all False before the first
        corridor() call)."""
        return self.poly_count < 0

    def coldstart(self, state=None, only_failed=True, thrust=7.3, stream=None, keep=None):
        """initMPCOutput for the planners whose last solve failed (nmpc_solver.cpp:363-364, :265-286), on the device.
        state [B,9] = stateMpc_ (odometry), or None: each planner restarts from its plan's stage-1 state.
        keep [B] int32: the planners with keep == 1 keep their plan (TickState.keep: :363's whole condition, and never a gated planner)
        instead of those with solver.exitflag == 1."""
        flags = keep if keep is not None else self.solver.exitflag
        _check(lib().frp_nmpc_coldstart_batch(self.B, self.N, tensor_ptr(state), tensor_ptr(flags) if only_failed else None,
                                              float(thrust), tensor_ptr(self.mpc_output), stream_ptr(stream, self.solver.device)), "frp_nmpc_coldstart_batch")

    def references(self, kino_path, time_offset, ref_pos, ref_yaw, replan=None, kino_size=None, Ts=0.05, stream=None):
        """SURVEY 8f row f-4 (first half): ref_total_pos_ / ref_total_yaw_ of all B planners from the kinodynamic
        path (getCurTraj + calculate_yaw, nmpc_solver.cpp:109-142, 834-862), on the device."""
        reference_batch_device(kino_path, time_offset, self.mpc_output, ref_pos, ref_yaw, replan, kino_size, Ts, stream)

    def replan(self, planner, end_pt, external_acc, replan, time_offset=None, end_vel=None, init=True, mass=0.74, g=9.81, stream=None,
               t_cur=None, odom=None, Ts=0.05, local_box=None, tick=None):
        """The FSM's REPLAN_TRAJ step (nmpc_manage.cpp:215-235 -> NMPCSolver::getKinoPath, nmpc_solver.cpp:145-223) for the planners
        whose tick raised kino_replan_ (`replan` [B] int32, as written by references() / full_tick): a kinodynamic A* to end_pt
        [B,3] with external_acc [B,3] in the primitives, on the device (AstarPlanner = frp_nmpc_astar_batch).
        Start state as in the reference (:159-186): a planner whose last solve succeeded (solver.exitflag == 1) starts from its plan
        interpolated at t_cur [B] seconds after the plan's start -- row floor(t_cur / Ts) towards the next one; None = the plan's
        stage-1 row (mpc_output[:, 1], the state the tick is about to apply) -- with the acceleration the planned thrust produces (:169-181), provided floor(t_cur / Ts) < N - 1 and t_cur >= 0;
        every other planner starts from odom = (pos [B,3], vel [B,3]) with zero acceleration.  The repeated search after NO_PATH starts
        from the odometry state too (:190-193).  odom = None is NOT the reference's behaviour: fallback and retry then start from the
        plan's stage-1 state (a warning is issued once); a caller that has odometry passes it.
        The planner object owns the per-planner paths (planner.kino_path / kino_size): pass them to references() / full_tick as the
        path.  Planners that found a path get time_offset = 0 (kino_start_time_ = now, :219) and go back to the normal solver (:218).
        local_box: int32 [B,6] of OccupancyMap.local_view for a planner built on that map (voxels outside a planner's box read as free,
        occ_map.cpp:101-102); None: the whole map is local.
        tick: a TickState.  "The last solve succeeded" is then tick.exit_code == 1 -- the last solve that ran for the planner, as in the
        reference, where solver.exitflag also holds the discarded solves of gated planners -- and the planners that got a path also get
        cmd_status <- PUB_TRAJ and pub_end <- 0 (:222-223); tick.replan is the natural `replan` argument.
        Returns the mask (bool [B]) of planners that received a new path.  Everything here -- the state gather, the search, the
        masks -- is enqueued on `stream` (torch's current stream when None)."""
        t = self.torch
        s = stream if stream is not None else t.cuda.current_stream(self.solver.device)
        with t.cuda.stream(s):
            B, N = self.B, self.N
            rows = self.mpc_output[:, :N]                      # pre_mpc_output_: rows 0..N-1 of the deque
            tc = t_cur if t_cur is not None else t.zeros((B,), dtype=t.float64, device=rows.device)
            idx = t.floor(tc / Ts).to(t.int64)
            use_plan = ((tick.exit_code if tick is not None else self.solver.exitflag) == 1) & (idx < N - 1) & (tc >= 0.0)
            i0 = idx.clamp(0, N - 2)
            ar = t.arange(B, device=rows.device)
            r0, r1 = rows[ar, i0], rows[ar, i0 + 1]
            mo = r0 + (t.fmod(tc, Ts) / Ts)[:, None] * (r1 - r0)
            if t_cur is None:
                mo = self.mpc_output[:, 1].clone()             # (the tick's convention here: the plan's next state)
            e = mo[:, 14:17]
            sr, cr, sp, cp, sy, cy = t.sin(e[:, 0]), t.cos(e[:, 0]), t.sin(e[:, 1]), t.cos(e[:, 1]), t.sin(e[:, 2]), t.cos(e[:, 2])
            zb = t.stack([cy * sp * cr + sy * sr, sy * sp * cr - cy * sr, cp * cr], 1)  # eulerToRot(e) [0 0 1]'
            acc = zb * (mo[:, 3:4] / mass)
            acc[:, 2] -= g
            if odom is None and not getattr(self, "_warned_no_odom", False):
                import warnings
                warnings.warn("DeviceFleet.replan without odom: fallback and retry start from the plan's stage-1 state, not from the "
                              "odometry state as in the reference (nmpc_solver.cpp:151-153, 190-193)")
                self._warned_no_odom = True
            o_pt, o_v = (odom if odom is not None else (self.mpc_output[:, 1, 8:11], self.mpc_output[:, 1, 11:14]))
            up = use_plan[:, None]
            s_pt = t.where(up, mo[:, 8:11], o_pt); s_v = t.where(up, mo[:, 11:14], o_v); s_a = t.where(up, acc, t.zeros_like(acc))
            ev = end_vel if end_vel is not None else t.zeros_like(end_pt)
            planner.upload(s_pt.contiguous(), s_v.contiguous(), s_a.contiguous(), end_pt, ev, external_acc,
                           retry=(o_pt.contiguous(), o_v.contiguous()))
            planner.plan(init=init, local_box=local_box, active=replan, stream=s)
            ok = (replan != 0) & (planner.status != ASTAR_NO_PATH)
            if time_offset is not None:
                time_offset.masked_fill_(ok, 0.0)
            if self.mode is not None:
                self.mode.masked_fill_(ok, L.MODEL_NORMAL)
            if tick is not None:
                tick.cmd_status.masked_fill_(ok, CMD_PUB_TRAJ)
                tick.pub_end.masked_fill_(ok, 0)
        return ok

    def full_tick(self, external_acc, kino_path, time_offset, cloud, ref_pos, ref_yaw, stream=None, replan=None,
                  kino_size=None, tube_consts=None, corridor_consts=None, Ts=0.05, coldstart=True, state=None, grid=None, cloud_count=None, cut=None,
                  view=None, tick=None, end_pt=None):
        """The reference's whole per-tick computation downstream of the A* (NMPCSolver::solveNMPC,
        nmpc_solver.cpp:351-482) for B planners, asynchronous on `stream`, nothing touching the host:
        stage references (f-4) -> tube (f-2) -> corridor (f-3) -> parameter packing (f-1) -> NLP solve -> result
        bookkeeping.  ref_pos [B,N,3] / ref_yaw [B,N] are caller-owned scratch that receives the references.
        With coldstart (default) planners whose previous solve failed first restart from the constant plan (:363-364).
        cloud [B,P,3] with cloud_count [B]: per-planner clouds, as OccupancyMap.local_view exports them; or the shared cloud and grid
        of OccupancyMap.shared_view() with cut = OccupancyMap.cut(local_box): the same polytopes without the per-planner copies; or
        cloud = None and view = a SharedView (OccupancyMap.shared_view_device) updated on this stream, with the same cut: the same
        again for a map that changes every tick.
        tick: a TickState -- the whole of solveNMPC with its decisions (include/frp_nmpc_outcome.h), state [B,9] and end_pt ([3] or [B,3])
        required: tick_begin -> cold start of the planners tick.keep names -> references (their flag goes to tick.ref_replan; `replan`
        is not used) -> tube -> corridor -> pack -> solve -> tick_end -> update of the planners tick.accept names ->
        snapshot_commands(accept=tick.accept).  Planners that do not run this tick (tick.gate != TICK_RUN) stay in the batch: it remains
        one launch of every stage, their solve is discarded and neither their plan nor their state changes.  With a fleet that carries
        modes, tick_end applies the switch rule (update_mode is not needed).  tick.reset_output, when set, is consumed by tick_begin."""
        if tick is not None:
            return self._full_tick_outcome(tick, external_acc, kino_path, time_offset, cloud, ref_pos, ref_yaw, stream, kino_size, tube_consts,
                                           corridor_consts, Ts, state, grid, cloud_count, cut, view, end_pt)
        if coldstart:
            self.coldstart(state, True, stream=stream)
        self.references(kino_path, time_offset, ref_pos, ref_yaw, replan, kino_size, Ts, stream)
        self.tube(tube_consts, stream)
        self.corridor(cloud, ref_pos, ref_yaw, corridor_consts, stream, cloud_count=cloud_count, grid=grid, cut=cut, view=view)
        self.pack(external_acc, ref_pos, ref_yaw, stream)
        self.solver.solve(stream)
        self.update(stream)

    def _full_tick_outcome(self, tick, external_acc, kino_path, time_offset, cloud, ref_pos, ref_yaw, stream, kino_size, tube_consts, corridor_consts,
                           Ts, state, grid, cloud_count, cut, view, end_pt):
        assert state is not None and end_pt is not None, "full_tick(tick=...) needs the odometry `state` and the goal `end_pt`"
        tick.begin(tick.reset_output, stream)
        self.coldstart(state, True, stream=stream, keep=tick.keep)
        self.references(kino_path, time_offset, ref_pos, ref_yaw, tick.ref_replan, kino_size, Ts, stream)
        self.tube(tube_consts, stream)
        self.corridor(cloud, ref_pos, ref_yaw, corridor_consts, stream, cloud_count=cloud_count, grid=grid, cut=cut, view=view)
        self.pack(external_acc, ref_pos, ref_yaw, stream)
        self.solver.solve(stream)
        ds = self.solver
        tick.end(ds.z, ds.exitflag, self.mpc_output, state, end_pt, kino_path, kino_size if kino_size is not None else tick.path_size(kino_path.shape[-2]),
                 time_offset, Ts=Ts, mode=self.mode, stream=stream)
        self.update(stream, accept=tick.accept)
        self.snapshot_commands(accept=tick.accept, stream=stream)

    def tick(self, external_acc, ref_pos, ref_yaw, stream=None, tube_consts=None, propagate_tube=False):
        """One receding-horizon tick of all B planners, asynchronous on `stream`.  With propagate_tube the
        tube matrices are recomputed from the current plans first, as the reference does every tick."""
        if propagate_tube:
            self.tube(tube_consts, stream)
        self.pack(external_acc, ref_pos, ref_yaw, stream)
        self.solver.solve(stream)
        self.update(stream)

    def _command_buffers(self):
        t = self.torch
        ds = self.solver
        if getattr(self, "pre_plan", None) is None:
            self.pre_plan = t.zeros((self.B, self.N, L.NZ), dtype=t.float64, device=ds.device)
            self.have_traj = t.zeros((self.B,), dtype=t.int32, device=ds.device)
            self._accept = t.zeros((self.B,), dtype=t.int32, device=ds.device)       # the default mask, and
            self._accept_bool = t.zeros((self.B,), dtype=t.bool, device=ds.device)   # the comparison it is converted from

    def snapshot_commands(self, accept=None, stream=None):
        """pre_mpc_output_ = mpc_output_; have_mpc_traj_ = true (nmpc_solver.cpp:527-528) for the planners whose last solve is accepted:
        self.pre_plan [B,N,17] <- solver.z, self.have_traj [B] <- 1 there; every other planner keeps both.  Both tensors belong to the
        fleet and are allocated (zeros: no trajectory yet) on first use -- call once outside a graph capture.
        pre_plan is NOT mpc_output: the reference copies before it wraps the yaw and duplicates the last row (:527 against :531-543).
        accept [B] int32, non-zero = accepted.  None: solver.exitflag == 1, which is only the FIRST branch of the reference's rule
        (:398-421): it also accepts a MAXIT result after repeated failures (replan_count_ > 3 && exit_code == 0).  TickState.accept is
        the whole rule, computed on the device (full_tick(tick=...) passes it); any other policy is the caller's own mask."""
        t = self.torch
        ds = self.solver
        s = stream if stream is not None else t.cuda.current_stream(ds.device)
        self._command_buffers()
        if accept is None:
            with t.cuda.stream(s):
                t.eq(ds.exitflag, 1, out=self._accept_bool)
                self._accept.copy_(self._accept_bool)
            accept = self._accept
        command_snapshot_device(ds.z, accept, self.pre_plan, self.have_traj, s)

    def commands(self, t_cur, status, pub_end, end_pt, odom=None, init_yaw=None, t_yaw=None, out=None, stream=None, Ts=None, mass=None, g=None):
        """The 100 Hz command timer (NMPCSolver::cmdTrajCallback, nmpc_solver.cpp:865-987) for all B planners: S = t_cur.shape[1]
        consecutive callbacks sampled from the snapshot of snapshot_commands(), in one launch -- command_batch_device has the arguments.
        t_cur counts from pre_mpc_start_time_, which the reference resets at EVERY solveNMPC call (:359), rejected ones included."""
        assert getattr(self, "pre_plan", None) is not None, "call snapshot_commands() first: it owns pre_plan / have_traj"
        return command_batch_device(self.pre_plan, self.have_traj, t_cur, status, pub_end, end_pt, odom, init_yaw, t_yaw, out, Ts, mass, g, stream)
