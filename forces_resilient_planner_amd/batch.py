"""The batched NLP solve: host arrays through frp_nmpc_solve_batch_host* (with the pinned-page registry), device tensors through
DeviceSolver, and the kernel timing around either.

Every function here runs HIP kernels on the MI355X; there is no CPU fallback: a missing library or device raises.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import layout as L
from .capi import INFO_STRIDE, Batch, Options, _check, c_double_p, lib, stream_ptr


def default_options(**kw) -> Options:
    o = Options()
    lib().frp_nmpc_default_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def solve_batch_host(w, opt: Options | None = None, MF: int | None = None, x0=None, out=None):
    """Solve a workload dict (host numpy arrays) on the GPU through frp_nmpc_solve_batch_host.
    out: (z, flag, iters, info) arrays of an earlier call to write into (a caller in a loop does not re-allocate)."""
    B, N, M = int(w["xinit"].shape[0]), int(w["N"]), int(w["M"])
    xinit = np.ascontiguousarray(w["xinit"], dtype=np.float64)
    z0 = np.ascontiguousarray(w["x0"] if x0 is None else x0, dtype=np.float64)
    params = np.ascontiguousarray(w["params"], dtype=np.float64)
    nf = None if w.get("nfaces") is None else np.ascontiguousarray(w["nfaces"], dtype=np.int32)
    if MF is None:
        MF = int(nf.max()) if nf is not None and nf.size else M
    if out is not None:
        z, flag, iters, info = out
    else:
        z = np.zeros((B, N, L.NZ)); flag = np.zeros(B, dtype=np.int32); iters = np.zeros(B, dtype=np.int32)
        info = np.zeros((B, INFO_STRIDE))
    models = None if w.get("models") is None else np.ascontiguousarray(w["models"], dtype=np.int32)  # per-problem normal / final
    b = Batch(B, N, M, MF, int(w["model"]), xinit.ctypes.data, z0.ctypes.data, params.ctypes.data,
              nf.ctypes.data if nf is not None else None, z.ctypes.data, flag.ctypes.data, iters.ctypes.data,
              info.ctypes.data, models.ctypes.data if models is not None else None)
    _check(lib().frp_nmpc_solve_batch_host(ctypes.byref(b), ctypes.byref(opt) if opt is not None else None),
           "frp_nmpc_solve_batch_host")
    return z, flag, iters, info


def solver_variant(B, N, M, MF, model, opt: Options | None = None) -> str:
    """The kernel instantiation a solve of B problems of this shape would launch now (frp_nmpc_solver_variant), e.g.
    "frp::lr::nmpc_ipm_lds_kernel<20, 2, true, 3, false>".  The selection never reads the batch's arrays: any non-NULL
    address stands in for them."""
    one = 8
    b = Batch(B, N, M, MF, model, one, one, one, None, one, one, one, None, None)
    buf = ctypes.create_string_buffer(128)
    _check(lib().frp_nmpc_solver_variant(ctypes.byref(b), ctypes.byref(opt) if opt is not None else None, buf, len(buf)),
           "frp_nmpc_solver_variant")
    return buf.value.decode()


def solve_batch_host_begin(w, out, opt: Options | None = None, MF: int | None = None):
    """frp_nmpc_solve_batch_host_begin: every array of `w` (C-contiguous float64 / int32) and of `out` = (z, flag, iters, info) registered with
    host_register; returns the ticket.  The outputs are valid after solve_batch_host_wait(ticket)."""
    B, N, M = int(w["xinit"].shape[0]), int(w["N"]), int(w["M"])
    nf = w.get("nfaces")
    if MF is None:
        MF = int(nf.max()) if nf is not None and nf.size else M
    z, flag, iters, info = out
    models = w.get("models")
    for a in (w["xinit"], w["x0"], w["params"], z, info):
        assert a.flags["C_CONTIGUOUS"] and a.dtype == np.float64
    for a in (nf, models, flag, iters):
        assert a is None or (a.flags["C_CONTIGUOUS"] and a.dtype == np.int32)
    b = Batch(B, N, M, MF, int(w["model"]), w["xinit"].ctypes.data, w["x0"].ctypes.data, w["params"].ctypes.data,
              nf.ctypes.data if nf is not None else None, z.ctypes.data, flag.ctypes.data, iters.ctypes.data,
              info.ctypes.data, models.ctypes.data if models is not None else None)
    t = ctypes.c_int(-1)
    _check(lib().frp_nmpc_solve_batch_host_begin(ctypes.byref(b), ctypes.byref(opt) if opt is not None else None, ctypes.byref(t)),
           "frp_nmpc_solve_batch_host_begin")
    return int(t.value)


def solve_batch_host_wait(ticket):
    _check(lib().frp_nmpc_solve_batch_host_wait(int(ticket)), "frp_nmpc_solve_batch_host_wait")


_registered = {}  # ptr -> [array, count]: a strong reference for as long as the library holds the pages pinned under that address


def host_register(*arrays):
    """frp_nmpc_host_register for numpy arrays a caller reuses from call to call (inputs and the `out` arrays of solve_batch_host):
    with every array of a call registered, frp_nmpc_solve_batch_host stages nothing.  The wrapper keeps a reference to every
    registered array until host_unregister: an array that were garbage-collected while registered would leave its address range
    in the library's registry, and a later array placed at the same address would be taken for the old mapping."""
    for a in arrays:
        if a is not None:
            assert a.flags["C_CONTIGUOUS"]
            _check(lib().frp_nmpc_host_register(a.ctypes.data, a.nbytes), "frp_nmpc_host_register")
            ent = _registered.setdefault(a.ctypes.data, [a, 0])
            ent[1] += 1


def host_unregister(*arrays):
    for a in arrays:
        if a is not None:
            _check(lib().frp_nmpc_host_unregister(a.ctypes.data), "frp_nmpc_host_unregister")
            ent = _registered.get(a.ctypes.data)
            if ent is not None:
                ent[1] -= 1
                if ent[1] <= 0:
                    del _registered[a.ctypes.data]


def host_unregister_all():
    _check(lib().frp_nmpc_host_unregister_all(), "frp_nmpc_host_unregister_all")
    _registered.clear()


def stage_eval_host(z, params, M, model, want=("f", "gf", "c", "Jc", "h")):
    z = np.ascontiguousarray(z, dtype=np.float64); params = np.ascontiguousarray(params, dtype=np.float64)
    B, N = z.shape[0], z.shape[1]
    out = dict(f=np.zeros((B, N)), gf=np.zeros((B, N, 17)), c=np.zeros((B, N, 13)), Jc=np.zeros((B, N, 221)),
               h=np.zeros((B, N, max(M, 1))))
    ptr = lambda k: out[k].ctypes.data_as(c_double_p) if k in want else None
    _check(lib().frp_nmpc_stage_eval_host(B, N, M, model, z.ctypes.data_as(c_double_p), params.ctypes.data_as(c_double_p),
                                          ptr("f"), ptr("gf"), ptr("c"), ptr("Jc"), ptr("h")), "frp_nmpc_stage_eval_host")
    return out


class DeviceSolver:
    """Device-resident batched solver: torch tensors hold the HBM buffers, the C-ABI gets raw pointers."""

    def __init__(self, B, N, M, MF, model, device="cuda:0"):
        import torch
        self.torch = torch
        self.B, self.N, self.M, self.MF, self.model = B, N, M, MF, model
        self.device = torch.device(device)
        f64 = dict(dtype=torch.float64, device=self.device)
        self.xinit = torch.empty((B, L.NX), **f64)
        self.x0 = torch.empty((B, N, L.NZ), **f64)
        self.params = torch.empty((B, N, L.npar(M)), **f64)
        self.nfaces = torch.empty((B, N), dtype=torch.int32, device=self.device)
        self.z = torch.zeros((B, N, L.NZ), **f64)
        # zero = "no solve yet / MAXIT": DeviceFleet's cold start and update branch on exitflag == 1 before the first solve has
        # written it, so a fresh solver must not expose recycled allocator memory (the reference's !initialized_output_)
        self.exitflag = torch.zeros((B,), dtype=torch.int32, device=self.device)
        self.iters = torch.zeros((B,), dtype=torch.int32, device=self.device)
        self.info = torch.empty((B, INFO_STRIDE), **f64)
        self.ws_bytes = int(lib().frp_nmpc_workspace_bytes(B, N, MF))
        self.ws = torch.empty((self.ws_bytes // 8 + 1,), **f64)
        self.use_nfaces = True
        # receding-horizon callers: queue the problems by the PREVIOUS solve's iteration counts (frp_nmpc_batch.order_hint);
        # off = by the objective of the initial guess
        self.order_by_last_iters = False
        self.opt = default_options()

    def upload(self, w):
        t = self.torch
        self._packed_by = None  # (a fleet's pack may no longer assume what it left in params / nfaces)
        self.xinit.copy_(t.from_numpy(np.ascontiguousarray(w["xinit"])))
        self.x0.copy_(t.from_numpy(np.ascontiguousarray(w["x0"])))
        self.params.copy_(t.from_numpy(np.ascontiguousarray(w["params"])))
        self.nfaces.copy_(t.from_numpy(np.ascontiguousarray(w["nfaces"], dtype=np.int32)))

    def _batch(self, lo=0, hi=None):
        """The problems [lo, hi) of this solver's buffers as a frp_nmpc_batch (the whole batch by default)."""
        hi = self.B if hi is None else hi
        models = getattr(self, "models", None)
        return Batch(hi - lo, self.N, self.M, self.MF, self.model, self.xinit[lo:].data_ptr(), self.x0[lo:].data_ptr(),
                     self.params[lo:].data_ptr(), self.nfaces[lo:].data_ptr() if self.use_nfaces else None, self.z[lo:].data_ptr(),
                     self.exitflag[lo:].data_ptr(), self.iters[lo:].data_ptr(), self.info[lo:].data_ptr(),
                     models[lo:].data_ptr() if models is not None else None,
                     self.iters[lo:].data_ptr() if self.order_by_last_iters else None)

    def solve_range(self, lo, hi, stream=None, piece=0):
        """Solve the problems [lo, hi) of the batch only (a piece of a shard whose later pieces are still arriving):
        asynchronous on `stream`.  Pieces that may run at the same time (different streams) pass different `piece` numbers:
        each gets a queue workspace of its own (the work-queue head lives there)."""
        if hi <= lo:
            return
        if not hasattr(self, "_piece_ws"):
            self._piece_ws = {}
        if piece not in self._piece_ws:
            self._piece_ws[piece] = self.ws if piece == 0 else self.torch.empty_like(self.ws)
        ws = self._piece_ws[piece]
        b = self._batch(lo, hi)
        _check(lib().frp_nmpc_solve_batch(ctypes.byref(b), ctypes.byref(self.opt), ws.data_ptr(), self.ws_bytes,
                                          stream_ptr(stream, self.device)), "frp_nmpc_solve_batch")

    def solve(self, stream=None):
        """Asynchronous launch on `stream` (a torch.cuda.Stream) or torch's current stream."""
        b = self._batch()
        _check(lib().frp_nmpc_solve_batch(ctypes.byref(b), ctypes.byref(self.opt), self.ws.data_ptr(), self.ws_bytes,
                                          stream_ptr(stream, self.device)), "frp_nmpc_solve_batch")

    def time_solve(self, reps, stream=None):
        """Average kernel duration (ms) over `reps` launches, HIP events on the launch stream."""
        b = self._batch()
        ms = ctypes.c_float(0)
        _check(lib().frp_nmpc_time_solve(ctypes.byref(b), ctypes.byref(self.opt), self.ws.data_ptr(), self.ws_bytes,
                                         stream_ptr(stream, self.device), reps, ctypes.byref(ms)), "frp_nmpc_time_solve")
        return ms.value


def kernel_timing_begin(max_launches, stride=1):
    """From here to kernel_timing_end() every `stride`-th solve launch carries a hipEvent pair around its dominant kernel (on its own stream)."""
    _check(lib().frp_nmpc_kernel_timing_begin(int(max_launches), int(stride)), "frp_nmpc_kernel_timing_begin")


def kernel_timing_end():
    """(average ms of the dominant kernel over the launches since kernel_timing_begin, number of launches)."""
    ms, n = ctypes.c_float(0), ctypes.c_int(0)
    _check(lib().frp_nmpc_kernel_timing_end(ctypes.byref(ms), ctypes.byref(n)), "frp_nmpc_kernel_timing_end")
    return ms.value, n.value
