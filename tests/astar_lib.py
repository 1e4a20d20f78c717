"""ctypes loader for the kinodynamic-A* oracle (oracle/astar_oracle.c in liboracle.so) -- test infrastructure only."""
import ctypes

import numpy as np

from . import oracle_lib as OL

D = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int)
MAX_PATH = 256


class AstarParams(ctypes.Structure):
    _fields_ = [("occ", ctypes.c_void_p), ("grid", ctypes.c_int * 3), ("origin", ctypes.c_double * 3), ("map_size", ctypes.c_double * 3),
                ("resolution", ctypes.c_double), ("use_local", ctypes.c_int), ("local_min", ctypes.c_int * 3), ("local_max", ctypes.c_int * 3),
                ("ego_r", ctypes.c_double), ("ego_h", ctypes.c_double),
                ("max_tau", ctypes.c_double), ("init_max_tau", ctypes.c_double), ("max_vel", ctypes.c_double), ("max_acc", ctypes.c_double),
                ("w_time", ctypes.c_double), ("horizon", ctypes.c_double), ("lambda_heu", ctypes.c_double),
                ("allocate_num", ctypes.c_int), ("check_num", ctypes.c_int), ("tie_breaker", ctypes.c_double), ("max_expand", ctypes.c_int)]


class AstarResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("use_node_num", ctypes.c_int), ("iter_num", ctypes.c_int), ("is_shot_succ", ctypes.c_int),
                ("n_path", ctypes.c_int), ("coef_shot", ctypes.c_double * 12), ("t_shot", ctypes.c_double),
                ("path_state", (ctypes.c_double * 6) * MAX_PATH), ("path_input", (ctypes.c_double * 3) * MAX_PATH),
                ("path_duration", ctypes.c_double * MAX_PATH), ("path_node", ctypes.c_int * MAX_PATH)]


def lib():
    l = OL.lib()
    for n in ("orc_det_cbrt", "orc_det_acos", "orc_det_cos"):
        getattr(l, n).restype = ctypes.c_double
        getattr(l, n).argtypes = [ctypes.c_double]
    return l


def make_params(world, local_box=None, max_expand=4096):
    """world: dict from forces_resilient_planner_amd.workloads.astar_world (occ uint8 [nx,ny,nz] + map / search constants).
    local_box: None, or the six ints (min_id, max_id) of isInLocalMap -- voxels outside read as free."""
    p = AstarParams()
    occ = np.ascontiguousarray(world["occ"], dtype=np.uint8)
    p._occ_keepalive = occ
    p.occ = occ.ctypes.data
    p.grid[:] = occ.shape; p.origin[:] = world["origin"]; p.map_size[:] = world["map_size"]; p.resolution = world["resolution"]
    p.use_local = 0
    if local_box is not None:
        p.use_local = 1
        p.local_min[:] = [int(v) for v in local_box[:3]]; p.local_max[:] = [int(v) for v in local_box[3:6]]
    p.ego_r = world["ego_r"]; p.ego_h = world["ego_h"]
    for k in ("max_tau", "init_max_tau", "max_vel", "max_acc", "w_time", "horizon", "lambda_heu", "allocate_num", "check_num", "tie_breaker"):
        setattr(p, k, world[k])
    p.max_expand = max_expand
    return p


def plan_batch(world, start_pt, start_v, start_a, end_pt, end_v, f_ext, init=True, Ts=0.05, cap=2048, nthreads=0, retry_pt=None, retry_v=None,
               local_box=None, max_expand=4096):
    """NMPCSolver::getKinoPath's search + getKinoTraj for B planners on the CPU oracle.
    local_box: None, or int [B,6] -- one box per planner (the oracle's use_local is per call: one call per distinct box).
    Returns dict(status [B], kino_path [B,cap,3], kino_size [B] (the UNTRUNCATED sample count; min(., cap) rows are stored),
    retried [B], results [B] AstarResult)."""
    B = start_pt.shape[0]
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    sp, sv, sa, ep, ev, fe = map(c, (start_pt, start_v, start_a, end_pt, end_v, f_ext))
    rp = c(retry_pt) if retry_pt is not None else None
    rv = c(retry_v) if retry_v is not None else None
    path = np.zeros((B, cap, 3)); size = np.zeros(B, dtype=np.int32); status = np.zeros(B, dtype=np.int32); retried = np.zeros(B, dtype=np.int32)
    res = (AstarResult * B)()

    def call(p, rows):
        n = len(rows)
        sub = [c(a[rows]) if a is not None else None for a in (sp, sv, sa, ep, ev, fe, rp, rv)]
        pth = np.zeros((n, cap, 3)); sz = np.zeros(n, dtype=np.int32); st = np.zeros(n, dtype=np.int32); rt = np.zeros(n, dtype=np.int32)
        r = (AstarResult * n)()
        lib().orc_astar_batch(n, ctypes.byref(p), OL.P(sub[0]), OL.P(sub[1]), OL.P(sub[2]), OL.P(sub[3]), OL.P(sub[4]), 1 if init else 0, OL.P(sub[5]),
                              ctypes.c_double(Ts), OL.P(pth), cap, sz.ctypes.data_as(IP), st.ctypes.data_as(IP), r, rt.ctypes.data_as(IP), nthreads,
                              OL.P(sub[6]), OL.P(sub[7]))
        for j, b in enumerate(rows):
            path[b] = pth[j]; size[b] = sz[j]; status[b] = st[j]; retried[b] = rt[j]
            ctypes.memmove(ctypes.byref(res[b]), ctypes.byref(r[j]), ctypes.sizeof(AstarResult))

    if local_box is None:
        call(make_params(world, None, max_expand), list(range(B)))
    else:
        boxes = np.asarray(local_box).reshape(B, 6)
        groups = {}
        for b in range(B):
            groups.setdefault(tuple(int(v) for v in boxes[b]), []).append(b)
        for box, rows in groups.items():
            call(make_params(world, box, max_expand), rows)
    return dict(status=status, kino_path=path, kino_size=size, retried=retried, results=res)


def kino_traj(world, f_ext, result, Ts=0.05, cap=2048):
    """orc_astar_kino_traj on one result: (pts [min(n, cap), 3], n) with n the untruncated sample count."""
    p = make_params(world)
    pts = np.zeros((cap, 3))
    fe = np.ascontiguousarray(f_ext, dtype=np.float64)
    l = lib()
    l.orc_astar_kino_traj.restype = ctypes.c_int
    n = l.orc_astar_kino_traj(ctypes.byref(p), OL.P(fe), ctypes.byref(result), ctypes.c_double(Ts), OL.P(pts), cap)
    return pts[:min(n, cap)].copy(), n


def quartic(a, b, c, d, e):
    """orc_astar_quartic: the roots quartic() reports, in the reference's order."""
    r = (ctypes.c_double * 4)()
    l = lib()
    l.orc_astar_quartic.restype = ctypes.c_int
    n = l.orc_astar_quartic(*(ctypes.c_double(v) for v in (a, b, c, d, e)), r)
    return [r[i] for i in range(n)]


def heuristic(x1, x2, w_time, max_vel, tie_breaker):
    """orc_astar_heuristic: (cost, optimal_time) of estimateHeuristic."""
    p = AstarParams()
    p.w_time = w_time; p.max_vel = max_vel; p.tie_breaker = tie_breaker
    a = np.ascontiguousarray(x1, dtype=np.float64); b = np.ascontiguousarray(x2, dtype=np.float64)
    t = ctypes.c_double(0.0)
    l = lib()
    l.orc_astar_heuristic.restype = ctypes.c_double
    cost = l.orc_astar_heuristic(ctypes.byref(p), OL.P(a), OL.P(b), ctypes.byref(t))
    return cost, t.value


def transit(ext, s0, um, tau):
    """orc_astar_transit: stateTransit of s0 [6] under input um and the external acceleration ext for tau."""
    s1 = np.zeros(6)
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    e, s, u = c(ext), c(s0), c(um)
    lib().orc_astar_transit(OL.P(e), OL.P(s), OL.P(u), ctypes.c_double(tau), OL.P(s1))
    return s1
