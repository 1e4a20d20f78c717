"""The statement of peer avoidance (include/frp_nmpc.h section 19) in NumPy: a planner's peers as boxes of map voxels, brute force over all
pairs, the path walk against them, and the world a planner's A* searches (the map with its boxes written into occ).  The peers and their
order are tests/peers_oracle.py's cloud rule.  Every difference, sum and product is a float64 operation of its own, in the header's
order, so the device (built without contraction) gives the same bits.  `count` (a collections.Counter or None) takes one tick per
named branch."""
import numpy as np

from . import peers_oracle as PO

MAX_NEAR = PO.MAX_NEAR
BRANCHES = ("not_entered", "no_peer", "peer", "more_than_64", "peer_no_traj", "peer_with_traj", "stage_outside", "k0", "k8", "half_zero", "nonfinite",
            "outside_map", "own_voxel", "clip_lo_x", "clip_lo_y", "clip_lo_z", "clip_hi_x", "clip_hi_y", "clip_hi_z", "kept", "exact_fill", "overflow_q")
BRANCHES_WALK = ("no_traj", "no_boxes", "sample_outside_map", "sample_free", "sample_hit", "clean")
FINITE = 1.7976931348623157e308


def _tick(count, name):
    if count is not None:
        count[name] += 1


def voxel_f(x, origin, inv):
    """floor((x - origin) * inv): posToIndex before its conversion, one rounding each."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor((np.float64(x) - np.float64(origin)) * np.float64(inv))


def boxes(state, ent, pre_plan, have_traj, stages, half, R, origin, resolution, grid, Q, count=None):
    """state [B,>=3], ent [B] = peers_oracle.entered(state[:, None])[:, 0].  Returns (boxes [B,Q,6] int32 -- rows past a count are zero --,
    count [B], overflow [B], dropped_own [B]) int32."""
    state = np.asarray(state, dtype=np.float64)
    B, N = state.shape[0], pre_plan.shape[1]
    R2 = np.float64(R) * np.float64(R)
    inv = np.float64(1.0) / np.float64(resolution)
    half = np.asarray(half, dtype=np.float64)
    D2 = PO.dist2(state[:, :3])
    out = np.zeros((B, Q, 6), dtype=np.int32)
    cnt, overflow, dropped = (np.zeros((B,), dtype=np.int32) for _ in range(3))
    _tick(count, "k0" if len(stages) == 0 else "k8" if len(stages) == 8 else "k_other")
    if not half.any():
        _tick(count, "half_zero")
    for b in range(B):
        if not ent[b]:
            _tick(count, "not_entered")
            continue
        with np.errstate(invalid="ignore"):
            q = np.nonzero(ent & (np.arange(B) != b) & (D2[b] <= R2))[0]
        if q.size == 0:
            _tick(count, "no_peer")
            continue
        _tick(count, "peer")
        q = q[np.lexsort((q, D2[b, q]))]
        if q.size > MAX_NEAR:
            _tick(count, "more_than_64")
            overflow[b] = 1
            q = q[:MAX_NEAR]
        own = [voxel_f(state[b, k], origin[k], inv) for k in range(3)]
        rows = []
        for p in q:
            centres = [state[p, :3]]
            if have_traj[p] != 0:
                _tick(count, "peer_with_traj")
                for st in stages:
                    if 0 <= st < N:
                        centres.append(pre_plan[p, st, 8:11])
                    else:
                        _tick(count, "stage_outside")
            else:
                _tick(count, "peer_no_traj")
            for c in centres:
                with np.errstate(invalid="ignore", over="ignore"):
                    lo = [voxel_f(np.float64(c[k]) - half[k], origin[k], inv) for k in range(3)]
                    hi = [voxel_f(np.float64(c[k]) + half[k], origin[k], inv) for k in range(3)]
                if not all(abs(v) <= FINITE for v in lo + hi):
                    _tick(count, "nonfinite")
                    continue
                if any(hi[k] < 0.0 or lo[k] > float(grid[k] - 1) for k in range(3)):
                    _tick(count, "outside_map")
                    continue
                if all(lo[k] <= own[k] <= hi[k] for k in range(3)):
                    _tick(count, "own_voxel")
                    dropped[b] += 1
                    continue
                row = []
                for k in range(3):
                    if lo[k] < 0.0:
                        _tick(count, "clip_lo_" + "xyz"[k])
                    row.append(0 if lo[k] < 0.0 else int(lo[k]))
                for k in range(3):
                    if hi[k] > float(grid[k] - 1):
                        _tick(count, "clip_hi_" + "xyz"[k])
                    row.append(grid[k] - 1 if hi[k] > float(grid[k] - 1) else int(hi[k]))
                rows.append(row)
        n = len(rows)
        if n > Q:
            _tick(count, "overflow_q")
            cnt[b] = -n
            continue
        if n:
            _tick(count, "kept")
            out[b, :n] = np.array(rows, dtype=np.int32)
        if n == Q and n:
            _tick(count, "exact_fill")
        cnt[b] = n
    return out, cnt, overflow, dropped


def rows_of(bx, cnt, b):
    """The rows both consumers read of planner b: none for a count below 1, never more than Q."""
    n = int(cnt[b])
    return bx[b, :min(n, bx.shape[1])] if n >= 1 else bx[b, :0]


def check_paths(bx, cnt, kino_path, kino_size, have_traj, stride, origin, resolution, grid, count=None):
    """first_hit [B] int32: the smallest sample index 0, stride, ... < min(kino_size, K) whose voxel, inside the map, lies in a box; -1."""
    B, K = kino_path.shape[:2]
    inv = np.float64(1.0) / np.float64(resolution)
    out = np.full((B,), -1, dtype=np.int32)
    for b in range(B):
        n = min(int(kino_size[b]), K)
        if have_traj is not None and have_traj[b] == 0:
            _tick(count, "no_traj")
            continue
        rows = rows_of(bx, cnt, b)
        if len(rows) == 0:
            _tick(count, "no_boxes")
            continue
        for s in range(0, n, stride):
            f = [voxel_f(kino_path[b, s, k], origin[k], inv) for k in range(3)]
            if not all(0.0 <= f[k] <= float(grid[k] - 1) for k in range(3)):
                _tick(count, "sample_outside_map")
                continue
            i = [int(v) for v in f]
            if any(all(r[k] <= i[k] <= r[3 + k] for k in range(3)) for r in rows):
                _tick(count, "sample_hit")
                out[b] = s
                break
            _tick(count, "sample_free")
        else:
            _tick(count, "clean")
    return out


def world_with_boxes(world, rows):
    """A copy of an A* world with the boxes' voxels occupied: what planner b's overlay search searches."""
    w = dict(world)
    occ = np.array(world["occ"], dtype=np.uint8, copy=True)
    g = occ.shape
    for r in rows:
        lo = [max(int(r[k]), 0) for k in range(3)]
        hi = [min(int(r[3 + k]), g[k] - 1) for k in range(3)]
        if all(lo[k] <= hi[k] for k in range(3)):
            occ[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = 1
    w["occ"] = occ
    return w


def plan_with_boxes(world, q, bx, cnt, init=True, local_box=None, cap=2048):
    """oracle/astar_oracle.c per planner (B = 1 through tests/astar_lib.plan_batch) on that planner's world; the fields of plan_batch."""
    from . import astar_lib as AL
    B = q["start_pt"].shape[0]
    outs = []
    for b in range(B):
        w = world_with_boxes(world, rows_of(bx, cnt, b))
        sl = slice(b, b + 1)
        outs.append(AL.plan_batch(w, q["start_pt"][sl], q["start_v"][sl], q["start_a"][sl], q["end_pt"][sl], q["end_v"][sl], q["f_ext"][sl], init=init, cap=cap,
                                  local_box=None if local_box is None else np.asarray(local_box)[sl]))
    return dict(status=np.concatenate([o["status"] for o in outs]), kino_path=np.concatenate([o["kino_path"] for o in outs]),
                kino_size=np.concatenate([o["kino_size"] for o in outs]), retried=np.concatenate([o["retried"] for o in outs]),
                results=[o["results"][0] for o in outs], _keep=outs)
