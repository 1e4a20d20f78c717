"""The statement of the fleet peers (include/frp_nmpc.h section 18) in NumPy: brute force over all pairs, no grid.  The box decides who is
ENTERED and nothing else.  Every product and sum is a float64 operation of its own, in the header's order, so the device (built without
contraction) gives the same bits.  `count` (a collections.Counter or None) takes one tick per named branch."""
import numpy as np

MAX_NEAR = 64
I_NEAREST, I_WITH_HITS, I_NEAR, I_HIT, I_SAMPLES = range(5)
INT_FIELDS = ("nearest", "near_samples", "hit_samples", "samples")
FIELDS = ("sep2_min",) + INT_FIELDS + ("first_hit",)
BRANCHES_SEPARATION = ("entered", "nonfinite", "outside_box", "inactive", "no_peer", "peer", "tie_lowest_id", "replaced", "equal_not_replaced",
                       "larger_not_replaced", "near", "hit", "first_hit_set", "first_hit_kept", "peer_beyond_warn")
BRANCHES_CLOUD = ("count_negative", "not_entered", "no_peer", "peer", "more_than_64", "peer_no_traj", "peer_with_traj", "k0", "k8", "r_body_zero",
                  "r_body_seven", "point_nonfinite", "cut_lo_x", "cut_lo_y", "cut_lo_z", "cut_hi_x", "cut_hi_y", "cut_hi_z", "stored", "exact_fill",
                  "overflow_p")


def _tick(count, name):
    if count is not None:
        count[name] += 1


def entered(pos, origin, dims, cell, active=None, count=None):
    """bool [B,S]: sample (b, s) of pos [B,S,>=3] is finite, its cell (int)floor((p - origin) / cell) is inside dims, and b is active."""
    pos = np.asarray(pos, dtype=np.float64)
    B, S = pos.shape[:2]
    out = np.zeros((B, S), dtype=bool)
    for b in range(B):
        for s in range(S):
            if active is not None and active[b] == 0:
                _tick(count, "inactive")
                continue
            p = pos[b, s, :3]
            if not np.all(np.abs(p) <= 1.7976931348623157e308):
                _tick(count, "nonfinite")
                continue
            f = np.floor((p - np.asarray(origin, dtype=np.float64)) / np.float64(cell))
            if not all(0.0 <= f[k] < float(dims[k]) for k in range(3)):
                _tick(count, "outside_box")
                continue
            _tick(count, "entered")
            out[b, s] = True
    return out


def dist2(P):
    """D2[b, q] = (dx * dx + dy * dy) + dz * dz with d = P[b] - P[q], P [B,3]."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = P[:, None, :] - P[None, :, :]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def new_record(B, R):
    R = np.float64(R)
    return dict(sep2_min=np.full((B,), R * R, dtype=np.float64), nearest=np.full((B,), -1, dtype=np.int32), near_samples=np.zeros((B,), dtype=np.int32),
                hit_samples=np.zeros((B,), dtype=np.int32), samples=np.zeros((B,), dtype=np.int32), first_hit=np.full((B,), -1, dtype=np.int64))


def reset(rec, R, mask=None):
    fresh = new_record(len(rec["samples"]), R)
    sel = np.ones(len(rec["samples"]), dtype=bool) if mask is None else np.asarray(mask) != 0
    for f in FIELDS:
        rec[f][sel] = fresh[f][sel]


def separation(rec, pos, ent, R, d_warn, d_hit, tick, advance=1, count=None):
    """One call on pos [B,S,>=3] with ent = entered(...): the record in place; returns the counter after the call."""
    pos = np.asarray(pos, dtype=np.float64)
    B, S = ent.shape
    R2, w2, h2 = np.float64(R) * np.float64(R), np.float64(d_warn) * np.float64(d_warn), np.float64(d_hit) * np.float64(d_hit)
    for s in range(S):
        D2 = dist2(pos[:, s, :3])
        for b in range(B):
            if not ent[b, s]:
                continue
            rec["samples"][b] += 1
            with np.errstate(invalid="ignore"):
                q = np.nonzero(ent[:, s] & (np.arange(B) != b) & (D2[b] <= R2))[0]
            if q.size == 0:
                _tick(count, "no_peer")
                continue
            _tick(count, "peer")
            dd = D2[b, q]
            m = dd.min()
            at = q[dd == m]
            if at.size > 1:
                _tick(count, "tie_lowest_id")
            if m < rec["sep2_min"][b]:
                _tick(count, "replaced")
                rec["sep2_min"][b], rec["nearest"][b] = m, at[0]
            else:
                _tick(count, "equal_not_replaced" if m == rec["sep2_min"][b] else "larger_not_replaced")
            if (dd <= w2).any():
                _tick(count, "near")
                rec["near_samples"][b] += 1
            else:
                _tick(count, "peer_beyond_warn")
            if (dd <= h2).any():
                _tick(count, "hit")
                rec["hit_samples"][b] += 1
                if rec["first_hit"][b] < 0:
                    _tick(count, "first_hit_set")
                    rec["first_hit"][b] = tick
                else:
                    _tick(count, "first_hit_kept")
    return tick + advance


def summary(rec, mask=None):
    """(out_i [5] int64, out_f [1] float64) over the vehicles with mask != 0."""
    B = len(rec["samples"])
    sel = np.ones(B, dtype=bool) if mask is None else np.asarray(mask) != 0
    out_i, out_f = np.zeros((5,), dtype=np.int64), np.full((1,), np.inf)
    out_i[I_NEAREST] = -1
    if sel.any():
        ids = np.nonzero(sel)[0]
        m = rec["sep2_min"][ids].min()
        out_f[0], out_i[I_NEAREST] = m, ids[rec["sep2_min"][ids] == m][0]
    out_i[I_WITH_HITS] = int((rec["hit_samples"][sel] > 0).sum())
    out_i[I_NEAR], out_i[I_HIT], out_i[I_SAMPLES] = (int(rec[f][sel].astype(np.int64).sum()) for f in ("near_samples", "hit_samples", "samples"))
    return out_i, out_f


def cloud(state, ent, pre_plan, have_traj, stages, r_body, R, local_box, map_origin, resolution, cloud, cloud_count, count=None):
    """The peer cloud of every planner: state [B,>=3] the current positions, ent [B] = entered(state[:, None])[:, 0].  cloud [B,P,3] and
    cloud_count [B] in place; returns (added [B] int32, overflow [B] int32)."""
    state = np.asarray(state, dtype=np.float64)
    B, P, N = state.shape[0], cloud.shape[1], pre_plan.shape[1]
    R2, r = np.float64(R) * np.float64(R), np.float64(r_body)
    o, res = np.asarray(map_origin, dtype=np.float64), np.float64(resolution)
    D2 = dist2(state[:, :3])
    added, overflow = np.zeros((B,), dtype=np.int32), np.zeros((B,), dtype=np.int32)
    _tick(count, "k0" if len(stages) == 0 else "k8" if len(stages) == 8 else "k_other")
    _tick(count, "r_body_zero" if r == 0.0 else "r_body_seven")
    for b in range(B):
        cc = int(cloud_count[b])
        if cc < 0:
            _tick(count, "count_negative")
            continue
        if not ent[b]:
            _tick(count, "not_entered")
            continue
        with np.errstate(invalid="ignore"):
            q = np.nonzero(ent & (np.arange(B) != b) & (D2[b] <= R2))[0]
        if q.size == 0:
            _tick(count, "no_peer")
            continue
        _tick(count, "peer")
        q = q[np.lexsort((q, D2[b, q]))]            # ascending in (d2, id)
        if q.size > MAX_NEAR:
            _tick(count, "more_than_64")
            overflow[b] = 1
            q = q[:MAX_NEAR]
        lo = o + local_box[b, :3].astype(np.float64) * res
        hi = o + local_box[b, 3:].astype(np.float64) * res
        pts = []
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
                cands = [np.array(c, dtype=np.float64)]
                if r != 0.0:
                    for axis in range(3):
                        for sign in (1, -1):
                            v = np.array(c, dtype=np.float64)
                            v[axis] = v[axis] + r if sign > 0 else v[axis] - r
                            cands.append(v)
                for v in cands:
                    if not np.all(np.abs(v) <= 1.7976931348623157e308):
                        _tick(count, "point_nonfinite")
                        continue
                    cut = [("cut_lo_" + "xyz"[k]) for k in range(3) if not lo[k] <= v[k]] + [("cut_hi_" + "xyz"[k]) for k in range(3) if not v[k] < hi[k]]
                    if cut:
                        for name in cut:
                            _tick(count, name)
                        continue
                    pts.append(v)
        n = len(pts)
        added[b] = n
        if cc + n > P:
            _tick(count, "overflow_p")
            cloud_count[b] = -(cc + n)
            continue
        if n:
            _tick(count, "stored")
            cloud[b, cc:cc + n] = np.array(pts)
        if cc + n == P and n:
            _tick(count, "exact_fill")
        cloud_count[b] = cc + n
    return added, overflow
