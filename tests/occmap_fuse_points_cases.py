"""The point scans and expected results that tests/test_occmap_fuse_points_cpu.py and tests/test_gpu_occmap_fuse_points.py share.  A scan
is (points [n, 3] float64 array, origin (x, y, z)); the expected map is always built the same way: a fresh FusionOracle on the start
values of tests/occmap_fusion_batch_cases.py, then FusionOracle.raycast(points with the non-finite rows removed, origin) for the
active, accepted scans in order.  The expected status of a scan is what raycast_relaxed gives for it: its round count and
stats["rays"].  Every chain is computed once per process and never modified."""
import functools

import numpy as np

from tests import occmap_fusion_batch_cases as BC
from tests import occmap_fusion_oracle as FO

NAN, INF = float("nan"), float("inf")
MIDDLE = FO.PLACEMENTS["middle"]


def oracle(**kw):
    om = FO.FusionOracle(**FO.TEST_GEO, **FO.LAUNCH_CLAMPS, **kw)
    om.buffer[...] = BC.start_values()
    return om


def finite_rows(points):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    return p[np.isfinite(p).all(axis=1)]


def widened(points):
    """What the device makes of a float32 scan: every coordinate rounded to float, then widened exactly."""
    return np.asarray(points, dtype=np.float64).astype(np.float32).astype(np.float64)


_RELAXED = {}


def relaxed(points, origin, **kw):
    """(rounds, rays) of one scan by rounds, and whether the rounds reach the serial scan's stops -- on a map of its own: neither
    depends on the map's values.  Computed once per scan and process."""
    key = (finite_rows(points).tobytes(), tuple(float(v) for v in origin), tuple(sorted(kw.items())))
    if key not in _RELAXED:
        _RELAXED[key] = _relaxed(points, origin, **kw)
    return _RELAXED[key]


def _relaxed(points, origin, **kw):
    pts = [tuple(float(v) for v in p) for p in finite_rows(points)]
    a, b = oracle(**kw), oracle(**kw)
    serial = a.raycast(pts, origin)
    stops, rounds = b.raycast_relaxed(pts, origin)
    same = stops == serial and a.buffer.tobytes() == b.buffer.tobytes() and a.box_skips == 0 and b.box_skips == 0
    return rounds, b.stats["rays"], same


def chain(scans, skip=(), cap=None, **kw):
    """The serial oracle over `scans` in the given order.  Scans whose index is in `skip` are left out (status None); with `cap`, a
    scan that needs more rounds is left out as well (status [-cap, rays]).  Returns (oracle, [status per scan])."""
    om = oracle(**kw)
    status = []
    for k, (points, origin) in enumerate(scans):
        if k in skip:
            status.append(None)
            continue
        rounds, rays, _ = relaxed(points, origin, **kw)
        if cap is not None and rounds > cap:
            status.append([-cap, rays])
            continue
        om.raycast([tuple(float(v) for v in p) for p in finite_rows(points)], origin)
        status.append([rounds, rays])
    assert om.box_skips == 0
    return om, status


def want(status):
    return [[0, 0] if s is None else s for s in status]


def pack(scans, P=None, tail=None, dtype=np.float64):
    """([S, P, 3] points, [S] int32 counts, [S, 3] origins) of scans with different lengths.  tail: what the storage beyond each
    scan's count holds (a [3] row; default NaN)."""
    P = max(len(p) for p, _ in scans) if P is None else P
    pts = np.empty((len(scans), P, 3), dtype=np.float64)
    pts[...] = NAN if tail is None else tail
    for k, (p, _) in enumerate(scans):
        pts[k, :len(p)] = p
    count = np.array([len(p) for p, _ in scans], dtype=np.int32)
    origin = np.array([o for _, o in scans], dtype=np.float64).reshape(len(scans), 3)
    return np.ascontiguousarray(pts.astype(dtype)), count, origin


# ---- 1. realistic scans: what the cameras of the fusion tests see, as clouds ----
REALISTIC = [(s, p) for s in FO.SCENES for p in FO.PLACEMENTS]


@functools.lru_cache(maxsize=None)
def realistic(scene, placement):
    T = FO.pose(FO.PLACEMENTS[placement])
    pts = np.array(oracle().project(FO.scene(scene), FO.TEST_K, T), dtype=np.float64).reshape(-1, 3)
    pts.setflags(write=False)
    return pts, tuple(float(v) for v in T[:3, 3])


@functools.lru_cache(maxsize=None)
def realistic_chain(scene, placement, as_float):
    pts, origin = realistic(scene, placement)
    return chain([(widened(pts) if as_float else pts, origin)])


@functools.lru_cache(maxsize=None)
def float_sensitive():
    """A scan whose map changes when its points are rounded to float: every coordinate sits 1e-10 m below a voxel face, where a
    float has a spacing of 1e-7 m and more, so rounding moves about every other coordinate onto or across its face."""
    rng = np.random.default_rng(5)
    k = np.c_[rng.integers(40, 60, 48), rng.integers(10, 55, 48), rng.integers(3, 30, 48)]
    pts = np.array(FO.TEST_GEO["origin"]) + k * 0.1 - 1e-10
    pts.setflags(write=False)
    return pts, MIDDLE


@functools.lru_cache(maxsize=None)
def float_sensitive_chain(as_float):
    pts, origin = float_sensitive()
    return chain([(widened(pts) if as_float else pts, origin)])


def realistic_scans():
    return [realistic(s, p) for s, p in REALISTIC]


@functools.lru_cache(maxsize=None)
def realistic_batch_chain():
    return chain(realistic_scans())


# ---- 2. the six camera frames of the batched depth tests as clouds ----
@functools.lru_cache(maxsize=None)
def six_scans():
    om = oracle()
    return [(np.array(om.project(d, BC.K, T), dtype=np.float64).reshape(-1, 3), tuple(float(v) for v in T[:3, 3])) for d, T in BC.six_frames()]


# ---- 3. edge sets, hand-built ----
def _in_voxel(rng, lo, n):
    """n points inside the voxel whose lower corner is lo (a multiple of the resolution away from the map's origin)."""
    return np.asarray(lo) + rng.uniform(0.004, 0.096, (n, 3))


@functools.lru_cache(maxsize=None)
def edge_sets():
    """{name: (points, origin)}.  The map is [-3.2, 3.2) x [-3.2, 3.2) x [0, 3.2) in voxels of 0.1; rays are 0.1 ... 6 m long."""
    rng = np.random.default_rng(41)
    real, mid = realistic("random", "middle")
    sets = {}
    sets["count 0"] = (np.zeros((0, 3)), mid)
    d = rng.normal(size=(40, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    sets["all closer than min_ray_length"] = (np.array(mid) + d * rng.uniform(0.0, 0.09, (40, 1)), mid)
    corner = (-3.0, -3.0, 0.25)
    far = np.c_[rng.uniform(1.8, 3.1, 60), rng.uniform(1.8, 3.1, 60), rng.uniform(0.3, 3.0, 60)]       # 6.8 m and more from the corner, inside the map
    assert (np.linalg.norm(far - corner, axis=1) > 6.5).all()
    sets["beyond max_ray_length"] = (far, corner)
    near_face = FO.PLACEMENTS["near_face"]
    out = np.c_[rng.uniform(-2.0, 2.0, 50), rng.uniform(3.3, 5.0, 50), rng.uniform(0.5, 2.8, 50)]       # beyond the +y face, within 6 m
    out[10:20] = out[0:10]                                                                               # repeated points: INVALID_IDX is not deduplicated
    assert (np.linalg.norm(out - near_face, axis=1) < 5.5).all()
    sets["ends outside the map"] = (out, near_face)
    # 24 points in the voxel [1.0, 1.1) x [0.5, 0.6) x [1.2, 1.3), the first near one corner and the last near the opposite one, among
    # points of two neighbouring voxels whose rays cross the first one's
    crowd = _in_voxel(rng, (1.0, 0.5, 1.2), 24)
    crowd[0] = (1.004, 0.504, 1.204); crowd[-1] = (1.096, 0.596, 1.296)
    others = np.r_[_in_voxel(rng, (1.4, 0.7, 1.1), 6), _in_voxel(rng, (1.7, 0.9, 1.4), 6)]
    sets["many points in one voxel"] = (np.r_[crowd, others], mid)
    sets["many points in one voxel, reversed"] = (np.r_[crowd[::-1], others[::-1]], mid)
    same = np.array([[0.09, 0.09, 1.69], [0.01, 0.09, 1.69], [0.09, 0.01, 1.69]])                       # 0.1 m and more from the sensor, in its voxel
    sets["sensor and point in one voxel"] = (same, (0.01, 0.01, 1.605))
    outside = (-4.0, 0.3, 1.5)                                                                           # 0.8 m beyond the -x face
    inside = np.c_[rng.uniform(-3.1, 1.0, 60), rng.uniform(-2.0, 2.5, 60), rng.uniform(0.1, 3.1, 60)]
    sets["sensor outside the map"] = (inside, outside)
    faces = np.array([[0.5, 0.3, 1.0], [-3.2, -3.2, 0.0], [3.2, 0.0, 1.0], [1.0, -3.2, 3.2], [-0.7, 0.0, 1.6], [0.0, 0.0, 3.1], [2.0, 1.0, 0.0],
                      [-3.2 + 17 * 0.1, -3.2 + 40 * 0.1, 9 * 0.1]])                                      # on voxel faces, the map's own among them
    sets["points on voxel faces"] = (faces, mid)
    holes = real.copy()
    for k, row in enumerate(range(3, len(holes), 37)):
        holes[row, k % 3] = (NAN, INF, -INF)[k % 3]
    holes[0] = (NAN, NAN, NAN); holes[-1] = (INF, 1.0, -INF)
    sets["NaN and inf rows"] = (holes, mid)
    sets["count below P"] = (real[:401].copy(), mid)
    for p, _ in sets.values():
        p.setflags(write=False)
    return sets


EDGE_NAMES = ("count 0", "all closer than min_ray_length", "beyond max_ray_length", "ends outside the map", "many points in one voxel",
              "many points in one voxel, reversed", "sensor and point in one voxel", "sensor outside the map", "points on voxel faces",
              "NaN and inf rows", "count below P")
# what the storage beyond a scan's count is filled with: NaN bit patterns (quiet, signalling, negative), huge and infinite values
POISON = np.array([0x7FF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, 0x7FF0000000000000],
                  dtype=np.uint64).view(np.float64)


def poison(pts, count):
    """pts [S, P, 3] with everything beyond count[s] overwritten by POISON, cycling."""
    out = np.array(pts, copy=True)
    for s in range(out.shape[0]):
        tail = out[s, int(count[s]):].reshape(-1)
        tail[...] = np.resize(POISON, tail.shape).astype(out.dtype)
    return out


@functools.lru_cache(maxsize=None)
def edge_chain(name):
    return chain([edge_sets()[name]])


@functools.lru_cache(maxsize=None)
def edge_batch_chain():
    return chain([edge_sets()[n] for n in EDGE_NAMES])


# ---- 4. order across scans: a wall 1.2 m in front of the sensor, then rays that pass through it (hits, then misses) ----
ORDER = (("wall", "middle"), ("steps", "middle"))


def order_scans():
    return [realistic(*k) for k in ORDER]


@functools.lru_cache(maxsize=None)
def order_chain(reverse):
    s = order_scans()
    return chain(s[::-1] if reverse else s)


# ---- 5. status and containment ----
def single_ray(k):
    """A scan of one point: one ray, final after the first round."""
    return np.array([[1.0 + 0.13 * k, -0.8 + 0.21 * k, 0.9 + 0.05 * k]]), (0.2 - 0.1 * k, 0.1 * k, 1.5)


def cap_scans():
    """Around a scan that needs several rounds: scans that are final after one (single rays, and no ray at all)."""
    return [single_ray(0), realistic("random", "middle"), single_ray(1), edge_sets()["all closer than min_ray_length"]]


@functools.lru_cache(maxsize=None)
def cap_chain():
    return chain(cap_scans(), cap=1)


@functools.lru_cache(maxsize=None)
def many_scans(S):
    """S scans of one to four points each, at sensor positions on a circle."""
    rng = np.random.default_rng(77)
    out = []
    for k in range(S):
        a = 2 * np.pi * k / 64
        o = (1.5 * np.cos(a), 1.5 * np.sin(a), 1.0 + 0.01 * k)
        n = 1 + k % 4
        out.append((np.c_[rng.uniform(-2.5, 2.5, n), rng.uniform(-2.5, 2.5, n), rng.uniform(0.3, 2.9, n)], o))
    return out


@functools.lru_cache(maxsize=None)
def many_chain(S):
    return chain(many_scans(S))
