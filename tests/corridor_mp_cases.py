"""The cases of tests/golden/corridor_mp.npz (tests/tools/gen_corridor_mp.py writes it; tests/test_corridor_mp_cpu.py and
tests/test_gpu_corridor_offset.py read it): worlds built like tests/test_gpu_parity.py::_corridor_world, plus a rotation of the whole
world about z, for seed ellipsoids that are spheres (offset_x = 0), prolate (offset_x > 0) and oblate discs (offset_x < 0).

With f = seed_len / 2 and r = f / (f + offset_x) the seed ellipsoid has semi-axes (f, f r, f r) along the heading.  numpy only: the
fixture's reader needs neither mpmath nor a GPU."""
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "corridor_mp.npz")
N, B = 20, 3
MARGIN = 1e-7          # a planner is decisive when every discrete decision of its reference run had more than this to spare
ROW_TOL = 1e-9         # the project's row tolerance (tests/test_gpu_parity.py::_check_corridor)
CONST_KEYS = ("bbox0", "bbox1", "bbox2", "seed_len", "inflation", "offset_x")
MARGIN_KINDS = ("pick", "keep_drop", "box", "in_seed", "reuse")

# name: (offset_x, seed_len, z rotation in degrees, tunnel, world seed, points drawn)
CASES = {
    "a_sphere": (0.0, 0.1, 0, 0.6, 101, 6000),
    "b_prolate": (0.15, 0.1, 0, 0.6, 102, 6000),
    "c_oblate": (-0.03, 0.1, 0, 0.6, 103, 6000),
    "d_oblate_45": (-0.03, 0.1, 45, 0.6, 104, 6000),
    "e_oblate_100": (-0.03, 0.1, 100, 0.6, 105, 6000),
    "f_prolate_45": (0.3, 0.4, 45, 0.6, 106, 6000),
    "d_oblate_45_shells": (-0.03, 0.1, 45, 0.6, 107, 20000),
    "f_prolate_45_shells": (0.3, 0.4, 45, 0.6, 108, 20000),
}


def consts_of(name):
    off, sl = CASES[name][:2]
    return dict(bbox=(2.0, 2.0, 1.0), seed_len=sl, inflation=1.1, offset_x=off)


def consts_row(c):
    return np.array([*c["bbox"], c["seed_len"], c["inflation"], c["offset_x"]], dtype=np.float64)


def consts_dict(row):
    return dict(bbox=tuple(float(x) for x in row[:3]), seed_len=float(row[3]), inflation=float(row[4]), offset_x=float(row[5]))


def _centre():
    s = np.linspace(0, 5, N)
    return np.c_[s, 0.4 * np.sin(0.8 * s), 1.0 + 0.1 * np.cos(s)]


def _rotate(xyz, cs):
    """About z by the angle whose (cos, sin) is cs -- elementwise products and sums only, so the bits depend on cs alone."""
    c, s = float(cs[0]), float(cs[1])
    out = np.array(xyz, dtype=np.float64)
    x, y = out[..., 0].copy(), out[..., 1].copy()
    out[..., 0] = c * x - s * y
    out[..., 1] = s * x + c * y
    return out


def cloud_of(seed, P, tunnel, cs=None):
    """_corridor_world's cloud (the first three draws of its generator), rotated about z when cs = (cos, sin) is given."""
    rng = np.random.default_rng(seed)
    cloud = np.c_[rng.uniform(-3, 9, P), rng.uniform(-4, 4, P), rng.uniform(-0.5, 3, P)]
    centre = _centre()
    cx = np.interp(cloud[:, 0], centre[:, 0], centre[:, 1]); cz = np.interp(cloud[:, 0], centre[:, 0], centre[:, 2])
    cloud = cloud[np.hypot(cloud[:, 1] - cx, cloud[:, 2] - cz) > tunnel]
    return cloud if cs is None else _rotate(cloud, cs)


def cloud_sha256(cloud):
    return hashlib.sha256(np.ascontiguousarray(cloud, dtype=np.float64).tobytes()).hexdigest()


def world(seed, P=6000, B=B, tunnel=0.6, rot_deg=0):
    """(cloud, ref [B,N,3], yaw [B,N], E [B,N,3,3], (cos, sin) of the rotation).  rot_deg = 0 is _corridor_world(seed, P, B, N, tunnel)
    to the bit; otherwise cloud and references are turned about z, the yaws advanced, and the tube taken of the turned plan."""
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import tube_oracle as T
    rng = np.random.default_rng(seed)
    for lo, hi in ((-3, 9), (-4, 4), (-0.5, 3)):
        rng.uniform(lo, hi, P)                                      # the cloud's draws (cloud_of repeats them)
    centre = _centre()
    ref = centre[None] + rng.normal(0, 0.03, (B, N, 3))
    yaw = np.arctan2(np.gradient(centre[:, 1]), np.gradient(centre[:, 0]))[None] + rng.normal(0, 0.05, (B, N))
    a = np.deg2rad(float(rot_deg))
    cs = np.array([np.cos(a), np.sin(a)]) if rot_deg else np.array([1.0, 0.0])
    if rot_deg:
        ref = _rotate(ref, cs); yaw = yaw + a
    z = np.zeros((B, N, 17)); z[..., 3] = 7.3; z[..., 8:11] = ref; z[..., 16] = yaw
    z[..., 11:14] = rng.normal(0, 0.5, (B, N, 3)); z[..., 14:16] = rng.normal(0, 0.1, (B, N, 2))
    return cloud_of(seed, P, tunnel, cs if rot_deg else None), ref, yaw, T.tube_batch(z), cs


class Case:
    """One case of the fixture: inputs, the regenerated cloud (its digest checked), and the expected polytopes."""

    def __init__(self, fx, k):
        self.name = str(fx["case_name"][k])
        self.consts = consts_dict(fx["consts"][k])
        self.seed, self.P, self.tunnel = int(fx["seed"][k]), int(fx["P"][k]), float(fx["tunnel"][k])
        self.rot_deg, self.cs = float(fx["rot_deg"][k]), fx["rot_cs"][k]
        self.ref, self.yaw, self.E = fx["ref"][k], fx["yaw"][k], fx["E"][k]
        self.sha = str(fx["cloud_sha256"][k])
        self.poly_index, self.poly_count, self.nfaces = fx["poly_index"][k], fx["poly_count"][k], fx["nfaces"][k]
        self.decisive, self.undecided = fx["decisive"][k], fx["undecided"][k]
        self.margins, self.min_margin = fx["margins"][k], float(fx["min_margin"][k])
        self._rows, self._start = fx["rows"], fx["row_start"][k]

    def cloud(self):
        cloud = cloud_of(self.seed, self.P, self.tunnel, self.cs if self.rot_deg else None)
        assert cloud_sha256(cloud) == self.sha, f"{self.name}: the regenerated cloud is not the one the fixture was made from"
        return cloud

    def rows(self, p, k):
        """[nfaces, 4] = (a, b) rows of planner p's polytope k, in order."""
        s = int(self._start[p, k])
        return self._rows[s:s + int(self.nfaces[p, k])]


def load():
    with np.load(FIXTURE) as f:
        fx = {k: f[k] for k in f.files}
    assert tuple(fx["const_keys"]) == CONST_KEYS and tuple(fx["margin_kinds"]) == MARGIN_KINDS
    return [Case(fx, k) for k in range(len(fx["case_name"]))]


def compare_with_fixture(case, p, index, count, nfaces, rows_of):
    """Planner p of `case` against the fixture: indices, counts and row order identical, rows within ROW_TOL.  rows_of(k) -> [m,4].
    Returns the largest row deviation."""
    assert np.array_equal(index, case.poly_index[p]), (case.name, p, index, case.poly_index[p])
    assert int(count) == int(case.poly_count[p]), (case.name, p)
    worst = 0.0
    for k in range(int(case.poly_count[p])):
        assert int(nfaces[k]) == int(case.nfaces[p, k]), (case.name, p, k, int(nfaces[k]), int(case.nfaces[p, k]))
        dev = float(np.max(np.abs(np.asarray(rows_of(k)) - case.rows(p, k))))
        assert dev < ROW_TOL, (case.name, p, k, dev)
        worst = max(worst, dev)
    return worst


def check_properties(case_name, consts, cloud, ref, yaw, index, polys):
    """float64 properties of one planner's polytopes (list of (A [m,3], b [m])): unit normals, no in-box cloud point strictly inside,
    and p1, p2 and their midpoint of every decomposition's seed segment inside its polytope."""
    bb, sl = consts["bbox"], consts["seed_len"]
    first = {}
    for i, k in enumerate(index):
        first.setdefault(int(k), i)                                 # polytope k was decomposed at the first stage that uses it
    assert sorted(first) == list(range(len(polys))), (case_name, index)
    for k, (A, b) in enumerate(polys):
        assert np.max(np.abs(np.linalg.norm(A, axis=1) - 1.0)) < 1e-12, (case_name, k)
        i = first[k]
        h = np.array([np.cos(yaw[i]), np.sin(yaw[i]), 0.0]); dh = np.array([h[1], -h[0], 0.0])
        p1 = ref[i]; p2 = p1 + sl * h
        e = cloud - p1
        t, s, v = e @ h, e @ dh, e[:, 2]
        inbox = (np.abs(s) <= bb[1] + 1e-10) & (t >= -bb[0] - 1e-10) & (t <= sl + bb[0] + 1e-10) & (np.abs(v) <= bb[2] + 1e-10)
        assert inbox.any(), (case_name, k)
        inside = np.all(cloud[inbox] @ A.T - b < -1e-9, axis=1)
        assert not inside.any(), (case_name, k, int(inside.sum()))
        for q in (p1, p2, (p1 + p2) / 2):
            assert np.all(A @ q - b <= 0), (case_name, k, float(np.max(A @ q - b)))
