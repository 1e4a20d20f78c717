"""GPU tests of the occupancy map's distance field and clearance queries (include/frp_nmpc_occmap_distance.h,
csrc/frp_occmap_distance.hip, solver.DistanceField / FlightClearance) against the brute-force statement
tests/occmap_distance_oracle.py.  The field and d2 are integers: every comparison of them is np.array_equal.  clear is
resolution * sqrt(d2) with a correctly rounded square root and one product, as NumPy computes it: compared to the bit as well
(measured on an MI355X over every d2 that occurs for R = 64: the device's FP64 square root agrees with NumPy's in every bit)."""
import functools
import types

import numpy as np
import pytest

from forces_resilient_planner_amd import solver
from tests import occmap_distance_oracle as DO
from tests import occmap_oracle as OO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RES = 0.1


def geo(grid, origin=(-1.25, -1.0, 0.0)):
    """A map of exactly `grid` voxels of 0.1 m: sizes half a voxel short of a multiple, so that the ceil() of the grid size is safe.  The
    origin is no multiple of the resolution."""
    return dict(origin=origin, map_size=tuple((g - 0.5) * RES for g in grid), resolution=RES)


def device_map(occ, **g):
    import torch
    dm = solver.OccupancyMap(**g)
    assert dm.grid == tuple(occ.shape), (dm.grid, occ.shape)
    dm.log_odds.fill_(dm.clamp_min_log)
    dm.log_odds.masked_fill_(torch.from_numpy(np.array(occ, dtype=bool)).to(dm.device), dm.clamp_max_log)   # (a copy: the shared references are read-only)
    dm.refresh()
    return dm


def landmarks(grid, occ):
    """Occupied voxels at z = 0, 31, 32, 63, 64 and gz - 1 (those the grid has) of separate columns, and the eight corners."""
    gx, gy, gz = grid
    for i, z in enumerate(sorted({z for z in (0, 31, 32, 63, 64, gz - 1) if z < gz})):
        occ[(1 + 2 * i) % gx, (1 + i) % gy, z] = True
    for x in (0, gx - 1):
        for y in (0, gy - 1):
            for z in (0, gz - 1):
                occ[x, y, z] = True
    return occ


def sparse(grid, p, seed):
    return landmarks(grid, np.random.default_rng(seed).random(grid) < p)


# (name, grid, R, occupancy, FAR expected without / with the border); True: both FAR and values must occur, False: values alone, None: FAR alone
CASES = [("7x5x33-second-word-has-one-bit", (7, 5, 33), 2, lambda g: landmarks(g, np.zeros(g, dtype=bool)), (True, True)),
         ("13x9x70-three-words", (13, 9, 70), 4, lambda g: landmarks(g, np.zeros(g, dtype=bool)), (True, True)),
         ("6x6x40-R1", (6, 6, 40), 1, lambda g: sparse(g, 0.02, 21), (True, True)),
         ("4x3x2-R9-window-beyond-every-axis", (4, 3, 2), 9, lambda g: sparse(g, 0.0, 22), (False, False)),
         ("40x24x70-R6-sparse", (40, 24, 70), 6, lambda g: sparse(g, 0.005, 23), (True, True)),
         ("empty-7x5x33", (7, 5, 33), 2, lambda g: np.zeros(g, dtype=bool), (None, True)),
         ("empty-13x9x70-R64", (13, 9, 70), 64, lambda g: np.zeros(g, dtype=bool), (None, False)),
         ("full-13x9x70", (13, 9, 70), 4, lambda g: np.ones(g, dtype=bool), (False, False))]


@functools.lru_cache(maxsize=None)
def reference(i):
    """(occ, field without the border, field with it) of case i: computed once, shared, read-only."""
    name, grid, R, make, census = CASES[i]
    occ = make(grid)
    out = (occ, DO.field(occ, R, False), DO.field(occ, R, True))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_field_equals_the_statement_to_the_bit(i):
    import torch
    name, grid, R, make, census = CASES[i]
    occ, plain, bordered = reference(i)
    for want, expect in zip((plain, bordered), census):       # the census, on the CPU: no case passes on a degenerate field
        far, val = bool((want == DO.FAR).any()), bool((want != DO.FAR).any())
        print(f"{name}: FAR {int((want == DO.FAR).sum())}, values {int((want != DO.FAR).sum())}, distinct {len(np.unique(want))}, occupied {int(occ.sum())}")
        assert (far, val) == {True: (True, True), False: (False, True), None: (True, False)}[expect]
        assert (want[occ] == 0).all()
    assert (bordered <= plain).all()
    dm = device_map(occ, **geo(grid))
    for border, want in ((False, plain), (True, bordered)):
        df = dm.distance_field(R=R, border=border)
        torch.cuda.synchronize()
        got = df.field.cpu().numpy()
        assert got.dtype == np.uint16 and got.shape == grid
        assert np.array_equal(got, want), (name, border, int((got != want).sum()), np.argwhere(got != want)[:5])
        df.field.view(torch.int16).zero_()
        df.update()                                              # ... and again, into a field that held something else
        torch.cuda.synchronize()
        assert np.array_equal(df.field.cpu().numpy(), want)


def test_padding_bits_of_the_last_z_word_are_not_voxels():
    """No public call sets a bit at z >= gz (insert and refresh write voxels of the map only), so they are set in a copy of the
    workspace: every padding bit of every column.  Without the border they must not count; with it they are outside voxels, which count
    anyway."""
    import torch
    for i in (0, 1):                                            # gz = 33: 31 padding bits; gz = 70: 26
        name, grid, R, make, census = CASES[i]
        occ, plain, bordered = reference(i)
        gx, gy, gz = grid
        wz = (gz + 31) // 32
        dm = device_map(occ, **geo(grid))
        clean = dm.ws
        words = clean[:gx * gy * wz].cpu().numpy().view(np.uint32).reshape(gx, gy, wz)
        assert np.array_equal(words, DO.pack_plane(occ))          # the layout the statement reads is the device's
        pad = np.uint32((0xffffffff << (gz % 32)) & 0xffffffff)
        stale = words.copy()
        stale[:, :, wz - 1] |= pad
        assert (stale != words).any() and np.array_equal(DO.unpack_plane(stale, gz), occ)
        dirty = clean.clone()
        dirty[:gx * gy * wz] = torch.from_numpy(stale.reshape(-1).view(np.int32)).to(dm.device)
        for border, want in ((False, plain), (True, bordered)):
            df = dm.distance_field(R=R, border=border)
            dm.ws = dirty
            try:
                df.update()
                torch.cuda.synchronize()
            finally:
                dm.ws = clean
            assert np.array_equal(df.field.cpu().numpy(), want), (name, border)


def test_rebuild_after_the_map_changes_eager_and_replayed():
    import torch
    grid, R = (13, 9, 70), 3
    g = geo(grid)
    om = OO.OccMapOracle(**g)
    dm = solver.OccupancyMap(**g)
    assert tuple(om.grid_size) == grid == dm.grid
    rng = np.random.default_rng(31)
    lo, size = np.array(g["origin"]), np.array(g["map_size"])
    cloud = lambda n: (lo + rng.random((n, 3)) * size).astype(np.float32)
    fields = []
    df = {b: dm.distance_field(R=R, border=b) for b in (False, True)}

    def check(what):
        occ = om.occ().astype(bool)
        for b in (False, True):
            df[b].update()
        torch.cuda.synchronize()
        assert np.array_equal(dm.occ.cpu().numpy() != 0, occ), what
        for b in (False, True):
            want = DO.field(occ, R, b)
            assert (want == DO.FAR).any() and (want != DO.FAR).any()
            assert np.array_equal(df[b].field.cpu().numpy(), want), (what, b)
        fields.append(df[False].field.cpu().numpy().copy())

    pts = cloud(40)
    om.insert_cloud(pts); dm.insert_cloud(pts)
    check("after insert_cloud")
    box = (lo + np.array([0.2, 0.1, 1.0]), lo + np.array([0.9, 0.7, 5.0]))
    om.reset_buffer(*box); dm.clear_box(*box)
    check("after clear_box")
    assert not np.array_equal(fields[0], fields[1])
    # a captured update() replayed after the map changed equals an eager one
    captured = dm.distance_field(R=R, border=True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        captured.update(side)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured.update(torch.cuda.current_stream())
    torch.cuda.synchronize()
    for n in (25, 10):
        pts = cloud(n)
        om.insert_cloud(pts); dm.insert_cloud(pts)
        captured.field.view(torch.int16).fill_(7)
        graph.replay()
        df[True].update()
        torch.cuda.synchronize()
        want = DO.field(om.occ().astype(bool), R, True)
        assert torch.equal(captured.field.view(torch.int16), df[True].field.view(torch.int16))
        assert np.array_equal(captured.field.cpu().numpy(), want)
        fields.append(want)
    assert not np.array_equal(fields[-1], fields[-2])


# ---- clearance ----
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _expected_clear(d2):
    """resolution * sqrt(d2) as NumPy rounds it (a correctly rounded square root, one product); +inf for FAR, 0.0 for -1."""
    d2 = np.asarray(d2)
    c = np.float64(RES) * np.sqrt(np.where(d2 > 0, d2, 0).astype(np.float64))
    return np.where(d2 == DO.FAR, np.inf, np.where(d2 < 0, 0.0, c))


def test_clearance_of_points_on_faces_outside_and_not_finite():
    import torch
    i = 4                                                        # the sparse 40 x 24 x 70 map: zeros, values up to 36 and FAR all occur
    name, grid, R, make, census = CASES[i]
    occ, plain, bordered = reference(i)
    g = geo(grid)
    om = OO.OccMapOracle(**g)
    lo = np.array(g["origin"])
    hi_face = lo + np.array(grid) * RES
    rng = np.random.default_rng(41)
    inner = lambda n: lo + rng.random((n, 3)) * (np.array(grid) * RES)
    pts = [inner(150)]
    faces = inner(120)                                           # on voxel faces, origin + k * res as doubles, and one ulp to either side
    k = np.floor((faces - lo) / RES)
    on = lo + k * RES
    which = rng.random(faces.shape) < 0.6
    faces[which] = on[which]
    pts += [faces, np.nextafter(faces, -np.inf), np.nextafter(faces, np.inf)]
    centre = lo + (np.array(grid) / 2.0) * RES
    for a in range(3):                                           # outside on each of the six sides: just beyond, one ulp beyond, far beyond
        for face, s in ((lo[a], -1.0), (hi_face[a], 1.0)):
            for d in (0.03, 0.0, 1.0e6):
                p = centre.copy()
                p[a] = face + s * d if d else np.nextafter(face, s * np.inf) if s < 0 else face
                pts.append(p[None, :])
    pts.append(np.array([om.index_to_pos(v) for v in np.argwhere(occ)[::30]]))    # inside occupied voxels
    bad = np.tile(centre, (7, 1))
    bad[0, 0] = np.nan; bad[1, 1] = np.inf; bad[2, 2] = -np.inf; bad[3] = np.nan; bad[4, 0] = np.inf; bad[4, 1] = np.nan; bad[5, 2] = 1.0e300; bad[6, 0] = -1.0e300
    pts.append(bad)
    far_voxel = tuple(np.argwhere(plain == DO.FAR)[0])
    pts.append(om.index_to_pos(far_voxel)[None, :])
    pts = np.concatenate(pts)
    wants = {}
    for border, fld in ((False, plain), (True, bordered)):       # the statement's answers and their census first, on the CPU
        want_c, want_d = wants[border] = DO.clearances(om, fld, pts)
        print(f"border {border}: outside {int((want_d < 0).sum())}, FAR {int((want_d == DO.FAR).sum())}, zero {int((want_d == 0).sum())}, values {int(((want_d > 0) & (want_d != DO.FAR)).sum())} of {len(pts)}")
        assert (want_d < 0).sum() >= 20 and (want_d == 0).any() and ((want_d > 0) & (want_d != DO.FAR)).sum() >= 50
        assert want_d[-1] == fld[far_voxel] and (border or want_d[-1] == DO.FAR)   # a point whose voxel is FAR
        assert np.array_equal(_bits(want_c), _bits(_expected_clear(want_d)))
        assert (want_d[-8:-1] == -1).all() and (want_c[-8:-1] == 0.0).all()         # the seven positions that are not finite, or absurd
    dm = device_map(occ, **g)
    for border in (False, True):
        want_c, want_d = wants[border]
        df = dm.distance_field(R=R, border=border)
        clear, d2 = df.clearance(pts.copy(), d2=True)
        alone = df.clearance(torch.from_numpy(pts.copy()).to(DEV))
        torch.cuda.synchronize()
        assert np.array_equal(d2.cpu().numpy(), want_d)
        assert np.array_equal(_bits(clear.cpu().numpy()), _bits(want_c)) and np.array_equal(_bits(alone.cpu().numpy()), _bits(want_c))
    assert df.clearance(np.zeros((0, 3))).shape == (0,)


def test_clearance_over_every_squared_distance_up_to_r64():
    """One occupied corner voxel and R = 64: d2 = x^2 + y^2 + z^2 takes about 1800 distinct values up to 4096, and the square root
    of each is compared to the bit -- and, printed before the assertion, against 50 digits next to NumPy's own error."""
    import mpmath
    import torch
    grid, R = (66, 8, 8), 64
    occ = np.zeros(grid, dtype=bool)
    occ[0, 0, 0] = True
    fld = DO.field(occ, R, False)
    g = geo(grid)
    om = OO.OccMapOracle(**g)
    vox = np.argwhere(np.ones(grid, dtype=bool))
    pts = np.array([om.index_to_pos(v) for v in vox])
    want_c, want_d = DO.clearances(om, fld, pts)
    assert np.array_equal(want_d, fld.reshape(-1).astype(np.int32)) and (want_d == DO.FAR).any() and len(np.unique(want_d)) > 1500 and 4096 in want_d
    dm = device_map(occ, **g)
    df = dm.distance_field(R=R, border=False)
    clear, d2 = df.clearance(pts, d2=True)
    torch.cuda.synchronize()
    clear, d2 = clear.cpu().numpy(), d2.cpu().numpy()
    assert np.array_equal(df.field.cpu().numpy(), fld) and np.array_equal(d2, want_d)
    mpmath.mp.dps = 50
    fin = want_d != DO.FAR
    exact = [mpmath.mpf(RES) * mpmath.sqrt(int(v)) for v in want_d[fin]]
    e_dev = max(abs(mpmath.mpf(float(c)) - e) for c, e in zip(clear[fin], exact))
    e_np = max(abs(mpmath.mpf(float(c)) - e) for c, e in zip(want_c[fin], exact))
    print(f"clear over {int(fin.sum())} voxels, {len(np.unique(want_d))} distinct d2: worst error against 50 digits: device {float(e_dev):.3e}, NumPy {float(e_np):.3e}; "
          f"bits that differ from NumPy's: {int((_bits(clear) != _bits(want_c)).sum())}")
    assert np.array_equal(_bits(clear), _bits(want_c))


# ---- traces ----
def _vehicle(n, S, trace=True):
    """A solver.Vehicle for n vehicles without a fleet behind it (the class reads the fleet's size and device alone)."""
    import torch
    fleet = types.SimpleNamespace(torch=torch, B=n, solver=types.SimpleNamespace(device=torch.device(DEV)))
    return solver.Vehicle(fleet, trace=trace, S=S)


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


@pytest.mark.parametrize("stride", [9, 3])
def test_clearance_trace_accumulates_as_the_statement_does(stride):
    import torch
    B, S = 5, 5
    name, grid, R, make, census = CASES[0]
    occ, plain, bordered = reference(0)
    g = geo(grid)
    om = OO.OccMapOracle(**g)
    lo = np.array(g["origin"])
    rng = np.random.default_rng(51 + stride)
    trace = rng.normal(0.0, 50.0, (B, S, stride))                 # (what follows the position is never read: anything)
    trace[:, :, 0:3] = lo + rng.random((B, S, 3)) * (np.array(grid) * RES)
    trace[0, :, 0:3] = om.index_to_pos((3, 2, 16))                 # FAR throughout: min_clear stays +inf
    trace[1, 2, 0:3] = om.index_to_pos((0, 0, 0))                  # inside an occupied voxel
    trace[3, 1, 1] = np.nan                                        # a NaN sample: a hit, min_clear = 0
    trace[4, 4, 0] = lo[0] - 0.01                                  # outside
    active = np.array([1, 1, 0, 1, 1], dtype=np.int32)
    start = [np.array([np.inf, np.inf, 7.5, np.inf, np.inf]), np.array([0, 0, 3, 0, 0], dtype=np.int32), np.array([0, 0, 11, 0, 0], dtype=np.int32)]
    want = DO.trace_accumulate(om, plain, trace, *start, active=active)
    assert np.isposinf(want[0][0]) and want[0][1] == 0.0 and want[1][1] >= 1 and want[0][3] == 0.0 and want[1][3] >= 1 and want[1][4] >= 1
    assert (want[0][2], want[1][2], want[2][2]) == (7.5, 3, 11) and list(want[2]) == [5, 5, 11, 5, 5]
    dm = device_map(occ, **g)
    df = dm.distance_field(R=R, border=False)
    veh = _vehicle(B, S)
    fc = solver.FlightClearance(veh, df)
    torch.cuda.synchronize()
    assert np.isposinf(fc.min_clear.cpu().numpy()).all() and not fc.hits.any() and not fc.samples.any()
    d_trace = _dev(trace, np.float64)
    fc.min_clear[2] = 7.5; fc.hits[2] = 3; fc.samples[2] = 11        # the inactive vehicle keeps whatever it holds
    fc.update(trace=d_trace, active=_dev(active, np.int32))
    torch.cuda.synchronize()
    got = [a.cpu().numpy() for a in (fc.min_clear, fc.hits, fc.samples)]
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    # a second call goes on from there (everybody active): the statement applied twice
    want2 = DO.trace_accumulate(om, plain, trace, *want)
    fc.update(trace=d_trace)
    torch.cuda.synchronize()
    got2 = [a.cpu().numpy() for a in (fc.min_clear, fc.hits, fc.samples)]
    assert np.array_equal(_bits(got2[0]), _bits(want2[0])) and np.array_equal(got2[1], want2[1]) and np.array_equal(got2[2], want2[2])
    # one S = 5 call equals five S = 1 calls
    one = solver.FlightClearance(veh, df)
    for s in range(S):
        one.update(trace=d_trace[:, s:s + 1].contiguous())
    whole = solver.FlightClearance(veh, df)
    whole.update(trace=d_trace)
    # a captured call replays to the bit
    cap = solver.FlightClearance(veh, df)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        cap.update(trace=d_trace, stream=side)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cap.update(trace=d_trace, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    cap.reset()
    graph.replay()
    torch.cuda.synchronize()
    for other in (one, cap):
        assert torch.equal(other.min_clear.view(torch.int64), whole.min_clear.view(torch.int64)) and torch.equal(other.hits, whole.hits) and torch.equal(other.samples, whole.samples)
    assert list(whole.samples.cpu().numpy()) == [S] * B
    # masked reset
    keep = [a.clone() for a in (whole.min_clear, whole.hits, whole.samples)]
    mask = np.array([0, 1, 0, 1, 0], dtype=np.int32)
    whole.reset(mask=_dev(mask, np.int32))
    torch.cuda.synchronize()
    mc, h, n = (a.cpu().numpy() for a in (whole.min_clear, whole.hits, whole.samples))
    for b in range(B):
        if mask[b]:
            assert np.isposinf(mc[b]) and h[b] == 0 and n[b] == 0
        else:
            assert _bits(mc[b]) == _bits(keep[0][b].item()) and h[b] == keep[1][b].item() and n[b] == keep[2][b].item() == S
    whole.reset()
    torch.cuda.synchronize()
    assert np.isposinf(whole.min_clear.cpu().numpy()).all() and not whole.hits.any() and not whole.samples.any()


def test_flight_clearance_reads_the_trace_the_vehicle_keeps_or_says_that_there_is_none():
    import torch
    occ, plain, bordered = reference(0)
    dm = device_map(occ, **geo(CASES[0][1]))
    df = dm.distance_field(R=CASES[0][2])
    bare = _vehicle(4, 5, trace=False)
    with pytest.raises(ValueError, match="keeps no trace"):
        solver.FlightClearance(bare, df).update()
    est = solver.ForceEstimator(bare)                              # attaches itself: its meas is where Vehicle.step writes the trace
    est.meas[:, :, 0:3] = _dev(OO.OccMapOracle(**geo(CASES[0][1])).index_to_pos((0, 0, 0)), np.float64)
    fc = solver.FlightClearance(bare, df)
    fc.update()
    torch.cuda.synchronize()
    assert list(fc.hits.cpu().numpy()) == [5] * 4 and (fc.min_clear == 0.0).all()
    with pytest.raises(ValueError):
        fc.update(trace=torch.zeros((4, 5, 2), dtype=torch.float64, device=DEV))
    with pytest.raises(AssertionError):
        fc.update(trace=torch.zeros((3, 5, 9), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        dm.distance_field(R=65)


# ---- one closed loop ----
WALL_GRID, WALL_Y, WALL_R = (40, 24, 20), 18, 8
LINES_Y = (10, 12, 14)                                           # the vehicles' voxel rows: 8, 6 and 4 voxels from the wall
STEPS, S_LOOP = 4, 5


def wall_commands(om):
    """(x0 [B, 9], commands [STEPS][B, S, 16], kind): vehicles that start at 1.5 m/s along x on the voxel-centre lines y = LINES_Y at z =
    voxel 10, x = voxel 10, and position setpoints (FRP_COMMAND_YAW: a position and a yaw) that move 1.5 cm per 10 ms sample along x.
    Fixed after flying them through tests/vehicle_oracle.py and the statement on the CPU: 0.27 m along x in the 20 samples, 2 cm of
    sag, nothing sideways -- no hit, and the clearance of each line is its distance to the wall."""
    B = len(LINES_Y)
    cmds = np.zeros((STEPS, B, S_LOOP, solver.COMMAND_STRIDE))
    x0 = np.zeros((B, solver.VEHICLE_STATE))
    for b, y in enumerate(LINES_Y):
        start = om.index_to_pos((10, y, 10))
        x0[b, 0:3] = start
        x0[b, 3] = 1.5
        for k in range(STEPS):
            for s in range(S_LOOP):
                cmds[k, b, s, 0:3] = start + np.array([0.015 * (k * S_LOOP + s + 1), 0.0, 0.0])
    kind = np.full((B, S_LOOP), solver.COMMAND_YAW, dtype=np.int32)
    return x0, cmds, kind


def test_closed_loop_a_vehicle_flies_along_a_wall():
    import torch
    occ = np.zeros(WALL_GRID, dtype=bool)
    occ[:, WALL_Y, :] = True
    g = geo(WALL_GRID, origin=(0.0, 0.0, 0.0))
    om = OO.OccMapOracle(**g)
    fld = DO.field(occ, WALL_R, True)
    x0, cmds, kind = wall_commands(om)
    B = len(LINES_Y)
    dm = device_map(occ, **g)
    df = dm.distance_field(R=WALL_R, border=True)
    veh = _vehicle(B, S_LOOP)
    veh.reset(_dev(x0, np.float64))
    fc = solver.FlightClearance(veh, df)
    d_kind = _dev(kind, np.int32)
    traces = []
    for k in range(STEPS):
        veh.step(solver.Commands(_dev(cmds[k], np.float64), d_kind, None, None, None))
        fc.update()
        traces.append(veh.trace.clone())                         # (a device copy: nothing is read back inside the loop)
    torch.cuda.synchronize()
    flown = np.concatenate([t.cpu().numpy() for t in traces], axis=1)
    assert flown.shape == (B, STEPS * S_LOOP, solver.VEHICLE_STATE)
    want = DO.trace_accumulate(om, fld, flown, np.full(B, np.inf), np.zeros(B), np.zeros(B))
    print("min_clear", want[0], "hits", want[1], "moved", flown[:, -1, 0] - x0[:, 0])
    assert (want[1] == 0).all() and np.isfinite(want[0]).all() and (want[0] > 0.0).all() and list(want[2]) == [STEPS * S_LOOP] * B
    assert np.array_equal(want[0], RES * np.sqrt(np.array([64.0, 36.0, 16.0])))    # the lines' distances to the wall, centre to centre
    assert (flown[:, -1, 0] - x0[:, 0] > 0.1).all()                # the vehicles moved through more than one voxel
    assert np.array_equal(_bits(fc.min_clear.cpu().numpy()), _bits(want[0]))
    assert np.array_equal(fc.hits.cpu().numpy(), want[1]) and np.array_equal(fc.samples.cpu().numpy(), want[2])
