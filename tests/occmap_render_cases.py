"""The maps, cameras and expected images that tests/test_occmap_render_cpu.py and tests/test_gpu_occmap_render.py share: worlds of
workloads.astar_world cropped to a 4 m x 4 m test map, the poses of tests/occmap_fusion_oracle.py, and the renderer's
specification (tests/occmap_render_oracle.py) applied to them.  Every image is computed once per process.

The test map is 40 x 40 voxels of 0.1 m in x and y, placed so that its +y face is at 3.2 m like that of occmap_fusion_oracle.TEST_GEO:
the placement "near_face" is then 0.3 m from that face and half of its rays leave the map.  Two heights: 20 voxels (one word of the
bit plane per column) and 33 (a second word: rays cross the word boundary)."""
import functools

import numpy as np

from forces_resilient_planner_amd import workloads
from tests import occmap_fusion_oracle as FO
from tests import occmap_render_oracle as RO

GEO = {"low": dict(origin=(-2.0, -0.8, 0.0), map_size=(4.0, 4.0, 2.0), resolution=0.1),
       "tall": dict(origin=(-2.0, -0.8, 0.0), map_size=(4.0, 4.0, 3.3), resolution=0.1)}
GRID = {"low": (40, 40, 20), "tall": (40, 40, 33)}
MAX_RANGE = 6.0
IMAGES = {"small": (24, 32), "large": (48, 64)}
K = {"small": np.array([[20.0, 0.0, 15.5], [0.0, 20.0, 11.5], [0.0, 0.0, 1.0]]), "large": FO.TEST_K}
K_INT = {"small": np.array([[20.0, 0.0, 16.0], [0.0, 20.0, 12.0], [0.0, 0.0, 1.0]]),                 # an integer principal point
         "large": np.array([[40.0, 0.0, 32.0], [0.0, 40.0, 24.0], [0.0, 0.0, 1.0]])}

# Where the test map's voxel (0, 0, 0) lies in the 200 x 200 x 40 grid of workloads.astar_world (origin (-10, -10, -1)).  "pillars": the
# window at the test map's own place.  "wall": workloads' wall_gap world has its wall across x = -0.2 ... 0.2, which is where the cameras
# stand; the window is shifted by 3.2 m so that the wall crosses the test map 1.2 m in front of them (a camera inside the wall sees nothing).
WINDOW = {"pillars": (80, 92, 10), "wall": (66, 92, 10)}
KIND = {"pillars": "pillars", "wall": "wall_gap", "ceiling": "wall_gap"}   # "ceiling": the wall under a slab at z index 32 (tall map only):
WINDOW["ceiling"] = WINDOW["wall"]                                          # returns from the second word of the bit plane's columns
SEED = {"pillars": 3, "wall": 0, "ceiling": 0}       # (seed 0 of the pillars has one standing on the placement "middle")


@functools.lru_cache(maxsize=None)
def world_occ(scene, height):
    """occ [40, 40, gz] uint8 of the test map: the window of the astar_world; above the world's top the map is free."""
    w = workloads.astar_world(seed=SEED[scene], kind=KIND[scene])
    lo, g = WINDOW[scene], GRID[height]
    occ = np.zeros(g, dtype=np.uint8)
    src = w["occ"][lo[0]:lo[0] + g[0], lo[1]:lo[1] + g[1], lo[2]:lo[2] + g[2]]
    occ[:src.shape[0], :src.shape[1], :src.shape[2]] = src
    if scene == "ceiling":
        occ[:, :, 32] = 1
    occ.setflags(write=False)
    return occ


def world(scene, height):
    """The dict solver.OccupancyMap(world=...) takes."""
    return dict(GEO[height], occ=world_occ(scene, height).copy())


def oracle(scene, height):
    g = GEO[height]
    return RO.RenderOracle(world_occ(scene, height), g["origin"], g["resolution"])


def axis_pose(t):
    """An axis-aligned camera: the optical axis along world x, camera x = -world y, camera y = -world z (FO.pose at yaw = pitch = 0
    holds cos and sin of 0, i.e. exact zeros and ones)."""
    return FO.pose(t, yaw=0.0, pitch=0.0)


@functools.lru_cache(maxsize=None)
def rendered(scene, height, image, pose_key, int_k=False):
    """(depth, voxel, segment, status, steps) of one frame.  pose_key: a name of FO.PLACEMENTS, or ("axis" | "pose", x, y, z)."""
    rows, cols = IMAGES[image]
    Km = (K_INT if int_k else K)[image]
    return oracle(scene, height).render(pose_of(pose_key), Km, rows, cols, MAX_RANGE)


def pose_of(pose_key):
    if isinstance(pose_key, str):
        return FO.pose(FO.PLACEMENTS[pose_key])
    kind, x, y, z = pose_key
    return axis_pose((x, y, z)) if kind == "axis" else FO.pose((x, y, z))


def excluded(depth, seg):
    """The pixels the 2 mm rule leaves out of a round trip: a return whose segment inside its voxel spans less than 2 mm of depth."""
    return (depth != 0) & (seg < RO.MIN_SEGMENT)


def projected_voxels(depth, Km, T, height):
    """[rows, cols] int32: the linear index of the voxel that FusionOracle.project puts each returning pixel's point into (-1: no
    return, -2: a point outside the map)."""
    g = GEO[height]
    fo = FO.FusionOracle(g["origin"], g["map_size"], g["resolution"], depth_filter_margin=0, skip_pixel=1, depth_filter_mindist=0.0005)
    pts = fo.project(depth, Km, T)                               # scan order, the zero pixels left out by mindist
    out = np.full(depth.shape, -1, dtype=np.int32)
    where = np.argwhere(depth != 0)
    assert len(where) == len(pts)
    gy, gz = GRID[height][1], GRID[height][2]
    for (v, u), p in zip(where, pts):
        id_ = fo._index(p)
        out[v, u] = -2 if id_ is None else (id_[0] * gy + id_[1]) * gz + id_[2]
    return out


# ---- the six frames of the bit-identity test ----
OUTSIDE = ("pose", -2.6, 1.0, 1.2)      # 0.6 m outside the -x face, looking in


@functools.lru_cache(maxsize=None)
def occupied_cell_centre(scene, height):
    """The centre of an occupied voxel at camera height (the one nearest the map's middle): a camera there sees nothing."""
    occ = world_occ(scene, height)
    idx = np.argwhere(occ[:, :, 12] != 0)
    assert len(idx) > 0
    i = idx[np.argmin(((idx - np.array([20, 20])) ** 2).sum(1))]
    o = GEO[height]["origin"]
    return (o[0] + (i[0] + 0.5) * 0.1, o[1] + (i[1] + 0.5) * 0.1, o[2] + 12.5 * 0.1)


def six_poses(scene, height):
    """[6, 4, 4]: middle, near_face, outside looking in, inside an occupied voxel, (inactive: any pose), a NaN pose."""
    inside = ("pose",) + occupied_cell_centre(scene, height)
    T = np.stack([pose_of(k) for k in ("middle", "near_face", OUTSIDE, inside, "middle", "middle")])
    T[5, 1, 2] = float("nan")
    return T, ["middle", "near_face", OUTSIDE, inside]
