"""CPU restatement of the safety timer's collision checks, one statement of the reference per statement here, over
tests/occmap_oracle.OccMapOracle.get_voxel_state:
  * OccMap::checkPosSurround (occ_grid/src/occ_map.cpp:625-643; ":NNN" below is that file),
  * the goal test / search and the path loop of NMPCManage::checkReplanCallback (plan_manage/src/nmpc_manage.cpp:285-341;
    "m:NNN" below is that file), without the FSM transitions between them.
It is what tests/test_gpu_occmap_check.py compares frp_nmpc_occmap_check_* against; every quantity is an integer or a double that
is copied or results from ONE addition, so the comparison is to the bit.

Like its siblings (occmap_oracle.py, occmap_fusion_oracle.py) it is a restatement: the reference's two classes need Eigen and ROS
and cannot be run here, so nothing pins this file to the reference but reading the two side by side.
"""
import math

import numpy as np

EGO_R, EGO_H = 0.27, 0.0425   # occ_map/ego_r, ego_h of the reference's launch file


def half_extents(m, inflate_ratio, body=(EGO_R, EGO_H)):
    ego_r, ego_h = float(body[0]), float(body[1])
    x_size = int(math.ceil(ego_r * inflate_ratio / float(m.resolution)))                 # :627
    y_size = int(math.ceil(ego_r * inflate_ratio / float(m.resolution)))                 # :628
    z_size = int(math.ceil(ego_h * inflate_ratio / float(m.resolution)))                 # :629
    return x_size, y_size, z_size


def check_pos_surround(m, pos, inflate_ratio, box=None, body=(EGO_R, EGO_H)):
    """checkPosSurround(pos, inflate_ratio) (:625-643): True = free.  box: the planner's local box (OccMapOracle.local_box) or None."""
    x_size, y_size, z_size = half_extents(m, inflate_ratio, body)
    pos = np.asarray(pos, dtype=np.float64)
    for i in range(-x_size, x_size + 1):                                                  # :631
        for j in range(-y_size, y_size + 1):                                              # :632
            for k in range(-z_size, z_size + 1):                                          # :633
                grid = pos + np.array([i, j, k], dtype=np.float64) * m.resolution         # :635
                if m.get_voxel_state(grid, box) != 0:                                     # :636
                    return False                                                          # :638
    return True                                                                           # :642


def goal_search_table():
    """The offsets of m:299-305 from the three loops as written; theta counts degrees and goes into cos / sin unconverted (the
    reference's behaviour).  Returns (rows [(r cos theta, r sin theta, nz)], sizes of the nz loops in order)."""
    dr, dtheta, dz = 0.2, 30, 0.2                                                         # m:295
    rows, sizes = [], []
    r = dr
    while r <= 5 * dr + 1e-3:                                                             # m:299
        theta = float(-90)
        while theta <= 270:                                                               # m:300
            n = 0
            nz = 1.0
            while nz <= 1.6:                                                              # m:301
                rows.append((r * math.cos(theta), r * math.sin(theta), nz))               # m:303-305
                n += 1
                nz += dz
            sizes.append(n)
            theta += dtheta
        r += dr
    return rows, sizes


def check_goal(m, end_pt, have_target=True, box=None, body=(EGO_R, EGO_H)):
    """m:289-316 for one planner.  Returns (end_pt afterwards, goal_blocked, goal_hits)."""
    end_pt = np.array(end_pt, dtype=np.float64)
    blocked, hits = 0, 0
    if have_target:                                                                       # m:289
        if not check_pos_surround(m, end_pt, 1.2, box, body):                             # m:291
            blocked = 1
            dr, dtheta, dz = 0.2, 30, 0.2                                                 # m:295
            r = dr
            while r <= 5 * dr + 1e-3:                                                     # m:299
                theta = float(-90)
                while theta <= 270:                                                       # m:300
                    nz = 1.0
                    while nz <= 1.6:                                                      # m:301
                        new_x = end_pt[0] + r * math.cos(theta)                           # m:303
                        new_y = end_pt[1] + r * math.sin(theta)                           # m:304
                        new_z = nz                                                        # m:305
                        new_pt = np.array([new_x, new_y, new_z], dtype=np.float64)        # m:307
                        if check_pos_surround(m, new_pt, 1.5, box, body):                 # m:308
                            end_pt = new_pt                                               # m:309
                            hits += 1
                            break                                                         # m:312 (the nz loop only)
                        nz += dz
                    theta += dtheta
                r += dr
    return end_pt, blocked, hits


def check_path(m, kino_path, kino_size, have_traj=True, box=None, stride=5, body=(EGO_R, EGO_H)):
    """m:329-340 for one planner: the index of the first colliding sample among 0, stride, ... < kino_size, or -1.  kino_path [K,3]
    is storage of K samples of which kino_size are the path (kino_path_.size())."""
    if have_traj:                                                                         # m:329
        for i in range(0, min(int(kino_size), len(kino_path)), stride):                   # m:331
            if not check_pos_surround(m, kino_path[i], 1.2, box, body):                   # m:333
                return i                                                                  # m:335-337
    return -1
