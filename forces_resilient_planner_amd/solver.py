"""ctypes binding of the C-ABI in include/frp_nmpc.h (libfrp_nmpc_amd.so).

The product path: every function here runs HIP kernels on the MI355X; there is no CPU fallback --
if the library is missing or no device is visible the calls raise.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import layout as L

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FRP_LIB") or os.path.join(_PKG, "libfrp_nmpc_amd.so")  # FRP_LIB: an experiment build (tools/build_variant.sh)
INFO_STRIDE = 12
ABI_VERSION = 7  # FRP_NMPC_ABI_VERSION of include/frp_nmpc.h

c_double_p = ctypes.POINTER(ctypes.c_double)
c_int_p = ctypes.POINTER(ctypes.c_int)


class Options(ctypes.Structure):
    _fields_ = [("maxit", ctypes.c_int), ("tol_stat", ctypes.c_double), ("tol_eq", ctypes.c_double),
                ("tol_ineq", ctypes.c_double), ("tol_comp", ctypes.c_double), ("mu0", ctypes.c_double),
                ("ftb", ctypes.c_double), ("hessian", ctypes.c_int), ("diverge_mu", ctypes.c_double), ("twist", ctypes.c_int),
                ("timeout", ctypes.c_double)]  # seconds of wall clock per scope, 0 = no budget (frp_nmpc_options.timeout)


class Batch(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("N", ctypes.c_int), ("M", ctypes.c_int), ("MF", ctypes.c_int),
                ("model", ctypes.c_int),
                ("xinit", ctypes.c_void_p), ("x0", ctypes.c_void_p), ("params", ctypes.c_void_p),
                ("nfaces", ctypes.c_void_p), ("z", ctypes.c_void_p), ("exitflag", ctypes.c_void_p),
                ("iters", ctypes.c_void_p), ("info", ctypes.c_void_p), ("model_per_problem", ctypes.c_void_p),
                ("order_hint", ctypes.c_void_p)]


class Pack(ctypes.Structure):  # frp_nmpc_pack (include/frp_nmpc.h)
    _fields_ = [("B", ctypes.c_int), ("N", ctypes.c_int), ("M", ctypes.c_int), ("NPOLY", ctypes.c_int), ("F", ctypes.c_int),
                ("external_acc_per_stage", ctypes.c_int), ("mpc_output", ctypes.c_void_p), ("external_acc", ctypes.c_void_p), ("ref_pos", ctypes.c_void_p),
                ("ref_yaw", ctypes.c_void_p), ("ellipsoid", ctypes.c_void_p), ("poly_A", ctypes.c_void_p),
                ("poly_b", ctypes.c_void_p), ("poly_nfaces", ctypes.c_void_p), ("poly_index", ctypes.c_void_p),
                ("w_stage_wp", ctypes.c_double), ("w_stage_input", ctypes.c_double), ("w_input_rate", ctypes.c_double),
                ("w_terminal_wp", ctypes.c_double), ("w_terminal_input", ctypes.c_double),
                ("xinit", ctypes.c_void_p), ("x0", ctypes.c_void_p), ("params", ctypes.c_void_p), ("nfaces", ctypes.c_void_p),
                ("mode", ctypes.c_void_p), ("wf_stage_wp", ctypes.c_double), ("wf_stage_input", ctypes.c_double),
                ("wf_input_rate", ctypes.c_double), ("wf_terminal_wp", ctypes.c_double), ("wf_terminal_input", ctypes.c_double),
                ("padded_rows_are_zero", ctypes.c_int)]


class Tube(ctypes.Structure):  # frp_nmpc_tube (include/frp_nmpc.h)
    _fields_ = [("B", ctypes.c_int), ("N", ctypes.c_int), ("mpc_output", ctypes.c_void_p),
                ("mass", ctypes.c_double), ("drag", ctypes.c_double), ("ego_r", ctypes.c_double), ("ego_h", ctypes.c_double),
                ("noise", ctypes.c_double * 3), ("epsilon", ctypes.c_double), ("Ts", ctypes.c_double),
                ("ellipsoid", ctypes.c_void_p)]


class Corridor(ctypes.Structure):  # frp_nmpc_corridor (include/frp_nmpc.h)
    _fields_ = [("B", ctypes.c_int), ("N", ctypes.c_int), ("F", ctypes.c_int), ("P", ctypes.c_int),
                ("cloud", ctypes.c_void_p), ("cloud_per_planner", ctypes.c_int), ("cloud_count", ctypes.c_void_p),
                ("ref_pos", ctypes.c_void_p), ("ref_yaw", ctypes.c_void_p), ("ellipsoid", ctypes.c_void_p),
                ("bbox", ctypes.c_double * 3), ("seed_len", ctypes.c_double), ("inflation", ctypes.c_double),
                ("offset_x", ctypes.c_double),
                ("poly_A", ctypes.c_void_p), ("poly_b", ctypes.c_void_p), ("poly_nfaces", ctypes.c_void_p),
                ("poly_index", ctypes.c_void_p), ("poly_count", ctypes.c_void_p),
                ("grid_origin", ctypes.c_double * 3), ("grid_cell", ctypes.c_double), ("grid_dims", ctypes.c_int * 3),
                ("grid_points", ctypes.c_void_p), ("grid_index", ctypes.c_void_p), ("grid_start", ctypes.c_void_p)]


class CorridorCut(ctypes.Structure):  # frp_nmpc_corridor_cut (include/frp_nmpc.h); the tensor behind .box is kept alive on ._box
    _fields_ = [("box", ctypes.c_void_p), ("origin", ctypes.c_double * 3), ("resolution", ctypes.c_double)]


class Reference(ctypes.Structure):  # frp_nmpc_reference (include/frp_nmpc.h)
    _fields_ = [("B", ctypes.c_int), ("N", ctypes.c_int), ("K", ctypes.c_int), ("kino_path", ctypes.c_void_p),
                ("path_per_planner", ctypes.c_int), ("kino_size", ctypes.c_void_p), ("time_offset", ctypes.c_void_p),
                ("mpc_output", ctypes.c_void_p), ("Ts", ctypes.c_double), ("pi", ctypes.c_double),
                ("ref_pos", ctypes.c_void_p), ("ref_yaw", ctypes.c_void_p), ("replan", ctypes.c_void_p)]


class Astar(ctypes.Structure):  # frp_nmpc_astar (include/frp_nmpc.h)
    _fields_ = [("B", ctypes.c_int), ("occ", ctypes.c_void_p), ("grid", ctypes.c_int * 3), ("origin", ctypes.c_double * 3),
                ("map_size", ctypes.c_double * 3), ("resolution", ctypes.c_double), ("local_box", ctypes.c_void_p),
                ("ego_r", ctypes.c_double), ("ego_h", ctypes.c_double),
                ("max_tau", ctypes.c_double), ("init_max_tau", ctypes.c_double), ("max_vel", ctypes.c_double), ("max_acc", ctypes.c_double),
                ("w_time", ctypes.c_double), ("horizon", ctypes.c_double), ("lambda_heu", ctypes.c_double), ("tie_breaker", ctypes.c_double),
                ("allocate_num", ctypes.c_int), ("check_num", ctypes.c_int),
                ("start_pt", ctypes.c_void_p), ("start_vel", ctypes.c_void_p), ("start_acc", ctypes.c_void_p), ("end_pt", ctypes.c_void_p),
                ("end_vel", ctypes.c_void_p), ("external_acc", ctypes.c_void_p), ("active", ctypes.c_void_p), ("init_search", ctypes.c_int),
                ("Ts", ctypes.c_double), ("K", ctypes.c_int),
                ("kino_path", ctypes.c_void_p), ("kino_size", ctypes.c_void_p), ("status", ctypes.c_void_p), ("stats", ctypes.c_void_p),
                ("path_nodes", ctypes.c_void_p), ("retry_pt", ctypes.c_void_p), ("retry_vel", ctypes.c_void_p)]


class OccMap(ctypes.Structure):  # frp_nmpc_occmap (include/frp_nmpc.h)
    _fields_ = [("origin", ctypes.c_double * 3), ("map_size", ctypes.c_double * 3), ("resolution", ctypes.c_double), ("grid", ctypes.c_int * 3),
                ("clamp_min_log", ctypes.c_double), ("clamp_max_log", ctypes.c_double), ("min_occupancy_log", ctypes.c_double),
                ("local_radius", ctypes.c_double * 3), ("log_odds", ctypes.c_void_p), ("occ", ctypes.c_void_p)]


class OccMapView(ctypes.Structure):  # frp_nmpc_occmap_view (include/frp_nmpc.h)
    _fields_ = [("B", ctypes.c_int), ("centre", ctypes.c_void_p), ("P", ctypes.c_int), ("local_box", ctypes.c_void_p),
                ("cloud", ctypes.c_void_p), ("cloud_count", ctypes.c_void_p)]


class OccMapFuse(ctypes.Structure):  # frp_nmpc_occmap_fuse (include/frp_nmpc_occmap_fuse.h)
    _fields_ = [("rows", ctypes.c_int), ("cols", ctypes.c_int), ("depth", ctypes.c_void_p), ("last_depth", ctypes.c_void_p),
                ("last_T_wc", ctypes.c_double * 16), ("K", ctypes.c_double * 9), ("T_wc", ctypes.c_double * 16),
                ("depth_scale", ctypes.c_double), ("depth_filter_mindist", ctypes.c_double), ("depth_filter_tolerance", ctypes.c_double),
                ("depth_filter_margin", ctypes.c_int), ("skip_pixel", ctypes.c_int),
                ("prob_hit_log", ctypes.c_double), ("prob_miss_log", ctypes.c_double),
                ("min_ray_length", ctypes.c_double), ("max_ray_length", ctypes.c_double),
                ("max_rounds", ctypes.c_int), ("status", ctypes.c_void_p)]


class OccMapFuseBatch(ctypes.Structure):  # frp_nmpc_occmap_fuse_batch (include/frp_nmpc_occmap_fuse_batch.h)
    _fields_ = [("frames", ctypes.c_int), ("rows", ctypes.c_int), ("cols", ctypes.c_int), ("depth", ctypes.c_void_p), ("last_depth", ctypes.c_void_p),
                ("T_wc", ctypes.c_void_p), ("last_T_wc", ctypes.c_void_p), ("active", ctypes.c_void_p), ("K", ctypes.c_double * 9),
                ("depth_scale", ctypes.c_double), ("depth_filter_mindist", ctypes.c_double), ("depth_filter_tolerance", ctypes.c_double),
                ("depth_filter_margin", ctypes.c_int), ("skip_pixel", ctypes.c_int),
                ("prob_hit_log", ctypes.c_double), ("prob_miss_log", ctypes.c_double),
                ("min_ray_length", ctypes.c_double), ("max_ray_length", ctypes.c_double),
                ("max_rounds", ctypes.c_int), ("status", ctypes.c_void_p)]


class OccMapFusePoints(ctypes.Structure):  # frp_nmpc_occmap_fuse_points (include/frp_nmpc_occmap_fuse_points.h)
    _fields_ = [("scans", ctypes.c_int), ("P", ctypes.c_int), ("points", ctypes.c_void_p), ("points_f32", ctypes.c_void_p),
                ("count", ctypes.c_void_p), ("origin", ctypes.c_void_p), ("active", ctypes.c_void_p),
                ("prob_hit_log", ctypes.c_double), ("prob_miss_log", ctypes.c_double),
                ("min_ray_length", ctypes.c_double), ("max_ray_length", ctypes.c_double),
                ("max_rounds", ctypes.c_int), ("status", ctypes.c_void_p)]


class OccMapRender(ctypes.Structure):  # frp_nmpc_occmap_render (include/frp_nmpc_occmap_render.h)
    _fields_ = [("frames", ctypes.c_int), ("rows", ctypes.c_int), ("cols", ctypes.c_int), ("T_wc", ctypes.c_void_p), ("active", ctypes.c_void_p),
                ("K", ctypes.c_double * 9), ("depth_scale", ctypes.c_double), ("max_range", ctypes.c_double),
                ("depth", ctypes.c_void_p), ("voxel", ctypes.c_void_p), ("status", ctypes.c_void_p)]


class OccMapRenderScan(ctypes.Structure):  # frp_nmpc_occmap_render_scan (include/frp_nmpc_occmap_render_scan.h)
    _fields_ = [("scans", ctypes.c_int), ("P", ctypes.c_int), ("beams", ctypes.c_void_p), ("T_ws", ctypes.c_void_p), ("active", ctypes.c_void_p),
                ("min_range", ctypes.c_double), ("max_range", ctypes.c_double), ("far_range", ctypes.c_double),
                ("points", ctypes.c_void_p), ("points_f32", ctypes.c_void_p), ("origin", ctypes.c_void_p), ("count", ctypes.c_void_p),
                ("range", ctypes.c_void_p), ("voxel", ctypes.c_void_p), ("status", ctypes.c_void_p)]


class OccMapSharedView(ctypes.Structure):  # frp_nmpc_occmap_shared_view (include/frp_nmpc_occmap_view.h)
    _fields_ = [("cap", ctypes.c_int), ("cell", ctypes.c_double), ("dims", ctypes.c_int * 3),
                ("cloud", ctypes.c_void_p), ("count", ctypes.c_void_p), ("total", ctypes.c_void_p),
                ("grid_points", ctypes.c_void_p), ("grid_index", ctypes.c_void_p), ("grid_start", ctypes.c_void_p),
                ("cursor", ctypes.c_void_p), ("group_sums", ctypes.c_void_p)]


class CorridorLarge(ctypes.Structure):  # frp_nmpc_corridor_large (include/frp_nmpc_corridor_large.h)
    _fields_ = [("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t), ("overflow", ctypes.c_void_p)]


class Command(ctypes.Structure):  # frp_nmpc_command (include/frp_nmpc_command.h)
    _fields_ = [("B", ctypes.c_int), ("N", ctypes.c_int), ("S", ctypes.c_int), ("Ts", ctypes.c_double), ("mass", ctypes.c_double), ("g", ctypes.c_double),
                ("pre_plan", ctypes.c_void_p), ("t_cur", ctypes.c_void_p), ("status", ctypes.c_void_p), ("have_traj", ctypes.c_void_p),
                ("pub_end", ctypes.c_void_p), ("end_pt", ctypes.c_void_p), ("odom", ctypes.c_void_p), ("init_yaw", ctypes.c_void_p),
                ("t_yaw", ctypes.c_void_p), ("cmd", ctypes.c_void_p), ("kind", ctypes.c_void_p), ("finish", ctypes.c_void_p),
                ("reset_output", ctypes.c_void_p)]


class Tick(ctypes.Structure):  # frp_nmpc_tick (include/frp_nmpc_outcome.h)
    _fields_ = [("B", ctypes.c_int)] + [(n, ctypes.c_void_p) for n in ("fail_count", "replan_count", "kino_replan", "exit_code", "initialized", "cmd_status",
                                                                        "pub_end", "cmd_end_pt", "exec_mpc", "gate", "keep", "accept", "result", "replan")]


class TickIn(ctypes.Structure):  # frp_nmpc_tick_in (include/frp_nmpc_outcome.h)
    _fields_ = [("N", ctypes.c_int), ("K", ctypes.c_int), ("Ts", ctypes.c_double), ("z", ctypes.c_void_p), ("exitflag", ctypes.c_void_p),
                ("mpc_output", ctypes.c_void_p), ("state", ctypes.c_void_p), ("end_pt", ctypes.c_void_p), ("end_per_planner", ctypes.c_int),
                ("kino_path", ctypes.c_void_p), ("path_per_planner", ctypes.c_int), ("kino_size", ctypes.c_void_p), ("size_per_planner", ctypes.c_int),
                ("time_offset", ctypes.c_void_p), ("ref_replan", ctypes.c_void_p), ("mode", ctypes.c_void_p)]


class Fsm(ctypes.Structure):  # frp_nmpc_fsm (include/frp_nmpc_fsm.h)
    _fields_ = [("B", ctypes.c_int)] + [(n, ctypes.c_void_p) for n in ("state", "have_odom", "have_target", "have_traj", "trigger", "call_init_yaw",
                                                                        "consider_force", "replan_force_surpass", "surpass_count", "plan_fail_count",
                                                                        "exec_mpc", "cmd_status", "pub_end", "end_pt", "external_acc", "last_external_acc",
                                                                        "init_yaw", "yaw_odom", "change_yaw_time", "kino_start_time", "mode")]


class FsmExecIn(ctypes.Structure):  # frp_nmpc_fsm_exec_in (include/frp_nmpc_fsm.h)
    _fields_ = [("N", ctypes.c_int), ("Ts", ctypes.c_double), ("mass", ctypes.c_double), ("g", ctypes.c_double)] + \
               [(n, ctypes.c_void_p) for n in ("state", "pre_plan", "exit_code", "t_cur", "now", "search", "start_pt", "start_vel", "start_acc",
                                               "retry_pt", "retry_vel")]


class VehicleArgs(ctypes.Structure):  # frp_nmpc_vehicle (include/frp_nmpc_vehicle.h)
    _fields_ = [("B", ctypes.c_int), ("S", ctypes.c_int), ("n_sub", ctypes.c_int), ("mass", ctypes.c_double), ("g", ctypes.c_double), ("dt_cmd", ctypes.c_double),
                ("kp", ctypes.c_double * 3), ("kv", ctypes.c_double * 3), ("ka", ctypes.c_double * 3)] + \
               [(n, ctypes.c_void_p) for n in ("x", "f_true", "cmd", "kind", "hold", "trace", "sat")]


class EstimatorArgs(ctypes.Structure):  # frp_nmpc_estimator (include/frp_nmpc_estimator.h)
    _fields_ = [("B", ctypes.c_int), ("S", ctypes.c_int), ("min_samples", ctypes.c_int), ("dt", ctypes.c_double), ("alpha", ctypes.c_double)] + \
               [(n, ctypes.c_void_p) for n in ("meas", "thrust", "f_hat", "y_prev", "count", "force", "fresh", "residual", "status")]


class OccMapBody(ctypes.Structure):  # frp_nmpc_occmap_body (include/frp_nmpc_occmap_check.h)
    _fields_ = [("ego_r", ctypes.c_double), ("ego_h", ctypes.c_double)]


ASTAR_MAX_PATH = 256
ASTAR_REACH_HORIZON, ASTAR_REACH_END, ASTAR_NO_PATH, ASTAR_REACH_END_BUT_SHOT_FAILS = 1, 2, 3, 4

REFERENCE_PI = 3.1415926  # nmpc_solver.cpp:3

# getSikangConst's constants (nmpc_solver.cpp:302, :318, :323)
CORRIDOR_DEFAULTS = dict(bbox=(2.0, 2.0, 1.0), seed_len=0.1, inflation=1.1, offset_x=0.0)
CORRIDOR_MAX_F = 64
CORRIDOR_MAX_POINTS = 65536

# OccMap's ROS parameter defaults (occ_map.cpp:752-754) and the local range of the reference's launch files
OCCMAP_DEFAULTS = dict(clamp_min_log=0.12, clamp_max_log=0.97, min_occupancy_log=0.80, local_radius=(6.0, 6.0, 3.0))

# depth fusion: the occ_map/* values of the reference's launch file (plan_manage/launch/advanced_param.xml:69-92); max_rounds 0 = the
# library's default number of relaxation rounds (FRP_OCCMAP_FUSE_DEFAULT_ROUNDS)
OCCMAP_FUSE_DEFAULTS = dict(depth_scale=1000.0, depth_filter_mindist=0.1, depth_filter_tolerance=0.2, depth_filter_margin=1, skip_pixel=2,
                            prob_hit_log=1.2, prob_miss_log=-0.5, min_ray_length=0.1, max_ray_length=6.0, max_rounds=0)
OCCMAP_FUSE_DEFAULT_ROUNDS = 128  # FRP_OCCMAP_FUSE_DEFAULT_ROUNDS
# section (8)'s second header (include/frp_nmpc_occmap_fuse.h): checked at load time like EXPORTS
FUSE_EXPORTS = ["frp_nmpc_occmap_fuse_workspace_bytes", "frp_nmpc_occmap_fuse_depth"]
# ... and its batched form (include/frp_nmpc_occmap_fuse_batch.h): F frames per call, poses read on the device
FUSE_BATCH_EXPORTS = ["frp_nmpc_occmap_fuse_batch_workspace_bytes", "frp_nmpc_occmap_fuse_depth_batch"]
OCCMAP_FUSE_MAX_FRAMES = 64     # FRP_OCCMAP_FUSE_MAX_FRAMES
OCCMAP_FUSE_REFUSED = -256      # FRP_OCCMAP_FUSE_REFUSED: status[f][0] of a frame whose pose the device refuses
# ... and the same ray casting for point scans (include/frp_nmpc_occmap_fuse_points.h): S clouds with their sensor positions per call
FUSE_POINTS_EXPORTS = ["frp_nmpc_occmap_fuse_points_workspace_bytes", "frp_nmpc_occmap_fuse_points_batch"]
OCCMAP_FUSE_POINTS_MAX_SCANS = 64    # FRP_OCCMAP_FUSE_POINTS_MAX_SCANS
OCCMAP_FUSE_POINTS_PARAMS = ("prob_hit_log", "prob_miss_log", "min_ray_length", "max_ray_length", "max_rounds")  # the keys of OCCMAP_FUSE_DEFAULTS a point scan has

# section (8)'s fifth header (include/frp_nmpc_occmap_render.h): depth images rendered from the map, camera poses from planner states
RENDER_EXPORTS = ["frp_nmpc_occmap_render_depth", "frp_nmpc_occmap_camera_poses"]
# ... and the same sensor for a table of beam directions (include/frp_nmpc_occmap_render_scan.h): the point scans fuse_points takes
RENDER_SCAN_EXPORTS = ["frp_nmpc_occmap_render_scan_batch"]

# section (8)'s sixth header (include/frp_nmpc_occmap_view.h): the shared view rebuilt on the device, and the corridor entry that takes it
VIEW_EXPORTS = ["frp_nmpc_occmap_shared_view_dims", "frp_nmpc_occmap_shared_view_update", "frp_nmpc_corridor_batch_view"]
CORRIDOR_MAX_CELLS = 1 << 22       # FRP_CORRIDOR_MAX_CELLS
OCCMAP_VIEW_MAX_GROUPS = 1024      # FRP_OCCMAP_VIEW_MAX_GROUPS
OCCMAP_VIEW_LAUNCHES = 5           # FRP_OCCMAP_VIEW_LAUNCHES

# section (8)'s seventh header (include/frp_nmpc_corridor_large.h): shared clouds beyond CORRIDOR_MAX_POINTS
LARGE_EXPORTS = ["frp_nmpc_corridor_large_workspace_bytes", "frp_nmpc_corridor_batch_large", "frp_nmpc_occmap_shared_view_update_large"]
CORRIDOR_LARGE_MAX_POINTS = 1 << 22  # FRP_CORRIDOR_LARGE_MAX_POINTS
CORRIDOR_LARGE_LIST = 65536          # FRP_CORRIDOR_LARGE_LIST
CORRIDOR_LARGE_GROUPS = 512          # FRP_CORRIDOR_LARGE_GROUPS

# section (8)'s third header (include/frp_nmpc_occmap_check.h): the safety timer's checks, checked at load time like EXPORTS
CHECK_EXPORTS = ["frp_nmpc_occmap_check_surround", "frp_nmpc_occmap_check_paths", "frp_nmpc_occmap_check_goals"]
OCCMAP_BODY = (0.27, 0.0425)  # occ_map/ego_r, ego_h of the reference's launch file
SAFETY_INFLATE_CHECK, SAFETY_INFLATE_SEARCH = 1.2, 1.5  # checkReplanCallback's two ratios (nmpc_manage.cpp:291, :308, :333)

# section (8)'s distance header (include/frp_nmpc_occmap_distance.h): the truncated distance field and the clearance queries, checked at
# load time like EXPORTS.  No reference counterpart: the reference's map keeps no distance
DISTANCE_EXPORTS = ["frp_nmpc_occmap_distance_scratch_bytes", "frp_nmpc_occmap_distance_update", "frp_nmpc_occmap_clearance",
                    "frp_nmpc_occmap_clearance_trace", "frp_nmpc_occmap_clearance_reset"]
OCCMAP_DIST_FAR, OCCMAP_DIST_MAX_R = 65535, 64  # FRP_OCCMAP_DIST_FAR, FRP_OCCMAP_DIST_MAX_R
# CHOSEN, not derived: a radius of 20 voxels is 2 m at the reference's 0.1 m resolution -- beyond it a clearance reads +inf
OCCMAP_DIST_DEFAULT_R = 20


# the command timer (include/frp_nmpc_command.h)
COMMAND_EXPORTS = ["frp_nmpc_command_snapshot", "frp_nmpc_command_batch"]
CMD_INIT_POSITION, CMD_ROTATE_YAW, CMD_PUB_END, CMD_PUB_TRAJ, CMD_WAIT = range(5)  # FRP_CMD_*: enum CMD_STATUS (nmpc_utils.h:115-122)
COMMAND_NONE, COMMAND_TRAJ, COMMAND_END, COMMAND_YAW, COMMAND_NO_YAW_INPUT = 0, 1, 2, 3, -1  # FRP_COMMAND_*: kind[b][s]
COMMAND_STRIDE = 16  # FRP_COMMAND_STRIDE: position 0-2, quaternion x y z w 3-6, linear velocity 7-9, body rates 10-12, linear acceleration 13-15
COMMAND_DEFAULTS = dict(Ts=0.05, mass=0.74, g=9.81)  # nmpc_utils.h:189, nmpc/mass, the g of nmpc_solver.cpp

# the tick outcome (include/frp_nmpc_outcome.h)
OUTCOME_EXPORTS = ["frp_nmpc_tick_begin", "frp_nmpc_tick_end"]
TICK_RUN, TICK_IDLE, TICK_AT_END, TICK_ENDING = range(4)  # FRP_TICK_*: gate[b]
TICK_RESULT_IDLE = -4  # FRP_TICK_RESULT_IDLE: result[b] of a planner whose mpcCallback returned before solveNMPC

# the fleet state machine (include/frp_nmpc_fsm.h)
FSM_EXPORTS = ["frp_nmpc_fsm_goal", "frp_nmpc_fsm_force", "frp_nmpc_fsm_mpc", "frp_nmpc_fsm_safety", "frp_nmpc_fsm_exec_begin", "frp_nmpc_fsm_exec_end"]
FSM_INIT, FSM_WAIT_TARGET, FSM_INIT_YAW, FSM_GEN_NEW_TRAJ, FSM_REPLAN_TRAJ, FSM_EXEC_TRAJ = range(6)  # FRP_FSM_*: enum FSM_EXEC_STATE, in its order
FSM_EXT_NOISE_BOUND = 0.5  # nmpc/ext_noise_bound (nmpc_manage.cpp:13)
FSM_EXEC_PERIOD = 0.01     # the period of exec_timer_ (nmpc_manage.cpp:44) = that of the command timer

# the vehicle (include/frp_nmpc_vehicle.h)
VEHICLE_EXPORTS = ["frp_nmpc_vehicle_step", "frp_nmpc_vehicle_reset", "frp_nmpc_vehicle_message", "frp_nmpc_vehicle_odometry"]
VEHICLE_STATE, VEHICLE_HOLD_STRIDE, VEHICLE_MSG_STRIDE, VEHICLE_MAX_SUB = 9, 8, 13, 16  # FRP_VEHICLE_*
ODOM_WORLD, ODOM_BODY = 1, 2  # FRP_ODOM_*: odometryCallback, odometryTransCallback
VEHICLE_SAT_THRUST_LO, VEHICLE_SAT_THRUST_HI, VEHICLE_SAT_ROLL, VEHICLE_SAT_PITCH, VEHICLE_SAT_RATE0, VEHICLE_SAT_ZERO_ACC, VEHICLE_SAT_YAW_WRAP = 1, 2, 4, 8, 16, 128, 256
# the controller's gains (no reference counterpart: the reference flies RotorS' controller) and what it is told; mass and g are the
# plant's own (csrc/frp_model.hpp), dt_cmd the command timer's period
VEHICLE_DEFAULTS = dict(kp=(6.0, 6.0, 8.0), kv=(4.0, 4.0, 5.0), ka=(10.0, 10.0, 4.0), mass=0.745319, g=9.81, dt_cmd=FSM_EXEC_PERIOD, n_sub=4)

# the force estimator (include/frp_nmpc_estimator.h)
ESTIMATOR_EXPORTS = ["frp_nmpc_vehicle_step_observed", "frp_nmpc_estimator_update", "frp_nmpc_estimator_reset"]
EST_SKIPPED, EST_FIRST, EST_ABSORBED = 0, 1, 2  # FRP_EST_*: status[b][s]
# CHOSEN, not derived (the reference has no estimator: its wrench comes from another node): a filter time constant of 0.1 s -- two of the
# planner's 50 ms periods, alpha = 1 - exp(-0.01 / 0.1) = 0.095 per 100 Hz sample, a step of 1 m/s^2 passes ext_noise_bound = 0.5 after
# 7 samples --, and an estimate that counts as fresh once 10 residuals (two periods) went into it
ESTIMATOR_DEFAULTS = dict(tau=0.1, min_samples=10)


def goal_search_table():
    """The candidate offsets of checkReplanCallback's goal search (plan_manage/src/nmpc_manage.cpp:295-305), from its three loops run
    as written: r and nz are accumulated in double (r += dr, nz += dz) against `r <= 5 * dr + 1e-3` and `nz <= 1.6`, and theta
    runs over DEGREES (-90 ... 270 in steps of 30) but is handed to cos / sin as it is, i.e. as RADIANS -- that is the reference's
    behaviour, kept.  Row c is (r * cos(theta), r * sin(theta), nz): the device adds the first two to the goal and takes the third
    as the new z.  Returns (table [n_groups * group_size, 3] float64, n_groups, group_size); a group is one (r, theta) pair's nz
    loop, the loop the reference's `break` leaves.  The counts come from the loops (5 * 13 groups of 4 in IEEE double)."""
    import math
    dr, dtheta, dz = 0.2, 30.0, 0.2                                       # :295
    rows, sizes = [], []
    r = dr
    while r <= 5 * dr + 1e-3:                                             # :299
        theta = -90.0
        while theta <= 270:                                               # :300
            n = 0
            nz = 1.0
            while nz <= 1.6:                                              # :301
                rows.append((r * math.cos(theta), r * math.sin(theta), nz))  # :303-305
                n += 1
                nz += dz
            sizes.append(n)
            theta += dtheta
        r += dr
    assert len(set(sizes)) == 1, sizes
    return np.array(rows, dtype=np.float64).reshape(-1, 3), len(sizes), sizes[0]


def lidar_beams(rings, columns, elevation_min, elevation_max, azimuth_span=2 * np.pi):
    """The beam table of a spinning LiDAR for OccupancyMap.render_scan: [rings * columns, 3] float64 unit vectors in the SENSOR frame
    (x forward, z up) in firing order, column-major -- all rings of azimuth 0, then the next azimuth --, so that the 64 consecutive
    beams of a wavefront point in nearby directions.  az_j = azimuth_span * j / columns, el_i = elevation_min + (elevation_max -
    elevation_min) * i / (rings - 1) (elevation_min when rings == 1), beam = (cos(el) cos(az), cos(el) sin(az), sin(el)).  A
    convenience: frp_nmpc_occmap_render_scan_batch takes any table."""
    rings, columns = int(rings), int(columns)
    if rings < 1 or columns < 1:
        raise ValueError("lidar_beams: at least one ring and one column")
    i, j = np.arange(rings, dtype=np.float64), np.arange(columns, dtype=np.float64)
    el = np.full(rings, float(elevation_min)) if rings == 1 else float(elevation_min) + (float(elevation_max) - float(elevation_min)) * i / (rings - 1)
    az = float(azimuth_span) * j / columns
    out = np.empty((columns, rings, 3), dtype=np.float64)
    out[:, :, 0] = np.cos(el)[None, :] * np.cos(az)[:, None]
    out[:, :, 1] = np.cos(el)[None, :] * np.sin(az)[:, None]
    out[:, :, 2] = np.sin(el)[None, :]
    return out.reshape(rings * columns, 3)


class SafetyCheck:
    """What OccupancyMap.safety_check returns (int32 [B] device tensors): goal_blocked (the goal collided at ratio 1.2), goal_hits (how
    often the search moved it), first_hit (smallest colliding path sample, -1: none) and replan = goal_blocked | (first_hit >= 0),
    the mask DeviceFleet.replan(replan=...) and AstarPlanner.plan(active=...) take."""

    def __init__(self, goal_blocked, goal_hits, first_hit, replan):
        self.goal_blocked, self.goal_hits, self.first_hit, self.replan = goal_blocked, goal_hits, first_hit, replan


# ROS parameter defaults of the tube model (nmpc_solver.cpp:68-74, nmpc_utils.h:188-189)
TUBE_DEFAULTS = dict(mass=0.74, drag=0.33, ego_r=0.27, ego_h=0.0425, noise=(0.5, 0.5, 0.5), epsilon=0.06, Ts=0.05)


class ForcesParams(ctypes.Structure):
    _fields_ = [("xinit", ctypes.c_double * 9), ("x0", ctypes.c_double * 340),
                ("all_parameters", ctypes.c_double * 2600), ("num_of_threads", ctypes.c_uint)]


class ForcesOutput(ctypes.Structure):
    _fields_ = [("x", (ctypes.c_double * 17) * 20)]


class ForcesInfo(ctypes.Structure):
    _fields_ = [("it", ctypes.c_int), ("it2opt", ctypes.c_int)] + \
               [(n, ctypes.c_double) for n in "res_eq res_ineq rsnorm rcompnorm pobj dobj dgap rdgap mu mu_aff sigma".split()] + \
               [("lsit_aff", ctypes.c_int), ("lsit_cc", ctypes.c_int)] + \
               [(n, ctypes.c_double) for n in "step_aff step_cc solvetime fevalstime".split()]


EXTFUNC = ctypes.CFUNCTYPE(None, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                           c_double_p, c_double_p, c_double_p, c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_int)

EXPORTS = ["frp_nmpc_default_options", "frp_nmpc_workspace_bytes", "frp_nmpc_solve_batch",
           "frp_nmpc_solve_batch_host", "frp_nmpc_stage_eval", "frp_nmpc_stage_eval_host", "frp_nmpc_time_solve",
           "frp_nmpc_version", "frp_nmpc_device_count", "FORCESNLPsolver_normal_solve",
           "FORCESNLPsolver_final_solve", "frp_nmpc_pack_batch", "frp_nmpc_update_batch", "frp_nmpc_tube_batch",
           "frp_nmpc_corridor_batch", "frp_nmpc_corridor_batch_cut", "frp_nmpc_reference_batch",
           "frp_nmpc_coldstart_batch", "frp_nmpc_cloud_grid_build",
           "frp_nmpc_mode_batch", "frp_nmpc_astar_batch", "frp_nmpc_astar_workspace_bytes",
           "frp_nmpc_kernel_timing_begin", "frp_nmpc_kernel_timing_end", "frp_nmpc_set_q4_min_batch",
           "frp_nmpc_abi_version", "frp_nmpc_abi_check", "frp_nmpc_host_register", "frp_nmpc_host_unregister",
           "frp_nmpc_host_registered", "frp_nmpc_host_unregister_all", "frp_nmpc_solve_batch_host_begin", "frp_nmpc_solve_batch_host_wait",
           "frp_nmpc_solver_variant", "frp_nmpc_occmap_workspace_bytes", "frp_nmpc_occmap_reset", "frp_nmpc_occmap_clear_box",
           "frp_nmpc_occmap_insert_cloud", "frp_nmpc_occmap_refresh", "frp_nmpc_occmap_local_view", "frp_nmpc_occmap_query"]

_lib = None


def lib():
    """Load libfrp_nmpc_amd.so (built in-tree by forces_resilient_planner_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        # PyTorch ships its own HIP runtime; the library links the system one.  Both coexist in one process as long
        # as torch's is initialised first (the reverse order leaves torch with "No HIP GPUs are available"), and
        # DeviceSolver / DeviceFleet hand torch-owned HBM to the library, so initialise torch here if it has a GPU.
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except ImportError:
            pass
        l = ctypes.CDLL(LIB_PATH)
        # the ctypes mirrors below against the library that was actually loaded (include/frp_nmpc.h: FRP_NMPC_ABI_CHECK): a stale
        # library would write another info stride into our arrays / read short option structs
        if not hasattr(l, "frp_nmpc_abi_check"):
            raise RuntimeError(f"{LIB_PATH} predates the ABI check (frp_nmpc.h ABI {ABI_VERSION}): rebuild it")
        l.frp_nmpc_abi_check.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
        if l.frp_nmpc_abi_check(ABI_VERSION, ctypes.sizeof(Options), ctypes.sizeof(Batch), INFO_STRIDE) != 0:
            raise RuntimeError(f"{LIB_PATH} was built from another include/frp_nmpc.h than these bindings (ABI {ABI_VERSION}, "
                               f"options {ctypes.sizeof(Options)} B, batch {ctypes.sizeof(Batch)} B, info stride {INFO_STRIDE})")
        l.frp_nmpc_workspace_bytes.restype = ctypes.c_size_t
        l.frp_nmpc_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
        l.frp_nmpc_version.restype = ctypes.c_char_p
        l.frp_nmpc_solve_batch.argtypes = [ctypes.POINTER(Batch), ctypes.POINTER(Options), ctypes.c_void_p,
                                           ctypes.c_size_t, ctypes.c_void_p]
        l.frp_nmpc_time_solve.argtypes = [ctypes.POINTER(Batch), ctypes.POINTER(Options), ctypes.c_void_p,
                                          ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
        l.frp_nmpc_solve_batch_host.argtypes = [ctypes.POINTER(Batch), ctypes.POINTER(Options)]
        l.frp_nmpc_set_q4_min_batch.argtypes = [ctypes.c_int]
        l.frp_nmpc_solver_variant.argtypes = [ctypes.POINTER(Batch), ctypes.POINTER(Options), ctypes.c_char_p, ctypes.c_size_t]
        l.frp_nmpc_host_register.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
        l.frp_nmpc_host_unregister.argtypes = [ctypes.c_void_p]
        l.frp_nmpc_host_registered.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
        l.frp_nmpc_solve_batch_host_begin.argtypes = [ctypes.POINTER(Batch), ctypes.POINTER(Options), ctypes.POINTER(ctypes.c_int)]
        l.frp_nmpc_solve_batch_host_wait.argtypes = [ctypes.c_int]
        l.frp_nmpc_kernel_timing_begin.argtypes = [ctypes.c_int, ctypes.c_int]
        l.frp_nmpc_kernel_timing_end.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]
        l.frp_nmpc_pack_batch.argtypes = [ctypes.POINTER(Pack), ctypes.c_void_p]
        l.frp_nmpc_update_batch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p]
        l.frp_nmpc_tube_batch.argtypes = [ctypes.POINTER(Tube), ctypes.c_void_p]
        l.frp_nmpc_corridor_batch.argtypes = [ctypes.POINTER(Corridor), ctypes.c_void_p]
        l.frp_nmpc_reference_batch.argtypes = [ctypes.POINTER(Reference), ctypes.c_void_p]
        if hasattr(l, "frp_nmpc_corridor_batch_cut"):  # (a library without it is refused by the EXPORTS check below)
            l.frp_nmpc_corridor_batch_cut.argtypes = [ctypes.POINTER(Corridor), ctypes.POINTER(CorridorCut), ctypes.c_void_p]
        l.frp_nmpc_cloud_grid_build.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        l.frp_nmpc_mode_batch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                          ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
        l.frp_nmpc_coldstart_batch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double,
                                               ctypes.c_void_p, ctypes.c_void_p]
        l.frp_nmpc_astar_workspace_bytes.restype = ctypes.c_size_t
        l.frp_nmpc_astar_workspace_bytes.argtypes = [ctypes.POINTER(Astar)]
        l.frp_nmpc_astar_batch.argtypes = [ctypes.POINTER(Astar), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        for name in EXPORTS + FUSE_EXPORTS + FUSE_BATCH_EXPORTS + FUSE_POINTS_EXPORTS + CHECK_EXPORTS + DISTANCE_EXPORTS + RENDER_EXPORTS + RENDER_SCAN_EXPORTS + VIEW_EXPORTS + LARGE_EXPORTS + COMMAND_EXPORTS + OUTCOME_EXPORTS + FSM_EXPORTS + VEHICLE_EXPORTS + ESTIMATOR_EXPORTS:  # a library without one of them is not this header's library: no call is ever skipped for a missing kernel
            if not hasattr(l, name):
                raise RuntimeError(f"{LIB_PATH} does not export {name}: rebuild it")
        pm, vp, sz = ctypes.POINTER(OccMap), ctypes.c_void_p, ctypes.c_size_t
        l.frp_nmpc_occmap_workspace_bytes.restype = ctypes.c_size_t
        l.frp_nmpc_occmap_workspace_bytes.argtypes = [pm]
        l.frp_nmpc_occmap_reset.argtypes = [pm, vp, sz, vp]
        l.frp_nmpc_occmap_refresh.argtypes = [pm, vp, sz, vp]
        l.frp_nmpc_occmap_clear_box.argtypes = [pm, c_double_p, c_double_p, vp, sz, vp]
        l.frp_nmpc_occmap_insert_cloud.argtypes = [pm, vp, ctypes.c_int, vp, sz, vp]
        l.frp_nmpc_occmap_local_view.argtypes = [pm, ctypes.POINTER(OccMapView), vp, sz, vp]
        l.frp_nmpc_occmap_query.argtypes = [pm, ctypes.c_int, vp, vp, vp, vp, vp, sz, vp]
        l.frp_nmpc_occmap_fuse_workspace_bytes.restype = ctypes.c_size_t
        l.frp_nmpc_occmap_fuse_workspace_bytes.argtypes = [pm, ctypes.POINTER(OccMapFuse)]
        l.frp_nmpc_occmap_fuse_depth.argtypes = [pm, ctypes.POINTER(OccMapFuse), vp, sz, vp, sz, vp]
        l.frp_nmpc_occmap_fuse_batch_workspace_bytes.restype = ctypes.c_size_t
        l.frp_nmpc_occmap_fuse_batch_workspace_bytes.argtypes = [pm, ctypes.POINTER(OccMapFuseBatch)]
        l.frp_nmpc_occmap_fuse_depth_batch.argtypes = [pm, ctypes.POINTER(OccMapFuseBatch), vp, sz, vp, sz, vp]
        l.frp_nmpc_occmap_fuse_points_workspace_bytes.restype = ctypes.c_size_t
        l.frp_nmpc_occmap_fuse_points_workspace_bytes.argtypes = [pm, ctypes.POINTER(OccMapFusePoints)]
        l.frp_nmpc_occmap_fuse_points_batch.argtypes = [pm, ctypes.POINTER(OccMapFusePoints), vp, sz, vp, sz, vp]
        l.frp_nmpc_occmap_render_depth.argtypes = [pm, ctypes.POINTER(OccMapRender), vp, sz, vp]
        l.frp_nmpc_occmap_camera_poses.argtypes = [ctypes.c_int, vp, c_double_p, vp, vp]
        l.frp_nmpc_occmap_shared_view_dims.argtypes = [pm, ctypes.c_double, ctypes.POINTER(ctypes.c_int * 3)]
        l.frp_nmpc_occmap_shared_view_update.argtypes = [pm, ctypes.POINTER(OccMapSharedView), vp, sz, vp]
        l.frp_nmpc_corridor_batch_view.argtypes = [ctypes.POINTER(Corridor), ctypes.POINTER(CorridorCut), vp]
        l.frp_nmpc_corridor_large_workspace_bytes.restype = ctypes.c_size_t
        l.frp_nmpc_corridor_large_workspace_bytes.argtypes = [ctypes.c_int]
        l.frp_nmpc_corridor_batch_large.argtypes = [ctypes.POINTER(Corridor), ctypes.POINTER(CorridorCut), ctypes.POINTER(CorridorLarge), vp]
        l.frp_nmpc_occmap_shared_view_update_large.argtypes = [pm, ctypes.POINTER(OccMapSharedView), vp, sz, vp]
        pb, ci, cd = ctypes.POINTER(OccMapBody), ctypes.c_int, ctypes.c_double
        l.frp_nmpc_occmap_check_surround.argtypes = [pm, pb, cd, ci, vp, vp, vp, vp, vp, sz, vp]
        l.frp_nmpc_occmap_check_paths.argtypes = [pm, pb, cd, ci, ci, ci, vp, vp, vp, vp, vp, vp, sz, vp]
        l.frp_nmpc_occmap_check_goals.argtypes = [pm, pb, cd, cd, ci, vp, vp, vp, ci, ci, vp, vp, vp, vp, sz, vp]
        l.frp_nmpc_occmap_distance_scratch_bytes.restype = ctypes.c_size_t
        l.frp_nmpc_occmap_distance_scratch_bytes.argtypes = [pm, ci]
        l.frp_nmpc_occmap_distance_update.argtypes = [pm, ci, ci, vp, vp, sz, vp, sz, vp]
        l.frp_nmpc_occmap_clearance.argtypes = [pm, vp, ci, ci, vp, vp, vp, vp]
        l.frp_nmpc_occmap_clearance_trace.argtypes = [pm, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]
        l.frp_nmpc_occmap_clearance_reset.argtypes = [ci, vp, vp, vp, vp, vp]
        l.frp_nmpc_command_snapshot.argtypes = [ci, ci, vp, vp, vp, vp, vp]
        l.frp_nmpc_command_batch.argtypes = [ctypes.POINTER(Command), vp]
        l.frp_nmpc_tick_begin.argtypes = [ctypes.POINTER(Tick), vp, vp]
        l.frp_nmpc_tick_end.argtypes = [ctypes.POINTER(Tick), ctypes.POINTER(TickIn), vp]
        pf = ctypes.POINTER(Fsm)
        l.frp_nmpc_fsm_goal.argtypes = [pf, vp, vp, vp]
        l.frp_nmpc_fsm_force.argtypes = [pf, vp, vp, cd, vp]
        l.frp_nmpc_fsm_mpc.argtypes = [pf, vp, vp]
        l.frp_nmpc_fsm_safety.argtypes = [pf, vp, vp, vp]
        l.frp_nmpc_fsm_exec_begin.argtypes = [pf, ctypes.POINTER(FsmExecIn), vp]
        l.frp_nmpc_fsm_exec_end.argtypes = [pf, vp, vp, vp, vp]
        l.frp_nmpc_vehicle_step.argtypes = [ctypes.POINTER(VehicleArgs), vp]
        l.frp_nmpc_vehicle_reset.argtypes = [ci, vp, vp, vp, vp, vp]
        l.frp_nmpc_vehicle_message.argtypes = [ci, ci, vp, vp, vp]
        l.frp_nmpc_vehicle_odometry.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp]
        l.frp_nmpc_vehicle_step_observed.argtypes = [ctypes.POINTER(VehicleArgs), vp, vp]
        l.frp_nmpc_estimator_update.argtypes = [ctypes.POINTER(EstimatorArgs), vp]
        l.frp_nmpc_estimator_reset.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp]
        _lib = l
    return _lib


def default_options(**kw) -> Options:
    o = Options()
    lib().frp_nmpc_default_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed with frp error {rc} (no HIP device / HIP error / bad argument; "
                           "this library has no CPU path)")


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
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        if not hasattr(self, "_piece_ws"):
            self._piece_ws = {}
        if piece not in self._piece_ws:
            self._piece_ws[piece] = self.ws if piece == 0 else self.torch.empty_like(self.ws)
        ws = self._piece_ws[piece]
        b = self._batch(lo, hi)
        _check(lib().frp_nmpc_solve_batch(ctypes.byref(b), ctypes.byref(self.opt), ws.data_ptr(), self.ws_bytes,
                                          ctypes.c_void_p(s.cuda_stream)), "frp_nmpc_solve_batch")

    def solve(self, stream=None):
        """Asynchronous launch on `stream` (a torch.cuda.Stream) or torch's current stream."""
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        b = self._batch()
        _check(lib().frp_nmpc_solve_batch(ctypes.byref(b), ctypes.byref(self.opt), self.ws.data_ptr(), self.ws_bytes,
                                          ctypes.c_void_p(s.cuda_stream)), "frp_nmpc_solve_batch")

    def time_solve(self, reps, stream=None):
        """Average kernel duration (ms) over `reps` launches, HIP events on the launch stream."""
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        b = self._batch()
        ms = ctypes.c_float(0)
        _check(lib().frp_nmpc_time_solve(ctypes.byref(b), ctypes.byref(self.opt), self.ws.data_ptr(), self.ws_bytes,
                                         ctypes.c_void_p(s.cuda_stream), reps, ctypes.byref(ms)), "frp_nmpc_time_solve")
        return ms.value


def kernel_timing_begin(max_launches, stride=1):
    """From here to kernel_timing_end() every `stride`-th solve launch carries a hipEvent pair around its dominant kernel (on its own stream)."""
    _check(lib().frp_nmpc_kernel_timing_begin(int(max_launches), int(stride)), "frp_nmpc_kernel_timing_begin")


def kernel_timing_end():
    """(average ms of the dominant kernel over the launches since kernel_timing_begin, number of launches)."""
    ms, n = ctypes.c_float(0), ctypes.c_int(0)
    _check(lib().frp_nmpc_kernel_timing_end(ctypes.byref(ms), ctypes.byref(n)), "frp_nmpc_kernel_timing_end")
    return ms.value, n.value


def tube_batch_device(mpc_output, ellipsoid, consts=None, stream=None):
    """frp_nmpc_tube_batch on device tensors: mpc_output [B,N+1,17] f64 -> ellipsoid [B,N,3,3] f64 (in place)."""
    import torch
    c = dict(TUBE_DEFAULTS)
    c.update(consts or {})
    B, rows, nz = mpc_output.shape
    assert nz == L.NZ and mpc_output.is_contiguous() and ellipsoid.is_contiguous() and mpc_output.dtype == torch.float64
    assert tuple(ellipsoid.shape) == (B, rows - 1, 3, 3) and ellipsoid.dtype == torch.float64
    s = stream if stream is not None else torch.cuda.current_stream(mpc_output.device)
    tb = Tube(B, rows - 1, mpc_output.data_ptr(), c["mass"], c["drag"], c["ego_r"], c["ego_h"],
              (ctypes.c_double * 3)(*c["noise"]), c["epsilon"], c["Ts"], ellipsoid.data_ptr())
    _check(lib().frp_nmpc_tube_batch(ctypes.byref(tb), ctypes.c_void_p(s.cuda_stream)), "frp_nmpc_tube_batch")


def reference_batch_device(kino_path, time_offset, mpc_output, ref_pos, ref_yaw, replan=None, kino_size=None, Ts=0.05,
                           stream=None):
    """frp_nmpc_reference_batch on device tensors: kino_path [K,3] (shared) or [B,K,3]; time_offset [B];
    mpc_output [B,N+1,17] -> ref_pos [B,N,3], ref_yaw [B,N], replan [B] int32."""
    import torch
    B, N, _ = ref_pos.shape
    per = 1 if kino_path.dim() == 3 else 0
    K = kino_path.shape[-2]
    for t in (kino_path, time_offset, mpc_output, ref_pos, ref_yaw):
        assert t.is_contiguous() and t.dtype == torch.float64
    assert tuple(mpc_output.shape) == (B, N + 1, L.NZ) and tuple(ref_yaw.shape) == (B, N) and tuple(time_offset.shape) == (B,)
    s = stream if stream is not None else torch.cuda.current_stream(ref_pos.device)
    rf = Reference(B, N, K, kino_path.data_ptr(), per, kino_size.data_ptr() if kino_size is not None else None,
                   time_offset.data_ptr(), mpc_output.data_ptr(), Ts, REFERENCE_PI, ref_pos.data_ptr(), ref_yaw.data_ptr(),
                   replan.data_ptr() if replan is not None else None)
    _check(lib().frp_nmpc_reference_batch(ctypes.byref(rf), ctypes.c_void_p(s.cuda_stream)), "frp_nmpc_reference_batch")


def reference_batch_host(kino_path, time_offset, mpc_output, kino_size=None, Ts=0.05, device="cuda:0"):
    """Host convenience: numpy in, (ref_pos [B,N,3], ref_yaw [B,N], replan [B]) out."""
    import torch
    lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)
    B, rows, _ = mpc_output.shape
    N = rows - 1
    rp = torch.zeros((B, N, 3), dtype=torch.float64, device=device); ry = torch.zeros((B, N), dtype=torch.float64, device=device)
    fl = torch.zeros((B,), dtype=torch.int32, device=device)
    ks = None if kino_size is None else torch.from_numpy(np.ascontiguousarray(kino_size, dtype=np.int32)).to(device)
    reference_batch_device(dev(kino_path), dev(time_offset), dev(mpc_output), rp, ry, fl, ks, Ts)
    torch.cuda.synchronize(device)
    return rp.cpu().numpy(), ry.cpu().numpy(), fl.cpu().numpy()


class Commands:
    """What command_batch_device / DeviceFleet.commands return (device tensors): cmd [B,S,16] f64 (position 0-2, quaternion x y z w 3-6,
    linear velocity 7-9, body rates 10-12, linear acceleration 13-15), kind [B,S] int32 (COMMAND_*), finish [B] int32 (finish_mpc_cmd_; written
    only where a callback touched it), reset_output [B] int32 (1 where PUB_END ran: cold-start that planner; written nowhere else) and
    status [B] int32, the caller's own tensor updated in place.  Pass the object back as `out` to reuse its buffers: finish and
    reset_output then carry over from call to call, as the reference's members do."""

    def __init__(self, cmd, kind, finish, reset_output, status):
        self.cmd, self.kind, self.finish, self.reset_output, self.status = cmd, kind, finish, reset_output, status


def command_snapshot_device(z, accept, pre_plan, have_traj, stream=None):
    """frp_nmpc_command_snapshot on device tensors: where accept [B] int32 != 0, pre_plan [B,N,17] <- z [B,N,17] (pre_mpc_output_ =
    mpc_output_, nmpc_solver.cpp:527, the solver's rows before the yaw wrap of :531-543) and have_traj [B] int32 <- 1."""
    import torch
    B, N, nz = z.shape
    assert nz == L.NZ and tuple(pre_plan.shape) == (B, N, L.NZ) and tuple(accept.shape) == (B,) and tuple(have_traj.shape) == (B,)
    assert z.dtype == pre_plan.dtype == torch.float64 and accept.dtype == have_traj.dtype == torch.int32
    assert z.is_contiguous() and pre_plan.is_contiguous() and accept.is_contiguous() and have_traj.is_contiguous()
    s = stream if stream is not None else torch.cuda.current_stream(z.device)
    vp = ctypes.c_void_p
    _check(lib().frp_nmpc_command_snapshot(B, N, vp(z.data_ptr()), vp(accept.data_ptr()), vp(pre_plan.data_ptr()), vp(have_traj.data_ptr()),
                                           vp(s.cuda_stream)), "frp_nmpc_command_snapshot")


def command_batch_device(pre_plan, have_traj, t_cur, status, pub_end, end_pt, odom=None, init_yaw=None, t_yaw=None, out=None, Ts=None,
                         mass=None, g=None, stream=None):
    """frp_nmpc_command_batch on device tensors: S consecutive callbacks of NMPCSolver::cmdTrajCallback (nmpc_solver.cpp:865-987) for
    each of B planners in one launch.  pre_plan [B,N,17] f64 + have_traj [B] int32 (command_snapshot_device), t_cur [B,S] f64 seconds
    since pre_mpc_start_time_, status [B] int32 CMD_* (updated IN PLACE), pub_end [B] int32, end_pt [B,3] f64; the yaw rotation's odom
    [B,9] f64, init_yaw [B] f64 and t_yaw [B,S] f64 seconds since change_yaw_time_: all three or none -- with none a planner in
    CMD_ROTATE_YAW gets kind COMMAND_NO_YAW_INPUT and zeros.  Ts, mass, g: COMMAND_DEFAULTS.  Returns a Commands object (out, when
    given: nothing is allocated then, so the call can be captured)."""
    import torch
    B, N, nz = pre_plan.shape
    assert nz == L.NZ and t_cur.dim() == 2 and t_cur.shape[0] == B
    S = t_cur.shape[1]
    yaw_in = (odom, init_yaw, t_yaw)
    if any(a is None for a in yaw_in) and not all(a is None for a in yaw_in):
        raise ValueError("odom, init_yaw and t_yaw go together: all three or none (frp_nmpc_command.odom)")
    f64 = [(pre_plan, (B, N, L.NZ)), (t_cur, (B, S)), (end_pt, (B, 3))] + ([(odom, (B, 9)), (init_yaw, (B,)), (t_yaw, (B, S))] if odom is not None else [])
    i32 = [(status, (B,)), (have_traj, (B,)), (pub_end, (B,))]
    dev = pre_plan.device
    if out is None:
        out = Commands(torch.zeros((B, S, COMMAND_STRIDE), dtype=torch.float64, device=dev), torch.zeros((B, S), dtype=torch.int32, device=dev),
                       torch.zeros((B,), dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev), status)
    out.status = status
    f64.append((out.cmd, (B, S, COMMAND_STRIDE)))
    i32 += [(out.kind, (B, S)), (out.finish, (B,)), (out.reset_output, (B,))]
    for t, shape in f64:
        assert t.dtype == torch.float64 and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev, (tuple(t.shape), shape, t.dtype)
    for t, shape in i32:
        assert t.dtype == torch.int32 and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev, (tuple(t.shape), shape, t.dtype)
    k = dict(COMMAND_DEFAULTS)
    k.update({n: float(v) for n, v in (("Ts", Ts), ("mass", mass), ("g", g)) if v is not None})
    ptr = lambda a: a.data_ptr() if a is not None else None
    c = Command(B, N, S, k["Ts"], k["mass"], k["g"], pre_plan.data_ptr(), t_cur.data_ptr(), status.data_ptr(), have_traj.data_ptr(),
                pub_end.data_ptr(), end_pt.data_ptr(), ptr(odom), ptr(init_yaw), ptr(t_yaw), out.cmd.data_ptr(), out.kind.data_ptr(),
                out.finish.data_ptr(), out.reset_output.data_ptr())
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    _check(lib().frp_nmpc_command_batch(ctypes.byref(c), ctypes.c_void_p(s.cuda_stream)), "frp_nmpc_command_batch")
    return out


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
        s = stream if stream is not None else torch.cuda.current_stream(self.gate.device)
        if reset_output is not None:
            assert reset_output.dtype == torch.int32 and tuple(reset_output.shape) == (self.B,) and reset_output.is_contiguous()
        t = self.struct()
        _check(lib().frp_nmpc_tick_begin(ctypes.byref(t), ctypes.c_void_p(reset_output.data_ptr()) if reset_output is not None else None,
                                         ctypes.c_void_p(s.cuda_stream)), "frp_nmpc_tick_begin")

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
        s = stream if stream is not None else torch.cuda.current_stream(z.device)
        t = self.struct()
        i = TickIn(N, K, float(Ts), z.data_ptr(), exitflag.data_ptr(), mpc_output.data_ptr(), state.data_ptr(), end_pt.data_ptr(), int(per_end),
                   kino_path.data_ptr(), int(per_path), kino_size.data_ptr(), int(per_size), time_offset.data_ptr(), ref_replan.data_ptr(),
                   mode.data_ptr() if mode is not None else None)
        _check(lib().frp_nmpc_tick_end(ctypes.byref(t), ctypes.byref(i), ctypes.c_void_p(s.cuda_stream)), "frp_nmpc_tick_end")


class LocalView:
    """What OccupancyMap.local_view returns (device tensors): local_box [B,6] int32 for AstarPlanner.plan / DeviceFleet.replan,
    cloud [B,P,3] f64 + cloud_count [B] int32 for corridor_batch_device / DeviceFleet.full_tick."""

    def __init__(self, local_box, cloud, cloud_count):
        self.local_box, self.cloud, self.cloud_count = local_box, cloud, cloud_count

    def overflowed(self):
        """Planners with more occupied voxels in range than the view stores (their count is minus the true one)."""
        return self.cloud_count < 0


class OccupancyMap:
    """The reference's OccMap (occ_grid/src/occ_map.cpp) in HBM, shared by all planners (frp_nmpc_occmap_*): the log-odds buffer,
    the byte grid the A* searches (.occ) and, per planner, the local box and the local obstacle cloud the corridor takes.
    world: the dict of workloads.astar_world -- its geometry, and its occ as the initial content (occupied voxels at
    clamp_max_log, the others at clamp_min_log); or explicit origin / map_size / resolution for an empty map.  fuse_depth() fuses a
    camera frame by ray casting (projectDepthImage / raycastProcess, include/frp_nmpc_occmap_fuse.h) with the reference's serial
    result to the bit, fuse_points() does the same ray casting for point scans (a LiDAR's cloud and the position it was taken from); a
    caller with another fusion of its own writes .log_odds and calls refresh().  render_depth() is the other
    direction: the depth images cameras at given poses see of this map (a ground-truth world feeding a belief map's fuse_depth_batch),
    and render_scan() the point scans a LiDAR's beam table measures in it (feeding fuse_points)."""

    def __init__(self, world=None, origin=None, map_size=None, resolution=None, local_radius=None, clamp_min_log=None,
                 clamp_max_log=None, min_occupancy_log=None, device="cuda:0"):
        import torch
        lib()
        self.torch = torch
        self.device = torch.device(device)
        d = dict(OCCMAP_DEFAULTS)
        for k, v in (("local_radius", local_radius), ("clamp_min_log", clamp_min_log), ("clamp_max_log", clamp_max_log),
                     ("min_occupancy_log", min_occupancy_log)):
            if v is not None:
                d[k] = v
        if world is not None:
            origin = world["origin"] if origin is None else origin
            map_size = world["map_size"] if map_size is None else map_size
            resolution = world["resolution"] if resolution is None else resolution
        self.origin = tuple(float(v) for v in origin); self.map_size = tuple(float(v) for v in map_size)
        self.resolution = float(resolution)
        self.local_radius = tuple(float(v) for v in d["local_radius"])
        self.clamp_min_log, self.clamp_max_log, self.min_occupancy_log = float(d["clamp_min_log"]), float(d["clamp_max_log"]), float(d["min_occupancy_log"])
        self.grid = tuple(int(np.ceil(m / self.resolution)) for m in self.map_size)  # occ_map.cpp:789
        self.world = world
        self.log_odds = torch.empty(self.grid, dtype=torch.float64, device=self.device)
        self.occ = torch.empty(self.grid, dtype=torch.uint8, device=self.device)
        m = self._map()
        self.ws_bytes = int(lib().frp_nmpc_occmap_workspace_bytes(ctypes.byref(m)))
        if self.ws_bytes == 0:
            raise ValueError("frp_nmpc_occmap refuses this map description (resolution, map_size, grid)")
        self.ws = torch.empty((self.ws_bytes // 4 + 1,), dtype=torch.int32, device=self.device)
        self.fuse_ws = None          # the fusion workspace: allocated by fuse_depth, grown when a larger frame needs it
        self.fuse_batch_ws = None    # the batched fusion's workspace: allocated by fuse_depth_batch, grown when a larger batch needs it
        self.fuse_points_ws = None   # the point scans' fusion workspace: allocated by fuse_points, grown when (S, P, max_ray_length) need more
        self._last_frame = None      # (depth, T_wc) of the previous filtered frame (last_depth_image, last_T_wc: occ_map.cpp:423-424)
        self._fusing_against = None  # the frame the latest filtered call reads on its stream: kept alive until the next call
        self._goal_table = None      # (table, n_groups, group_size) of goal_search_table() on the device: made by the first safety_check
        if world is not None and world.get("occ") is not None:
            o = torch.from_numpy(np.ascontiguousarray(world["occ"], dtype=np.uint8)).to(self.device)
            assert tuple(o.shape) == self.grid, (tuple(o.shape), self.grid)
            self.log_odds.fill_(self.clamp_min_log)
            self.log_odds.masked_fill_(o != 0, self.clamp_max_log)
            self.refresh()
        else:
            self.reset()

    def _map(self):
        return OccMap((ctypes.c_double * 3)(*self.origin), (ctypes.c_double * 3)(*self.map_size), self.resolution, (ctypes.c_int * 3)(*self.grid),
                      self.clamp_min_log, self.clamp_max_log, self.min_occupancy_log, (ctypes.c_double * 3)(*self.local_radius),
                      self.log_odds.data_ptr(), self.occ.data_ptr())

    def _call(self, name, *args, stream=None):
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        m = self._map()
        _check(getattr(lib(), name)(ctypes.byref(m), *args, ctypes.c_void_p(self.ws.data_ptr()), self.ws_bytes, ctypes.c_void_p(s.cuda_stream)), name)

    def _dev(self, a, dtype):
        return self._upload(a, dtype).to(self.device, dtype=dtype).contiguous()

    def astar_world(self):
        """The constants AstarPlanner reads: the world this map was built from, or the launch-file defaults around its geometry."""
        if self.world is not None:
            return self.world
        from . import workloads
        w = dict(workloads.ASTAR_DEFAULTS)
        w.update(origin=self.origin, map_size=self.map_size, resolution=self.resolution)
        return w

    def reset(self, stream=None):
        """Every voxel back to clamp_min_log (occ_map.cpp:831)."""
        self._call("frp_nmpc_occmap_reset", stream=stream)

    def refresh(self, stream=None):
        """occ and the bit plane from log_odds, after the caller wrote log_odds itself."""
        self._call("frp_nmpc_occmap_refresh", stream=stream)

    def clear_box(self, min_pos, max_pos, stream=None):
        """resetBuffer(min_pos, max_pos) (occ_map.cpp:15-36); host positions."""
        self._call("frp_nmpc_occmap_clear_box", (ctypes.c_double * 3)(*[float(v) for v in min_pos]), (ctypes.c_double * 3)(*[float(v) for v in max_pos]),
                   stream=stream)

    def insert_cloud(self, points, stream=None):
        """globalCloudCallback (occ_map.cpp:600-622): points [P,3] float32 (pcl::PointXYZ; anything else is converted to it first)."""
        pts = self._dev(points, self.torch.float32)
        assert pts.dim() == 2 and pts.shape[1] == 3
        self._call("frp_nmpc_occmap_insert_cloud", ctypes.c_void_p(pts.data_ptr()) if pts.shape[0] else None, int(pts.shape[0]), stream=stream)
        if stream is not None:
            pts.record_stream(stream)

    # ---- what the sensor routes below share: one argument path ----

    def _upload(self, a, dtype, what=""):
        """An array as a device tensor of `dtype` (uint16: the array `what` has to be uint16 already); a tensor as it is."""
        t = self.torch
        if t.is_tensor(a):
            return a
        if dtype == t.uint16:
            a = np.ascontiguousarray(a)
            if a.dtype != np.uint16:
                raise TypeError(f"{what} must be uint16 (the reference's depth_image.at<uint16_t>)")
            return t.from_numpy(a.view(np.int16)).to(self.device).view(t.uint16)
        return t.from_numpy(np.ascontiguousarray(a, dtype={t.float64: np.float64, t.float32: np.float32, t.int32: np.int32}[dtype])).to(self.device)

    def _tensor(self, a, dtype, shape, message, exc=TypeError, upload=False):
        """The checked device tensor behind an argument: an array is uploaded first (upload), a tensor is used in place.
        shape: a tuple, None for an extent that is free.  Anything but a contiguous tensor of that dtype and shape on the map's
        device: exc(message)."""
        t = self.torch
        if upload:
            a = self._upload(a, dtype)
        if (not t.is_tensor(a) or a.dtype != dtype or a.dim() != len(shape) or any(n is not None and n != m for n, m in zip(shape, a.shape))
                or a.device != self.log_odds.device or not a.is_contiguous()):
            raise exc(message)
        return a

    def _image(self, a, shape, what):
        """depth / last_depth of fuse_depth_batch (uploaded when an array)"""
        return self._tensor(self._upload(a, self.torch.uint16, what), self.torch.uint16, shape, f"{what} must be a contiguous [F, rows, cols] uint16 tensor on the map's device")

    def _fuse_params(self, f, method, params, keys=None):
        """The ray and filter parameters of the description f (`keys`; None: all): OCCMAP_FUSE_DEFAULTS under the caller's params."""
        keys = keys or tuple(OCCMAP_FUSE_DEFAULTS)
        unknown = set(params) - set(keys)
        if unknown:
            raise TypeError(f"{method}: unknown parameters {sorted(unknown)}")
        for k in keys:
            v = params.get(k, OCCMAP_FUSE_DEFAULTS[k])
            setattr(f, k, int(v) if k in ("depth_filter_margin", "skip_pixel", "max_rounds") else float(v))

    def _stream(self, stream):
        return stream if stream is not None else self.torch.cuda.current_stream(self.device)

    def _fuse(self, name, query, ws, f, refused, stream):
        """A fusion call: the workspace description f asks for (`query`; 0: ValueError(refused)), kept in self.<ws> and grown when a
        larger description needs it, then the call on the stream."""
        m = self._map()
        need = int(getattr(lib(), query)(ctypes.byref(m), ctypes.byref(f)))
        if need == 0:
            raise ValueError(refused)
        w = getattr(self, ws)
        if w is None or w.numel() < need:
            w = self.torch.empty((need,), dtype=self.torch.uint8, device=self.device)
            setattr(self, ws, w)
        _check(getattr(lib(), name)(ctypes.byref(m), ctypes.byref(f), ctypes.c_void_p(self.ws.data_ptr()), self.ws_bytes, ctypes.c_void_p(w.data_ptr()),
                                    int(w.numel()), ctypes.c_void_p(self._stream(stream).cuda_stream)), name)

    def _render(self, name, r, header, stream):
        """A render call on the stream; ValueError for a description the library refuses."""
        m = self._map()
        rc = getattr(lib(), name)(ctypes.byref(m), ctypes.byref(r), ctypes.c_void_p(self.ws.data_ptr()), self.ws_bytes,
                                  ctypes.c_void_p(self._stream(stream).cuda_stream))
        if rc == -1003:  # FRP_ERR_ARG
            raise ValueError(f"{name} refuses this description (see include/{header})")
        _check(rc, name)

    @staticmethod
    def _record(stream, *tensors):
        """The tensors a call on a stream of the caller's reads or writes stay allocated until it has run."""
        if stream is not None:
            for a in tensors:
                if a is not None:
                    a.record_stream(stream)

    @staticmethod
    def _ptr(a):
        return a.data_ptr() if a is not None else None

    def fuse_depth(self, depth, K, T_wc, *, shift_filter=False, status=None, stream=None, **params):
        """One camera frame into the map (OccMap::depthCallback's projectDepthImage + raycastProcess, occ_map.cpp:291-292):
        depth [rows, cols] uint16 (device tensor or array), K 3 x 3 intrinsics, T_wc 4 x 4 camera-to-world pose (host values).
        params: the keys of OCCMAP_FUSE_DEFAULTS.  log_odds, occ and the bit plane follow together -- no refresh().
        Returns the status tensor (int32 [2], device; nothing is synchronised): [0] relaxation rounds used, or minus max_rounds when
        the frame did not converge and the map was left untouched; [1] rays cast.
        shift_filter: the depth filter of :364-419 against the previous filtered frame, which the map keeps (with its pose)
        itself; the first filtered frame fuses nothing (has_first_depth_, :360-361) and returns [0, 0].
        status: a tensor to write into (a captured graph replays into the same buffer)."""
        t = self.torch
        f = OccMapFuse()
        self._fuse_params(f, "fuse_depth", params)
        depth = self._upload(depth, t.uint16, "depth")
        if depth.dtype != t.uint16 or depth.dim() != 2 or depth.device != self.log_odds.device:
            raise TypeError("depth must be a [rows, cols] uint16 tensor on the map's device")
        depth = depth.contiguous()
        T = np.ascontiguousarray(T_wc, dtype=np.float64).reshape(4, 4)
        Kh = np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        if status is None:
            status = t.zeros((2,), dtype=t.int32, device=self.device)
        assert status.dtype == t.int32 and status.numel() >= 2 and status.is_contiguous() and status.device == self.log_odds.device
        last = None
        if shift_filter:
            # The copy kept for the next frame is made on the stream of the call, behind whatever produced `depth` there (the caller
            # may reuse its tensor).  The previous frame stays referenced (_fusing_against) until the next call replaces it, so its
            # memory cannot go back to the allocator while this call's kernels, which read it, are still queued.
            with t.cuda.stream(self._stream(stream)):
                keep = depth.clone()
            last, self._last_frame = self._last_frame, (keep, T.copy())
            self._fusing_against = last
            if last is None:
                status.zero_()
                return status
            if tuple(last[0].shape) != tuple(depth.shape):
                raise ValueError("shift_filter: the frame size changed")
        f.rows, f.cols = int(depth.shape[0]), int(depth.shape[1])
        f.depth = depth.data_ptr()
        f.last_depth = last[0].data_ptr() if last is not None else None
        if last is not None:
            f.last_T_wc[:] = [float(v) for v in last[1].ravel()]
        f.K[:] = [float(v) for v in Kh.ravel()]
        f.T_wc[:] = [float(v) for v in T.ravel()]
        f.status = status.data_ptr()
        self._fuse("frp_nmpc_occmap_fuse_depth", "frp_nmpc_occmap_fuse_workspace_bytes", "fuse_ws", f,
                   "frp_nmpc_occmap_fuse_depth refuses this frame description (see include/frp_nmpc_occmap_fuse.h)", stream)
        self._record(stream, depth, last[0] if last is not None else None)
        return status

    def fuse_depth_batch(self, depth, K, T_wc, *, last_depth=None, last_T_wc=None, active=None, status=None, stream=None, **params):
        """F camera frames into the map in one call (include/frp_nmpc_occmap_fuse_batch.h): the map afterwards is, to the bit, what
        fuse_depth leaves after frames 0 ... F - 1 in that order; frames that are inactive, refused or not converged are skipped.
        depth [F, rows, cols] uint16, T_wc [F, 4, 4] float64; with the shift filter last_depth and last_T_wc of the same shapes (the
        caller keeps the previous frames; None: the unfiltered loops); active [F] int32 or None, 0 = the frame is not fused.  Each
        may be a numpy array, which is uploaded, or a device tensor, which is used IN PLACE: the poses are read by the kernels, so a
        captured call replays with whatever the caller has written into its tensors since.  K 3 x 3 (host) and params (the keys of
        OCCMAP_FUSE_DEFAULTS) are shared by the frames.
        Returns the status tensor (int32 [F, 2], device; nothing is synchronised): per frame [rounds used, rays cast] as fuse_depth
        reports them, [-max_rounds, rays] for a frame that did not converge (it contributes nothing, the others are fused),
        [0, 0] for an inactive frame, [OCCMAP_FUSE_REFUSED, 0] for a pose fuse_depth would refuse (non-finite, singular last rotation).
        status: a tensor to write into.  ValueError: a description the library refuses."""
        t = self.torch
        f = OccMapFuseBatch()
        self._fuse_params(f, "fuse_depth_batch", params)
        depth = self._image(depth, (None, None, None), "depth")
        F = int(depth.shape[0])
        T = self._tensor(T_wc, t.float64, (F, 4, 4), "T_wc must be a contiguous [F, 4, 4] float64 tensor on the map's device", upload=True)
        if (last_depth is None) != (last_T_wc is None):
            raise ValueError("fuse_depth_batch: last_depth and last_T_wc go together")
        last = lastT = None
        if last_depth is not None:
            last = self._image(last_depth, (None, None, None), "last_depth")
            lastT = self._tensor(last_T_wc, t.float64, (F, 4, 4), "last_T_wc must be a contiguous [F, 4, 4] float64 tensor on the map's device", upload=True)
            if tuple(last.shape) != tuple(depth.shape):
                raise ValueError("fuse_depth_batch: last_depth has another shape than depth")
        if active is not None:
            active = self._tensor(active, t.int32, (F,), "active must be a contiguous [F] int32 tensor on the map's device", upload=True)
        if status is None:
            status = t.zeros((F, 2), dtype=t.int32, device=self.device)
        self._tensor(status, t.int32, (F, 2), "status must be a contiguous [F, 2] int32 tensor on the map's device")
        Kh = np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
        f.frames, f.rows, f.cols = F, int(depth.shape[1]), int(depth.shape[2])
        f.depth, f.T_wc, f.status = depth.data_ptr(), T.data_ptr(), status.data_ptr()
        f.last_depth, f.last_T_wc, f.active = self._ptr(last), self._ptr(lastT), self._ptr(active)
        f.K[:] = [float(v) for v in Kh.ravel()]
        self._fuse("frp_nmpc_occmap_fuse_depth_batch", "frp_nmpc_occmap_fuse_batch_workspace_bytes", "fuse_batch_ws", f,
                   "frp_nmpc_occmap_fuse_depth_batch refuses this batch description (see include/frp_nmpc_occmap_fuse_batch.h)", stream)
        self._record(stream, depth, T, last, lastT, active)
        return status

    def fuse_points(self, points, origin, *, count=None, active=None, status=None, stream=None, **params):
        """S point scans into the map in one call (include/frp_nmpc_occmap_fuse_points.h): raycastProcess (occ_map.cpp:441-533) for
        a sensor that delivers a cloud in the world frame and the position it was taken from -- a LiDAR, a stereo rig.  The map
        afterwards is, to the bit, what fusing scans 0 ... S - 1 one after the other leaves; scans that are inactive, refused or not
        converged are skipped.  log_odds, occ and the bit plane follow together -- no refresh().
        points: a contiguous DEVICE tensor [S, P, 3], or [P, 3] for one scan, float64 or float32 (a float is widened exactly), used IN
        PLACE; a point with a NaN or infinite coordinate ("no return") is dropped and keeps its index.  origin [S, 3] or [3]
        float64, count [S] int32 or None (every scan holds P points; storage beyond count[s] is not read) and active [S] int32 or
        None may be numpy arrays, which are uploaded, or device tensors, which are used in place: the kernels read them, so a
        captured call replays with whatever the caller has written into its tensors since.  params: prob_hit_log, prob_miss_log,
        min_ray_length, max_ray_length, max_rounds of OCCMAP_FUSE_DEFAULTS, shared by the scans.
        Returns the status tensor (int32 [S, 2], device; nothing is synchronised) as fuse_depth_batch does: [rounds used, rays cast],
        [-max_rounds, rays] for a scan that did not converge, [0, 0] inactive, [OCCMAP_FUSE_REFUSED, 0] for a non-finite origin.
        status: a tensor to write into.  ValueError: arguments of another kind than described, or a description the library refuses."""
        t = self.torch
        f = OccMapFusePoints()
        self._fuse_params(f, "fuse_points", params, OCCMAP_FUSE_POINTS_PARAMS)
        if not t.is_tensor(points) or points.device != self.log_odds.device:
            raise ValueError("fuse_points: points must be a tensor on the map's device")
        if points.dtype not in (t.float64, t.float32):
            raise ValueError(f"fuse_points: points must be float64 or float32, not {points.dtype}")
        if points.dim() not in (2, 3) or points.shape[-1] != 3:
            raise ValueError(f"fuse_points: points must be [S, P, 3] or [P, 3], not {tuple(points.shape)}")
        if not points.is_contiguous():
            raise ValueError("fuse_points: points must be contiguous")
        S, P = (1, int(points.shape[0])) if points.dim() == 2 else (int(points.shape[0]), int(points.shape[1]))

        def per_scan(a, dtype, shape, what):
            a = self._upload(a, dtype)
            if S == 1 and a.dim() == len(shape) - 1 and a.is_contiguous():
                a = a.reshape(shape)  # one scan given without its leading dimension: a view, still the caller's storage
            return self._tensor(a, dtype, shape, f"fuse_points: {what} must be a contiguous {list(shape)} {dtype} tensor on the map's device "
                                "(or an array of that shape)", ValueError)

        origin = per_scan(origin, t.float64, (S, 3), "origin")
        if count is not None:
            count = per_scan(count, t.int32, (S,), "count")
        if active is not None:
            active = per_scan(active, t.int32, (S,), "active")
        if status is None:
            status = t.zeros((S, 2), dtype=t.int32, device=self.device)
        self._tensor(status, t.int32, (S, 2), "fuse_points: status must be a contiguous [S, 2] int32 tensor on the map's device", ValueError)
        f.scans, f.P = S, P
        f.points = points.data_ptr() if P > 0 and points.dtype == t.float64 else None
        f.points_f32 = points.data_ptr() if P > 0 and points.dtype == t.float32 else None
        f.count, f.active = self._ptr(count), self._ptr(active)
        f.origin, f.status = origin.data_ptr(), status.data_ptr()
        self._fuse("frp_nmpc_occmap_fuse_points_batch", "frp_nmpc_occmap_fuse_points_workspace_bytes", "fuse_points_ws", f,
                   f"frp_nmpc_occmap_fuse_points_batch refuses this description: {S} scans of {P} points (see include/frp_nmpc_occmap_fuse_points.h)", stream)
        self._record(stream, points, origin, count, active)
        return status

    def render_depth(self, T_wc, K, rows, cols, *, max_range, depth_scale=1000.0, active=None, out=None, voxel=None, status=None, stream=None):
        """What F cameras at the poses T_wc see of THIS map (include/frp_nmpc_occmap_render.h): the depth images
        [F, rows, cols] uint16 that fuse_depth_batch takes, one ray per pixel walked through the bit plane.  T_wc [F, 4, 4] float64
        and active [F] int32 (or None) may be numpy arrays, which are uploaded, or device tensors, which are used IN PLACE: the
        kernels read them, so a captured call replays with whatever the caller has written since.  K 3 x 3 (host), max_range in
        metres along the ray.  out: the depth tensor to write into (an inactive frame's image keeps what it holds; a fresh one is
        zero); voxel: an int32 tensor [F, rows, cols] for the linear voxel index of every return (-1: none), or None; status: an
        int32 tensor [F, 2] for {1, returns} / {0, 0} inactive / {OCCMAP_FUSE_REFUSED, 0} a non-finite pose.  Returns the depth
        tensor; nothing is synchronised.  ValueError: a description the library refuses."""
        t = self.torch
        T_wc = self._tensor(T_wc, t.float64, (None, 4, 4), "T_wc must be a contiguous [F, 4, 4] float64 tensor on the map's device", upload=True)
        F, rows, cols = int(T_wc.shape[0]), int(rows), int(cols)
        if active is not None:
            active = self._tensor(active, t.int32, (F,), "active must be a contiguous [F] int32 tensor on the map's device", upload=True)
        if F < 1 or rows < 1 or cols < 1:
            raise ValueError("render_depth: at least one frame, one row and one column")
        if out is None:
            out = t.zeros((F, rows, cols), dtype=t.int16, device=self.device).view(t.uint16)
        self._tensor(out, t.uint16, (F, rows, cols), "out must be a contiguous [F, rows, cols] uint16 tensor on the map's device")
        if voxel is not None:
            self._tensor(voxel, t.int32, (F, rows, cols), "voxel must be a contiguous [F, rows, cols] int32 tensor on the map's device")
        if status is None:
            status = t.zeros((F, 2), dtype=t.int32, device=self.device)
        self._tensor(status, t.int32, (F, 2), "status must be a contiguous [F, 2] int32 tensor on the map's device")
        r = OccMapRender()
        r.frames, r.rows, r.cols = F, rows, cols
        r.T_wc, r.active = T_wc.data_ptr(), self._ptr(active)
        r.K[:] = [float(v) for v in np.ascontiguousarray(K, dtype=np.float64).reshape(9)]
        r.depth_scale, r.max_range = float(depth_scale), float(max_range)
        r.depth, r.voxel, r.status = out.data_ptr(), self._ptr(voxel), status.data_ptr()
        self._render("frp_nmpc_occmap_render_depth", r, "frp_nmpc_occmap_render.h", stream)
        self._record(stream, T_wc, active, out, voxel, status)
        return out

    def render_scan(self, T_ws, beams, *, max_range, min_range=0.0, far_range=0.0, dtype=None, active=None, points=None, points_f32=None,
                    origin=None, count=None, range=None, voxel=None, status=None, stream=None):
        """What S range sensors at the poses T_ws measure of THIS map along a table of P beam directions
        (include/frp_nmpc_occmap_render_scan.h): the point scans [S, P, 3] in the world frame that fuse_points takes, in beam order,
        with their origins [S, 3] and counts [S] written on the device -- camera_poses -> render_scan -> fuse_points needs no host.
        T_ws [S, 4, 4] float64 sensor-to-world, beams [P, 3] float64 in the sensor frame (any length; lidar_beams() makes a spinning
        LiDAR's) and active [S] int32 (or None) may be numpy arrays, which are uploaded, or device tensors, which are used IN PLACE: the
        kernels read them, so a captured call replays with whatever the caller has written since.  max_range, min_range: metres along
        the beam.  A beam without a return gives a NaN point (fuse_points drops it), or with far_range >= max_range the point at
        far_range along the beam (fused with max_ray_length < far_range: a miss that carves free space).
        dtype: torch.float64 (the default) or torch.float32, the type of the points returned.  The output tensors are used if given,
        so that a captured call replays into them: points [S, P, 3] (its dtype then decides), points_f32 [S, P, 3] float32 written
        as well as float64 points (each float is the double rounded once), origin [S, 3] float64, count [S] int32, range [S, P]
        float64 (metres along the beam of the return, 0: none), voxel [S, P] int32 (linear voxel index of the return, -1: none),
        status [S, 2] int32 ({1, returns} / {0, 0} inactive, nothing of the scan written but count 0 / {OCCMAP_FUSE_REFUSED, 0} a
        non-finite pose, its points NaN).  Returns (points, origin, count, status); nothing is synchronised.  ValueError: a
        description the library refuses."""
        t = self.torch

        def given(a, dt, shape, what, free=False, upload=False):  # free: the shape was checked by the caller, its message says none
            return self._tensor(a, dt, shape, f"render_scan: {what} must be a contiguous {'' if free else list(shape)} {dt} tensor on the map's device",
                                upload=upload)

        T_ws = self._upload(T_ws, t.float64)
        if T_ws.dim() != 3 or tuple(T_ws.shape[1:]) != (4, 4):
            raise TypeError("render_scan: T_ws must be [S, 4, 4]")
        T_ws = given(T_ws, t.float64, (None, 4, 4), "T_ws", free=True)
        if not t.is_tensor(beams):
            beams = t.from_numpy(np.array(beams, dtype=np.float64, order="C")).to(self.device)  # (a copy: a table kept read-only uploads too)
        if beams.dim() != 2 or beams.shape[1] != 3:
            raise TypeError("render_scan: beams must be [P, 3]")
        beams = given(beams, t.float64, (None, 3), "beams", free=True)
        S, P = int(T_ws.shape[0]), int(beams.shape[0])
        if S < 1 or P < 1:
            raise ValueError("render_scan: at least one scan and one beam")
        if active is not None:
            active = given(active, t.int32, (S,), "active", upload=True)
        if points is None:
            dtype = t.float64 if dtype is None else dtype
            if dtype not in (t.float64, t.float32):
                raise TypeError(f"render_scan: dtype must be float64 or float32, not {dtype}")
            points = t.full((S, P, 3), float("nan"), dtype=dtype, device=self.device)
        elif not t.is_tensor(points) or points.dtype not in (t.float64, t.float32) or (dtype is not None and points.dtype != dtype):
            raise TypeError("render_scan: points must be a float64 or float32 tensor of the dtype asked for")
        points = given(points, points.dtype, (S, P, 3), "points")
        if points_f32 is not None:
            if points.dtype != t.float64:
                raise TypeError("render_scan: points_f32 goes with float64 points")
            points_f32 = given(points_f32, t.float32, (S, P, 3), "points_f32")
        origin = t.zeros((S, 3), dtype=t.float64, device=self.device) if origin is None else given(origin, t.float64, (S, 3), "origin")
        count = t.zeros((S,), dtype=t.int32, device=self.device) if count is None else given(count, t.int32, (S,), "count")
        status = t.zeros((S, 2), dtype=t.int32, device=self.device) if status is None else given(status, t.int32, (S, 2), "status")
        if range is not None:
            range = given(range, t.float64, (S, P), "range")
        if voxel is not None:
            voxel = given(voxel, t.int32, (S, P), "voxel")
        r = OccMapRenderScan()
        r.scans, r.P = S, P
        r.beams, r.T_ws, r.active = beams.data_ptr(), T_ws.data_ptr(), self._ptr(active)
        r.min_range, r.max_range, r.far_range = float(min_range), float(max_range), float(far_range)
        r.points = points.data_ptr() if points.dtype == t.float64 else None
        r.points_f32 = points.data_ptr() if points.dtype == t.float32 else self._ptr(points_f32)
        r.origin, r.count, r.status = origin.data_ptr(), count.data_ptr(), status.data_ptr()
        r.range, r.voxel = self._ptr(range), self._ptr(voxel)
        self._render("frp_nmpc_occmap_render_scan_batch", r, "frp_nmpc_occmap_render_scan.h", stream)
        self._record(stream, T_ws, beams, active, points, points_f32, origin, count, range, voxel, status)
        return points, origin, count, status

    def camera_poses(self, state, T_bc, out=None, stream=None):
        """T_wc [B, 4, 4] = T_wb(state) T_bc for planner states [B, 9] (position, velocity, Euler angles; device tensor, used in
        place, or array) and the body-to-camera transform T_bc 4 x 4 (host): what render_depth and fuse_depth_batch take as poses,
        computed where the states are (frp_nmpc_occmap_camera_poses).  out: the tensor to write into."""
        t = self.torch
        st = self._tensor(state, t.float64, (None, 9), "state must be a contiguous [B, 9] float64 tensor on the map's device", upload=True)
        B = int(st.shape[0])
        if out is None:
            out = t.zeros((B, 4, 4), dtype=t.float64, device=self.device)
        self._tensor(out, t.float64, (B, 4, 4), "out must be a contiguous [B, 4, 4] float64 tensor on the map's device")
        Tb = (ctypes.c_double * 16)(*[float(v) for v in np.ascontiguousarray(T_bc, dtype=np.float64).reshape(16)])
        _check(lib().frp_nmpc_occmap_camera_poses(B, ctypes.c_void_p(st.data_ptr()) if B else None, Tb, ctypes.c_void_p(out.data_ptr()) if B else None,
                                                  ctypes.c_void_p(self._stream(stream).cuda_stream)), "frp_nmpc_occmap_camera_poses")
        self._record(stream, st, out)
        return out


    def local_view(self, centres, P, out=None, stream=None):
        """local_box + localOccVisCallback's cloud (occ_map.cpp:177-215) of every planner: centres [B,3] f64 (device tensor or
        array), P points stored per planner.  centres = None: the whole map as one cloud (globalOccVisCallback, :150-175), B = 1.
        out: a LocalView of the same shapes to write into (a captured graph replays into the same buffers).  Nothing is
        synchronised: cloud_count (negative = overflow, LocalView.overflowed()) is a device tensor.
        P = 0 stores no cloud: local_box alone (cloud_count = minus each planner's count).  That is the per-tick call of the
        shared-cloud route -- shared_view() once per map change, then per tick local_view(centres, 0) and cut(view.local_box)."""
        t = self.torch
        c = None if centres is None else self._dev(centres, t.float64)
        B = 1 if c is None else int(c.shape[0])
        assert c is None or tuple(c.shape) == (B, 3)
        if out is None:
            out = LocalView(t.zeros((B, 6), dtype=t.int32, device=self.device), t.zeros((B, P, 3), dtype=t.float64, device=self.device),
                            t.zeros((B,), dtype=t.int32, device=self.device))
        assert tuple(out.cloud.shape) == (B, P, 3) and out.cloud.is_contiguous() and tuple(out.local_box.shape) == (B, 6)
        v = OccMapView(B, c.data_ptr() if c is not None else None, P, out.local_box.data_ptr(), out.cloud.data_ptr() if P else None,
                       out.cloud_count.data_ptr())
        self._call("frp_nmpc_occmap_local_view", ctypes.byref(v), stream=stream)
        if stream is not None and c is not None and c is not centres:
            c.record_stream(stream)
        return out

    def cut(self, local_box):
        """The visibility cut of frp_nmpc_corridor_batch_cut for local_box [B,6] int32 (device tensor, LocalView.local_box): what
        corridor_batch_device / DeviceFleet.corridor / full_tick take as `cut` beside the shared cloud of shared_view().  Planner b
        then sees the points with origin + min_id * resolution <= q < origin + max_id * resolution per axis -- its local cloud."""
        t = self.torch
        assert t.is_tensor(local_box) and local_box.dtype == t.int32 and local_box.dim() == 2 and local_box.shape[1] == 6 and local_box.is_contiguous()
        assert local_box.device == self.log_odds.device
        c = CorridorCut(local_box.data_ptr(), (ctypes.c_double * 3)(*self.origin), self.resolution)
        c._box = local_box
        return c

    def shared_view(self, cell=0.5, stream=None):
        """The whole-map cloud (local_view(None, .), every occupied voxel's centre in x, y, z order) trimmed to its count, and a
        CloudGrid over it: (cloud [n,3] f64, grid).  The grid is laid over the map itself -- origin = the map's, dims =
        ceil(map_size / cell) -- so nothing is read back to find its bounds.  ONE synchronisation, to read the count: call it
        when the map changes (insert_cloud / clear_box / refresh), not per tick.  A shared cloud holds at most
        FRP_CORRIDOR_MAX_POINTS points; a map with more occupied voxels raises ValueError (use per-planner clouds)."""
        t = self.torch
        s = stream if stream is not None else t.cuda.current_stream(self.device)
        v = self.local_view(None, CORRIDOR_MAX_POINTS, stream=stream)
        with t.cuda.stream(s):
            n = int(v.cloud_count[0].item())   # the one synchronisation
        if n < 0:
            raise ValueError(f"the map holds {-n} occupied voxels, a shared cloud at most FRP_CORRIDOR_MAX_POINTS = {CORRIDOR_MAX_POINTS}: "
                             "use per-planner clouds (local_view(centres, P))")
        with t.cuda.stream(s):
            cloud = v.cloud[0, :n].clone()
        dims = tuple(max(1, int(np.ceil(m / float(cell)))) for m in self.map_size)
        return cloud, CloudGrid(cloud, cell, origin=self.origin, dims=dims, stream=stream)

    def shared_view_device(self, cap=CORRIDOR_MAX_POINTS, cell=0.5, planners=4096):
        """A SharedView of this map: the cloud and grid of shared_view() in persistent buffers of `cap` points, rebuilt by
        SharedView.update() with nothing on the host.  The per-tick form of the shared-cloud route when the map changes every tick.
        cap may exceed CORRIDOR_MAX_POINTS, up to CORRIDOR_LARGE_MAX_POINTS: a LARGE view, for at most `planners` planners per
        corridor call (see SharedView)."""
        return SharedView(self, cap, cell, planners)

    def query(self, pos, local_box=None, planner=None, stream=None):
        """getVoxelState (occ_map.cpp:95-106) of pos [Q,3]: int32 [Q] device tensor, -1 outside the map, 0 free or outside the local
        map, 1 occupied.  local_box [.,6] of a local view with planner [Q] = its row per query (None: row 0)."""
        t = self.torch
        q = self._dev(pos, t.float64)
        Q = int(q.shape[0])
        st = t.zeros((Q,), dtype=t.int32, device=self.device)
        pl = None if planner is None else self._dev(planner, t.int32)
        lb = None if local_box is None else self._dev(local_box, t.int32)
        self._call("frp_nmpc_occmap_query", Q, ctypes.c_void_p(q.data_ptr()) if Q else None, pl.data_ptr() if pl is not None else None,
                   lb.data_ptr() if lb is not None else None, ctypes.c_void_p(st.data_ptr()), stream=stream)
        if stream is not None:
            for a in (q, pl, lb):
                if a is not None:
                    a.record_stream(stream)
        return st


    def check_surround(self, pos, inflate_ratio, local_box=None, planner=None, body=OCCMAP_BODY, stream=None):
        """checkPosSurround(pos, inflate_ratio) (occ_map.cpp:625-643) of pos [Q,3]: int32 [Q] device tensor, 1 = free (every probe of
        the inflated body is 0), 0 = collision (a probe is occupied or outside the map).  local_box / planner as in query()."""
        t = self.torch
        q = self._dev(pos, t.float64)
        Q = int(q.shape[0])
        assert tuple(q.shape) == (Q, 3)
        out = t.zeros((Q,), dtype=t.int32, device=self.device)
        pl = None if planner is None else self._dev(planner, t.int32)
        lb = None if local_box is None else self._dev(local_box, t.int32)
        bd = OccMapBody(float(body[0]), float(body[1]))
        self._call("frp_nmpc_occmap_check_surround", ctypes.byref(bd), float(inflate_ratio), Q, q.data_ptr() if Q else None,
                   pl.data_ptr() if pl is not None else None, lb.data_ptr() if lb is not None else None, out.data_ptr(), stream=stream)
        if stream is not None:
            for a in (q, pl, lb):
                if a is not None:
                    a.record_stream(stream)
        return out

    def safety_check(self, end_pt, kino_path, kino_size, have_target=None, have_traj=None, local_box=None, stride=5, stream=None,
                     body=OCCMAP_BODY, out=None):
        """One tick of the safety timer (NMPCManage::checkReplanCallback, nmpc_manage.cpp:285-341) for B planners, on the live bit
        plane: the goal test and search (frp_nmpc_occmap_check_goals; end_pt [B,3] f64 device tensor, UPDATED IN PLACE where the
        search moves a blocked goal) and the path walk (frp_nmpc_occmap_check_paths; kino_path [B,K,3] f64 / kino_size [B] int32 as
        AstarPlanner keeps them, every stride-th sample).  have_target / have_traj: int32 [B] or None (all set); local_box [B,6] of
        a local view or None.  Returns a SafetyCheck; nothing is synchronised.  out: a SafetyCheck to write into (a captured
        graph replays into the same buffers).  The FSM transitions stay with the caller."""
        t = self.torch
        dev = self.log_odds.device
        for a, dt in ((end_pt, t.float64), (kino_path, t.float64), (kino_size, t.int32)):
            assert t.is_tensor(a) and a.dtype == dt and a.is_contiguous() and a.device == dev
        B, K = int(kino_path.shape[0]), int(kino_path.shape[1])
        assert tuple(kino_path.shape) == (B, K, 3) and tuple(end_pt.shape) == (B, 3) and tuple(kino_size.shape) == (B,)
        opt = [None if a is None else self._dev(a, t.int32) for a in (have_target, have_traj, local_box)]
        ht, hj, lb = opt
        assert lb is None or tuple(lb.shape) == (B, 6)
        if out is None:
            z = lambda: t.zeros((B,), dtype=t.int32, device=self.device)
            out = SafetyCheck(z(), z(), z(), z())
        if self._goal_table is None:
            tab, ng, gs = goal_search_table()
            self._goal_table = (t.from_numpy(tab).to(self.device), ng, gs)
        tab, ng, gs = self._goal_table
        bd = OccMapBody(float(body[0]), float(body[1]))
        ptr = lambda a: a.data_ptr() if a is not None else None
        s = stream if stream is not None else t.cuda.current_stream(self.device)
        self._call("frp_nmpc_occmap_check_goals", ctypes.byref(bd), SAFETY_INFLATE_CHECK, SAFETY_INFLATE_SEARCH, B, end_pt.data_ptr(), ptr(ht), ptr(lb),
                   ng, gs, tab.data_ptr(), out.goal_blocked.data_ptr(), out.goal_hits.data_ptr(), stream=stream)
        self._call("frp_nmpc_occmap_check_paths", ctypes.byref(bd), SAFETY_INFLATE_CHECK, B, K, int(stride), kino_path.data_ptr(), kino_size.data_ptr(),
                   ptr(hj), ptr(lb), out.first_hit.data_ptr(), stream=stream)
        with t.cuda.stream(s):
            t.bitwise_or(out.goal_blocked, (out.first_hit >= 0).to(t.int32), out=out.replan)
        if stream is not None:
            for a in (end_pt, kino_path, kino_size, tab, out.goal_blocked, out.goal_hits, out.first_hit, out.replan) + tuple(opt):
                if a is not None:
                    a.record_stream(stream)
        return out

    def distance_field(self, R=OCCMAP_DIST_DEFAULT_R, border=True):
        """A DistanceField of this map (include/frp_nmpc_occmap_distance.h), built once from the bit plane as it is now.  R: the radius in
        voxels, 1 ... OCCMAP_DIST_MAX_R; the default of 20 is 2 m at the reference's 0.1 m resolution -- CHOSEN, not derived.  border:
        voxels outside the map count as occupied (checkPosSurround's reading)."""
        return DistanceField(self, R, border)


class DistanceField:
    """The truncated distance field of an OccupancyMap, on the device (include/frp_nmpc_occmap_distance.h): field [gx, gy, gz] uint16, the
    exact integer squared distance in voxels from each voxel to the nearest occupied one where that is <= R * R, else OCCMAP_DIST_FAR;
    with border=True the voxels outside the map count as occupied.  It has no reference counterpart (the reference's map keeps no
    distance).  Owns `field` and the scratch of the three passes; update() rebuilds from the map's CURRENT bit plane -- the field does
    not follow the map by itself.  clearance(pos) is resolution * sqrt(field) at the positions' voxels: a distance between voxel
    CENTRES (the header says what that bounds), +inf beyond R, 0.0 inside an occupied voxel, outside the map or for a position that is
    not finite."""

    def __init__(self, occmap, R=OCCMAP_DIST_DEFAULT_R, border=True):
        t = occmap.torch
        self.torch, self.occmap, self.R, self.border = t, occmap, int(R), bool(border)
        if not 1 <= self.R <= OCCMAP_DIST_MAX_R:
            raise ValueError(f"DistanceField: R is 1 ... {OCCMAP_DIST_MAX_R} voxels")
        m = occmap._map()
        self.scratch_bytes = int(lib().frp_nmpc_occmap_distance_scratch_bytes(ctypes.byref(m), self.R))
        if self.scratch_bytes == 0:
            raise ValueError("frp_nmpc_occmap_distance refuses this map description")
        self.field = t.empty(occmap.grid, dtype=t.uint16, device=occmap.device)
        self.scratch = t.empty((self.scratch_bytes,), dtype=t.uint8, device=occmap.device)
        self.update()

    def _stream(self, stream):
        return ctypes.c_void_p((stream if stream is not None else self.torch.cuda.current_stream(self.field.device)).cuda_stream)

    def update(self, stream=None):
        """frp_nmpc_occmap_distance_update: field <- the definition on the map's bit plane as the stream finds it (three launches)."""
        o = self.occmap
        m = o._map()
        _check(lib().frp_nmpc_occmap_distance_update(ctypes.byref(m), self.R, int(self.border), ctypes.c_void_p(self.field.data_ptr()),
                                                     ctypes.c_void_p(self.scratch.data_ptr()), self.scratch_bytes, ctypes.c_void_p(o.ws.data_ptr()), o.ws_bytes,
                                                     self._stream(stream)), "frp_nmpc_occmap_distance_update")

    def clearance(self, pos, d2=False, stream=None):
        """frp_nmpc_occmap_clearance of pos [Q,3] (float64 device tensor, or an array that is uploaded): float64 [Q] device tensor; with
        d2=True (clear, d2) with d2 int32 [Q]: the field's integer, OCCMAP_DIST_FAR included, -1 outside the map."""
        t, o = self.torch, self.occmap
        q = o._dev(pos, t.float64)
        Q = int(q.shape[0])
        assert tuple(q.shape) == (Q, 3)
        clear = t.zeros((Q,), dtype=t.float64, device=o.device)
        sq = t.zeros((Q,), dtype=t.int32, device=o.device) if d2 else None
        m = o._map()
        _check(lib().frp_nmpc_occmap_clearance(ctypes.byref(m), ctypes.c_void_p(self.field.data_ptr()), self.R, Q, q.data_ptr() if Q else None,
                                               clear.data_ptr() if Q else None, sq.data_ptr() if d2 and Q else None, self._stream(stream)),
               "frp_nmpc_occmap_clearance")
        o._record(stream, q, clear, sq)
        return (clear, sq) if d2 else clear


class FlightClearance:
    """How close every vehicle of a Vehicle came to an obstacle, on the device (frp_nmpc_occmap_clearance_trace): min_clear [B] float64
    (+inf until something nearer than the field's radius was seen), hits [B] int32 (samples with clearance 0.0: inside an occupied
    voxel, outside the map or not finite) and samples [B] int32.  It hooks into nothing: the caller launches update() after
    Vehicle.step / FleetFSM.period(..., vehicle=...), inside the same captured graph if they wish.  The positions are the TRUE plant
    states of the vehicle's trace, and the numbers are distances between voxel centres (include/frp_nmpc_occmap_distance.h); the
    body's radius is the caller's to subtract.  Tracking error and the rest of a flight record are not kept."""

    def __init__(self, vehicle, field):
        t = vehicle.torch
        dev = vehicle.x.device
        if field.field.device != dev:
            raise ValueError("FlightClearance: the vehicle and the distance field are on different devices")
        self.torch, self.vehicle, self.field, self.B = t, vehicle, field, vehicle.B
        self.min_clear = t.full((self.B,), float("inf"), dtype=t.float64, device=dev)
        self.hits, self.samples = t.zeros((self.B,), dtype=t.int32, device=dev), t.zeros((self.B,), dtype=t.int32, device=dev)

    def update(self, trace=None, active=None, stream=None):
        """The S samples of trace [B,S,stride >= 3] (float64; None: vehicle.trace, or else the attached estimator's meas -- the fallback
        Vehicle.step writes to) taken in order into min_clear, hits and samples; active [B] int32 or None: where it is 0 nothing of
        that vehicle changes."""
        t, v = self.torch, self.vehicle
        if trace is None:
            trace = v.trace if v.trace is not None else v.estimator.meas if v.estimator is not None else None
            if trace is None:
                raise ValueError("FlightClearance.update: this Vehicle keeps no trace (trace=True) and has no ForceEstimator attached; pass trace=")
        assert t.is_tensor(trace) and trace.dim() == 3, "trace is a [B, S, stride] tensor"
        S, stride = int(trace.shape[1]), int(trace.shape[2])
        if S < 1 or stride < 3:
            raise ValueError("FlightClearance.update: trace is [B, S >= 1, stride >= 3]")
        a = v._arg(active, t.int32, (self.B,)) if active is not None else None
        f = self.field
        m = f.occmap._map()
        _check(lib().frp_nmpc_occmap_clearance_trace(ctypes.byref(m), ctypes.c_void_p(f.field.data_ptr()), f.R, self.B, S, stride,
                                                     v._arg(trace, t.float64, (self.B, S, stride)), a, ctypes.c_void_p(self.min_clear.data_ptr()),
                                                     ctypes.c_void_p(self.hits.data_ptr()), ctypes.c_void_p(self.samples.data_ptr()), v._stream(stream)),
               "frp_nmpc_occmap_clearance_trace")

    def reset(self, mask=None, stream=None):
        """frp_nmpc_occmap_clearance_reset: where mask [B] int32 != 0 (None: everywhere) min_clear <- +inf, hits <- 0, samples <- 0."""
        t, v = self.torch, self.vehicle
        m = v._arg(mask, t.int32, (self.B,)) if mask is not None else None
        _check(lib().frp_nmpc_occmap_clearance_reset(self.B, m, ctypes.c_void_p(self.min_clear.data_ptr()), ctypes.c_void_p(self.hits.data_ptr()),
                                                     ctypes.c_void_p(self.samples.data_ptr()), v._stream(stream)), "frp_nmpc_occmap_clearance_reset")


class AstarPlanner:
    """SURVEY 8f row f-4 (second half): the kinodynamic A* of NMPCSolver::getKinoPath for B planners on the device
    (frp_nmpc_astar_batch).  `world`: occupancy grid occ[x][y][z] (uint8) + the map / search constants of the reference's launch
    files (forces_resilient_planner_amd.workloads.astar_world), or an OccupancyMap: the planner then searches the map's own occ
    buffer (no copy: later inserts are seen) -- pass the local_box of the map's local view to plan().  Outputs stay in HBM: kino_path [B,K,3] / kino_size [B] are what
    DeviceFleet.references() takes as a per-planner path."""

    def __init__(self, world, B, K=1024, Ts=0.05, device="cuda:0", want_path_nodes=False, allocate_num=None):
        import torch
        lib()
        self.torch = torch
        self.B, self.K, self.Ts = B, K, Ts
        self.device = torch.device(device)
        self.map = world if isinstance(world, OccupancyMap) else None
        if self.map is not None:
            assert self.map.device == self.device
            world = self.map.astar_world()
        self.world = world
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.occ = self.map.occ if self.map is not None else torch.from_numpy(np.ascontiguousarray(world["occ"], dtype=np.uint8)).to(self.device)
        self.kino_path = torch.zeros((B, K, 3), **f64)
        self.kino_size = torch.zeros((B,), **i32)
        self.status = torch.zeros((B,), **i32)
        self.stats = torch.zeros((B, 4), **i32)
        self.path_nodes = torch.zeros((B, ASTAR_MAX_PATH, 11), **f64) if want_path_nodes else None
        self.allocate_num = int(allocate_num or world["allocate_num"])
        self._q = [torch.zeros((B, 3), **f64) for _ in range(6)]
        self._retry = None  # (retry_pt, retry_vel): the start of the repeated search, when it differs (upload(..., retry=...))
        a = self._args()
        self.ws_bytes = int(lib().frp_nmpc_astar_workspace_bytes(ctypes.byref(a)))
        self.ws = torch.empty((self.ws_bytes // 8 + 1,), **f64)

    def _args(self, init=True, local_box=None, active=None, end_pt=None, end_vel=None, external_acc=None):
        w = self.world
        a = Astar()
        a.B = self.B; a.occ = self.occ.data_ptr(); a.grid[:] = tuple(self.occ.shape); a.origin[:] = w["origin"]; a.map_size[:] = w["map_size"]
        a.resolution = w["resolution"]; a.local_box = local_box.data_ptr() if local_box is not None else None
        a.ego_r = w["ego_r"]; a.ego_h = w["ego_h"]
        for k in ("max_tau", "init_max_tau", "max_vel", "max_acc", "w_time", "horizon", "lambda_heu", "tie_breaker", "check_num"):
            setattr(a, k, w[k])
        a.allocate_num = self.allocate_num
        a.start_pt, a.start_vel, a.start_acc, a.end_pt, a.end_vel, a.external_acc = (t.data_ptr() for t in self._q)
        for name, over in (("end_pt", end_pt), ("end_vel", end_vel), ("external_acc", external_acc)):  # a caller's own [B,3] in place of the uploaded one
            if over is not None:
                assert over.dtype == self.torch.float64 and tuple(over.shape) == (self.B, 3) and over.is_contiguous() and over.device == self.device
                setattr(a, name, over.data_ptr())
        a.active = active.data_ptr() if active is not None else None
        a.init_search = 1 if init else 0
        a.Ts = self.Ts; a.K = self.K
        a.kino_path = self.kino_path.data_ptr(); a.kino_size = self.kino_size.data_ptr(); a.status = self.status.data_ptr()
        a.stats = self.stats.data_ptr(); a.path_nodes = self.path_nodes.data_ptr() if self.path_nodes is not None else None
        a.retry_pt = self._retry[0].data_ptr() if self._retry is not None else None
        a.retry_vel = self._retry[1].data_ptr() if self._retry is not None else None
        return a

    def upload(self, start_pt, start_v, start_a, end_pt, end_v, f_ext, retry=None):
        """retry = (pt [B,3], vel [B,3]): the start of the repeated search (getKinoPath retries from the odometry state,
        nmpc_solver.cpp:190-193); None: the same start."""
        t = self.torch
        cp = lambda dst, src: dst.copy_(src if t.is_tensor(src) else t.from_numpy(np.ascontiguousarray(src, dtype=np.float64)))
        for dst, src in zip(self._q, (start_pt, start_v, start_a, end_pt, end_v, f_ext)):
            cp(dst, src)
        if retry is None:
            self._retry = None
        else:
            if self._retry is None:
                self._retry = [t.zeros_like(self._q[0]), t.zeros_like(self._q[0])]
            cp(self._retry[0], retry[0]); cp(self._retry[1], retry[1])

    def plan(self, init=True, local_box=None, stream=None, active=None, end_pt=None, end_vel=None, external_acc=None):
        """Asynchronous on `stream` (or torch's current stream): every planner's search + retry + getKinoTraj.
        active: int32 [B] device tensor -- only planners with a non-zero entry search (the others keep their path);
        a planner whose search ends in NO_PATH keeps its previous path as well.
        end_pt / end_vel / external_acc: [B,3] f64 device tensors read in place of the uploaded ones (FleetFSM hands over its own
        end_pt and external_acc: no copy)."""
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        a = self._args(init, local_box, active, end_pt, end_vel, external_acc)
        _check(lib().frp_nmpc_astar_batch(ctypes.byref(a), ctypes.c_void_p(self.ws.data_ptr()), self.ws_bytes, ctypes.c_void_p(s.cuda_stream)),
               "frp_nmpc_astar_batch")


class CloudGrid:
    """Uniform grid over a shared obstacle cloud (frp_nmpc_cloud_grid_build): built once per cloud, handed to
    corridor_batch_device / DeviceFleet.corridor so that a decomposition reads only the cells its local box touches."""

    def __init__(self, cloud, cell=0.5, origin=None, dims=None, stream=None):
        import torch
        assert cloud.dim() == 2 and cloud.shape[1] == 3 and cloud.is_contiguous() and cloud.dtype == torch.float64
        P = cloud.shape[0]
        if origin is None or dims is None:  # bounds of the cloud itself (host round trip; a map normally knows its bounds)
            finite = cloud[torch.isfinite(cloud).all(dim=1)]
            lo = finite.min(dim=0).values.cpu().numpy() if finite.numel() else np.zeros(3)
            hi = finite.max(dim=0).values.cpu().numpy() if finite.numel() else np.ones(3)
            origin = lo - 1e-9
            dims = np.maximum(1, np.ceil((hi - origin) / cell + 1e-9)).astype(int)
        self.origin = tuple(float(v) for v in origin); self.dims = tuple(int(v) for v in dims); self.cell = float(cell)
        cells = self.dims[0] * self.dims[1] * self.dims[2]
        dev = cloud.device
        self.points = torch.empty((max(P, 1), 3), dtype=torch.float64, device=dev)
        self.index = torch.empty((max(P, 1),), dtype=torch.int32, device=dev)
        self.start = torch.empty((cells + 1,), dtype=torch.int32, device=dev)
        scratch = torch.empty((cells,), dtype=torch.int32, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        _check(lib().frp_nmpc_cloud_grid_build(ctypes.c_void_p(cloud.data_ptr()) if P else None, P, (ctypes.c_double * 3)(*self.origin),
                                               self.cell, (ctypes.c_int * 3)(*self.dims), ctypes.c_void_p(self.points.data_ptr()),
                                               ctypes.c_void_p(self.index.data_ptr()), ctypes.c_void_p(self.start.data_ptr()),
                                               ctypes.c_void_p(scratch.data_ptr()), ctypes.c_void_p(s.cuda_stream)), "frp_nmpc_cloud_grid_build")
        s.synchronize()  # scratch may be freed


class SharedViewGrid:
    """The grid of a SharedView: CloudGrid's attributes (origin, dims, cell, points, index, start) over the view's persistent buffers.
    It describes view.cloud[:view.count] as of the last update()."""

    def __init__(self, origin, dims, cell, points, index, start):
        self.origin, self.dims, self.cell, self.points, self.index, self.start = origin, dims, cell, points, index, start


class SharedView:
    """The whole-map obstacle cloud of an OccupancyMap and its uniform grid, resident on the device (frp_nmpc_occmap_shared_view_update):
    cloud [cap,3] f64 whose first count[0] rows are local_view(None, cap).cloud[0, :n] to the bit, count / total [1] int32 (count =
    min(total, cap); total = the map's occupied voxels), grid = a SharedViewGrid laid over the map (origin = the map's, dims =
    ceil(map_size / cell)).  update() enqueues the rebuild -- five launches, no read-back, no allocation, capturable -- and the
    corridor takes the view with the grid ON:  corridor_batch_device(None, ..., view=view, cut=...) / DeviceFleet.corridor /
    full_tick(view=...).  Storage beyond count is never written and never read through the grid.
    cap > CORRIDOR_MAX_POINTS (up to CORRIDOR_LARGE_MAX_POINTS) makes a LARGE view (include/frp_nmpc_corridor_large.h): update() is
    frp_nmpc_occmap_shared_view_update_large, and the corridor entries route to frp_nmpc_corridor_batch_large.  Such a view owns what
    that call needs, allocated here once: the fallback's workspace for min(planners, CORRIDOR_LARGE_GROUPS) lists (256 KB each) and
    overflow, int32 [planners] -- after a corridor call of B <= planners planners overflow[:B] is 1 where a local box held more than
    CORRIDOR_LARGE_LIST points (that planner's result is the refusal marker: poly_count = INT_MIN, poly_nfaces = poly_index = 0) and 0
    elsewhere.  At or below CORRIDOR_MAX_POINTS nothing changes: overflow is None and the existing calls are used."""

    def __init__(self, occmap, cap=CORRIDOR_MAX_POINTS, cell=0.5, planners=4096):
        t = occmap.torch
        self.map, self.cap, self.cell = occmap, int(cap), float(cell)
        if not 1 <= self.cap <= CORRIDOR_LARGE_MAX_POINTS:
            raise ValueError(f"cap = {cap}: a shared cloud holds 1 .. FRP_CORRIDOR_LARGE_MAX_POINTS = {CORRIDOR_LARGE_MAX_POINTS} points")
        self.large = self.cap > CORRIDOR_MAX_POINTS
        self.planners = int(planners)
        if self.large and self.planners < 1:
            raise ValueError(f"planners = {planners}: a large view serves at least one planner")
        dims = (ctypes.c_int * 3)()
        m = occmap._map()
        if lib().frp_nmpc_occmap_shared_view_dims(ctypes.byref(m), self.cell, ctypes.byref(dims)) != 0:
            raise ValueError(f"cell = {cell}: not a positive finite size, or more than FRP_CORRIDOR_MAX_CELLS = {CORRIDOR_MAX_CELLS} cells over this map")
        self.dims = tuple(int(v) for v in dims)
        cells = self.dims[0] * self.dims[1] * self.dims[2]
        dev = occmap.device
        self.cloud = t.zeros((self.cap, 3), dtype=t.float64, device=dev)
        self.count = t.zeros((1,), dtype=t.int32, device=dev)
        self.total = t.zeros((1,), dtype=t.int32, device=dev)
        self.grid = SharedViewGrid(occmap.origin, self.dims, self.cell, t.zeros((self.cap, 3), dtype=t.float64, device=dev),
                                   t.zeros((self.cap,), dtype=t.int32, device=dev), t.zeros((cells + 1,), dtype=t.int32, device=dev))
        self._cursor = t.zeros((cells,), dtype=t.int32, device=dev)
        self._sums = t.zeros((OCCMAP_VIEW_MAX_GROUPS,), dtype=t.int32, device=dev)
        self.overflow = self._workspace = None
        if self.large:
            self._workspace = t.zeros((int(lib().frp_nmpc_corridor_large_workspace_bytes(self.planners)),), dtype=t.uint8, device=dev)
            self.overflow = t.zeros((self.planners,), dtype=t.int32, device=dev)

    def _large_args(self, B):
        """frp_nmpc_corridor_large for a corridor call of B planners through this (large) view."""
        if B > self.planners:
            raise ValueError(f"{B} planners through a large view made for planners = {self.planners}")
        return CorridorLarge(self._workspace.data_ptr(), self._workspace.numel(), self.overflow.data_ptr())

    def _args(self):
        g = self.grid
        return OccMapSharedView(self.cap, self.cell, (ctypes.c_int * 3)(*self.dims), self.cloud.data_ptr(), self.count.data_ptr(),
                                self.total.data_ptr(), g.points.data_ptr(), g.index.data_ptr(), g.start.data_ptr(),
                                self._cursor.data_ptr(), self._sums.data_ptr())

    def update(self, stream=None):
        """Rebuild cloud, count, total and grid from the map as it is on `stream` (torch's current stream when None).  Asynchronous."""
        v = self._args()
        self.map._call("frp_nmpc_occmap_shared_view_update_large" if self.large else "frp_nmpc_occmap_shared_view_update", ctypes.byref(v), stream=stream)

    def overflowed(self):
        """Device bool [1]: the map held more occupied voxels than cap at the last update (the first cap in x, y, z order were kept)."""
        return self.total > self.count


def corridor_batch_device(cloud, ref_pos, ref_yaw, ellipsoid, poly_A, poly_b, poly_nfaces, poly_index, poly_count=None,
                          cloud_count=None, consts=None, stream=None, grid=None, cut=None, view=None):
    """frp_nmpc_corridor_batch on device tensors.  cloud [P,3] (shared) or [B,P,3]; ref_pos [B,N,3]; ref_yaw [B,N];
    ellipsoid [B,N,3,3]; outputs poly_A [B,N,F,3], poly_b [B,N,F], poly_nfaces / poly_index [B,N] int32.
    cut (OccupancyMap.cut, a CorridorCut): frp_nmpc_corridor_batch_cut -- every planner sees only the points of the SHARED cloud
    inside its own local box.
    view (a SharedView, with cloud = None and neither grid nor cloud_count): frp_nmpc_corridor_batch_view -- the view's cloud with its
    device-side count AND its grid; combines with cut.  A large view (view.cap > CORRIDOR_MAX_POINTS) goes to
    frp_nmpc_corridor_batch_large with the view's workspace; view.overflow[:B] then tells which planners it refused."""
    import torch
    if view is not None:
        assert cloud is None and grid is None and cloud_count is None, "view= brings its own cloud, grid and count"
        cloud, grid, cloud_count = view.cloud, view.grid, view.count
    c = dict(CORRIDOR_DEFAULTS)
    c.update(consts or {})
    B, N, F, _ = poly_A.shape
    per = 1 if cloud.dim() == 3 else 0
    P = cloud.shape[-2]
    for t in (cloud, ref_pos, ref_yaw, ellipsoid, poly_A, poly_b):
        assert t.is_contiguous() and t.dtype == torch.float64
    assert tuple(ref_pos.shape) == (B, N, 3) and tuple(ellipsoid.shape) == (B, N, 3, 3) and tuple(poly_b.shape) == (B, N, F)
    assert poly_nfaces.dtype == torch.int32 and poly_index.dtype == torch.int32
    s = stream if stream is not None else torch.cuda.current_stream(ref_pos.device)
    cr = Corridor(B, N, F, P, cloud.data_ptr() if P else None, per, cloud_count.data_ptr() if cloud_count is not None else None,
                  ref_pos.data_ptr(), ref_yaw.data_ptr(), ellipsoid.data_ptr(), (ctypes.c_double * 3)(*c["bbox"]),
                  c["seed_len"], c["inflation"], c["offset_x"], poly_A.data_ptr(), poly_b.data_ptr(),
                  poly_nfaces.data_ptr(), poly_index.data_ptr(), poly_count.data_ptr() if poly_count is not None else None)
    if grid is not None:
        assert per == 0, "the grid belongs to a shared cloud"
        cr.grid_origin = (ctypes.c_double * 3)(*grid.origin); cr.grid_cell = grid.cell; cr.grid_dims = (ctypes.c_int * 3)(*grid.dims)
        cr.grid_points = grid.points.data_ptr(); cr.grid_index = grid.index.data_ptr(); cr.grid_start = grid.start.data_ptr()
    if cut is not None:
        assert per == 0, "the cut belongs to a shared cloud"
        assert getattr(cut, "_box", None) is None or cut._box.shape[0] == B, "one local_box row per planner"
    if view is not None and view.cap > CORRIDOR_MAX_POINTS:
        w = view._large_args(B)
        _check(lib().frp_nmpc_corridor_batch_large(ctypes.byref(cr), ctypes.byref(cut) if cut is not None else None, ctypes.byref(w),
                                                   ctypes.c_void_p(s.cuda_stream)), "frp_nmpc_corridor_batch_large")
        return
    if view is not None:
        _check(lib().frp_nmpc_corridor_batch_view(ctypes.byref(cr), ctypes.byref(cut) if cut is not None else None, ctypes.c_void_p(s.cuda_stream)),
               "frp_nmpc_corridor_batch_view")
        return
    if cut is not None:
        _check(lib().frp_nmpc_corridor_batch_cut(ctypes.byref(cr), ctypes.byref(cut), ctypes.c_void_p(s.cuda_stream)), "frp_nmpc_corridor_batch_cut")
        return
    _check(lib().frp_nmpc_corridor_batch(ctypes.byref(cr), ctypes.c_void_p(s.cuda_stream)), "frp_nmpc_corridor_batch")


def corridor_batch_host(cloud, ref_pos, ref_yaw, ellipsoid, F=CORRIDOR_MAX_F, consts=None, device="cuda:0", grid_cell=None):
    """Host convenience: numpy in, (poly_index [B,N], poly_A [B,N,F,3], poly_b [B,N,F], poly_nfaces [B,N], poly_count [B]) out."""
    import torch
    lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)
    B, N, _ = ref_pos.shape
    A = torch.zeros((B, N, F, 3), dtype=torch.float64, device=device); b = torch.zeros((B, N, F), dtype=torch.float64, device=device)
    nf = torch.zeros((B, N), dtype=torch.int32, device=device); pi = torch.zeros((B, N), dtype=torch.int32, device=device)
    cnt = torch.zeros((B,), dtype=torch.int32, device=device)
    d_cloud = dev(cloud).reshape(-1, 3)
    grid = CloudGrid(d_cloud, grid_cell) if grid_cell else None
    corridor_batch_device(d_cloud, dev(ref_pos), dev(ref_yaw), dev(ellipsoid), A, b, nf, pi, cnt, consts=consts, grid=grid)
    torch.cuda.synchronize(device)
    return pi.cpu().numpy(), A.cpu().numpy(), b.cpu().numpy(), nf.cpu().numpy(), cnt.cpu().numpy()


def tube_batch_host(plans, consts=None, device="cuda:0"):
    """Host convenience: plans [B,N,17] (rows 0..N-1 of the plan deque) -> E [B,N,3,3]."""
    import torch
    lib()
    plans = np.ascontiguousarray(plans, dtype=np.float64)
    B, N, _ = plans.shape
    mo = torch.zeros((B, N + 1, L.NZ), dtype=torch.float64, device=device)
    mo[:, :N] = torch.from_numpy(plans).to(device)
    E = torch.empty((B, N, 3, 3), dtype=torch.float64, device=device)
    tube_batch_device(mo, E, consts)
    torch.cuda.synchronize(device)
    return E.cpu().numpy()


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
        s = stream if stream is not None else self.torch.cuda.current_stream(self.solver.device)
        _check(lib().frp_nmpc_mode_batch(self.B, self.N, ctypes.c_void_p(self.mpc_output.data_ptr()), ctypes.c_void_p(time_offset.data_ptr()),
                                         ctypes.c_void_p(kino_size.data_ptr()), 1 if kino_size.numel() > 1 else 0,
                                         ctypes.c_void_p(end_pt.data_ptr()), 1 if end_pt.dim() == 2 else 0, float(Ts), float(radius),
                                         ctypes.c_void_p(self.mode.data_ptr()), ctypes.c_void_p(s.cuda_stream)), "frp_nmpc_mode_batch")

    def reset_mode(self):
        """A new kinodynamic path puts every planner back on the normal solver (nmpc_solver.cpp:218)."""
        self.mode.fill_(L.MODEL_NORMAL)

    def to_device(self, a, dtype=None):
        t = self.torch
        return t.from_numpy(np.ascontiguousarray(a)).to(self.solver.device, dtype=dtype)

    def pack(self, external_acc, ref_pos, ref_yaw, stream=None):
        s = stream if stream is not None else self.torch.cuda.current_stream(self.solver.device)
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
        _check(lib().frp_nmpc_pack_batch(ctypes.byref(pk), ctypes.c_void_p(s.cuda_stream)), "frp_nmpc_pack_batch")
        ds._packed_by = self

    def update(self, stream=None, keep_failed=True, accept=None):
        """accept [B] int32: the planners whose result is taken over are those with accept == 1 (TickState.accept, the reference's whole
        rule) instead of those with solver.exitflag == 1 (its first branch)."""
        s = stream if stream is not None else self.torch.cuda.current_stream(self.solver.device)
        ds = self.solver
        flags = accept if accept is not None else ds.exitflag
        _check(lib().frp_nmpc_update_batch(self.B, self.N, ctypes.c_void_p(ds.z.data_ptr()),
                                           ctypes.c_void_p(flags.data_ptr()) if keep_failed else None,
                                           ctypes.c_void_p(self.mpc_output.data_ptr()), ctypes.c_void_p(s.cuda_stream)),
               "frp_nmpc_update_batch")

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
        s = stream if stream is not None else self.torch.cuda.current_stream(self.solver.device)
        flags = keep if keep is not None else self.solver.exitflag
        _check(lib().frp_nmpc_coldstart_batch(self.B, self.N, ctypes.c_void_p(state.data_ptr()) if state is not None else None,
                                              ctypes.c_void_p(flags.data_ptr()) if only_failed else None,
                                              float(thrust), ctypes.c_void_p(self.mpc_output.data_ptr()),
                                              ctypes.c_void_p(s.cuda_stream)), "frp_nmpc_coldstart_batch")

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


class Vehicle:
    """The vehicle of every planner of a DeviceFleet, on the device (include/frp_nmpc_vehicle.h): a tracking plant that flies the command
    timer's samples and the reference's odometry callbacks, so that FleetFSM.period(..., vehicle=...) closes the loop without the host.
    Owns, all float64 device tensors unless noted: x [B,9] the plant state (position, world velocity, roll pitch yaw), hold [B,8] the last
    published position and yaw, f_true [B,3] the TRUE mass-normalised external force (the caller writes it; what the planner is told is
    the `force` / `force_fresh` of period(): the caller's own, or a ForceEstimator's), msg [B,13] the last odometry message, state [B,9] what the callbacks made of it (the
    `state` of period(), exec_step() and full_tick()), state_prev [B,9], fresh [B] int32 (ones: every planner hears every message), and
    with trace=True trace [B,S,9] / sat [B,S] int32 of the last step().
    kp, kv, ka, n_sub, mass, g, dt_cmd: VEHICLE_DEFAULTS -- the controller has no reference counterpart, the plant is the planner's own
    model (csrc/frp_model.hpp).  odom_type: ODOM_BODY (odometryTransCallback: the RotorS message, body-frame twist) or ODOM_WORLD."""

    def __init__(self, fleet, kp=None, kv=None, ka=None, n_sub=None, odom_type=ODOM_BODY, mass=None, g=None, dt_cmd=None, trace=False, S=5):
        t = fleet.torch
        dev = fleet.solver.device
        self.torch, self.fleet, self.B, self.S = t, fleet, fleet.B, int(S)
        k = dict(VEHICLE_DEFAULTS)
        k.update({n: v for n, v in (("kp", kp), ("kv", kv), ("ka", ka), ("n_sub", n_sub), ("mass", mass), ("g", g), ("dt_cmd", dt_cmd)) if v is not None})
        self.kp, self.kv, self.ka = (tuple(float(v) for v in k[n]) for n in ("kp", "kv", "ka"))
        assert len(self.kp) == len(self.kv) == len(self.ka) == 3
        self.n_sub, self.mass, self.g, self.dt_cmd = int(k["n_sub"]), float(k["mass"]), float(k["g"]), float(k["dt_cmd"])
        if odom_type not in (ODOM_WORLD, ODOM_BODY):
            raise ValueError("odom_type is ODOM_WORLD or ODOM_BODY")
        self.odom_type = int(odom_type)
        f64 = dict(dtype=t.float64, device=dev)
        self.x, self.state, self.state_prev = (t.zeros((self.B, VEHICLE_STATE), **f64) for _ in range(3))
        self.hold = t.zeros((self.B, VEHICLE_HOLD_STRIDE), **f64)
        self.f_true = t.zeros((self.B, 3), **f64)
        self.msg = t.zeros((self.B, VEHICLE_MSG_STRIDE), **f64)
        self.fresh = t.ones((self.B,), dtype=t.int32, device=dev)
        self.trace = t.zeros((self.B, self.S, VEHICLE_STATE), **f64) if trace else None
        self.sat = t.zeros((self.B, self.S), dtype=t.int32, device=dev) if trace else None
        self.estimator = None   # a ForceEstimator attaches itself here: step() and reset() then feed and reset it

    def _stream(self, stream):
        return ctypes.c_void_p((stream if stream is not None else self.torch.cuda.current_stream(self.x.device)).cuda_stream)

    def _arg(self, a, dtype, shape):
        assert self.torch.is_tensor(a) and a.dtype == dtype and tuple(a.shape) == shape and a.is_contiguous() and a.device == self.x.device, \
            (tuple(a.shape), shape, a.dtype)
        return ctypes.c_void_p(a.data_ptr())

    def reset(self, x0, mask=None, stream=None):
        """frp_nmpc_vehicle_reset: where mask [B] int32 != 0 (None: everywhere) x <- x0 [B,9] and hold <- its position and yaw: the
        vehicle hovers there until something is published.  `state` is the callbacks': call odometry(fsm) to publish the new pose."""
        t = self.torch
        m = self._arg(mask, t.int32, (self.B,)) if mask is not None else None
        _check(lib().frp_nmpc_vehicle_reset(self.B, self._arg(x0, t.float64, (self.B, VEHICLE_STATE)), m, ctypes.c_void_p(self.x.data_ptr()),
                                            ctypes.c_void_p(self.hold.data_ptr()), self._stream(stream)), "frp_nmpc_vehicle_reset")
        if self.estimator is not None:
            self.estimator.reset(mask, stream)

    def step(self, commands, stream=None):
        """frp_nmpc_vehicle_step: the S samples of a Commands object (cmd [B,S,16], kind [B,S]) flown in order under f_true; x and hold
        in place, trace / sat where the object was made with trace=True (S is then the constructor's).
        With a ForceEstimator attached (self.estimator): frp_nmpc_vehicle_step_observed instead -- the same flight, and the thrust of every
        sample into the estimator's `thrust`, the trace into this object's own trace or else the estimator's `meas` --, then its update()."""
        t = self.torch
        S = int(commands.cmd.shape[1])
        if self.trace is not None and S != self.S:
            raise ValueError(f"this Vehicle traces S = {self.S} samples per call, the commands hold {S}")
        est = self.estimator
        if est is not None and S != est.S:
            raise ValueError(f"the attached ForceEstimator takes S = {est.S} samples per call, the commands hold {S}")
        trace = self.trace if self.trace is not None else est.meas if est is not None else None
        v = VehicleArgs(self.B, S, self.n_sub, self.mass, self.g, self.dt_cmd, (ctypes.c_double * 3)(*self.kp), (ctypes.c_double * 3)(*self.kv),
                        (ctypes.c_double * 3)(*self.ka), self.x.data_ptr(), self.f_true.data_ptr(),
                        self._arg(commands.cmd, t.float64, (self.B, S, COMMAND_STRIDE)).value, self._arg(commands.kind, t.int32, (self.B, S)).value,
                        self.hold.data_ptr(), trace.data_ptr() if trace is not None else None, self.sat.data_ptr() if self.sat is not None else None)
        if est is None:
            _check(lib().frp_nmpc_vehicle_step(ctypes.byref(v), self._stream(stream)), "frp_nmpc_vehicle_step")
            return
        _check(lib().frp_nmpc_vehicle_step_observed(ctypes.byref(v), ctypes.c_void_p(est.thrust.data_ptr()), self._stream(stream)), "frp_nmpc_vehicle_step_observed")
        est.update(meas=trace, stream=stream)

    def message(self, stream=None):
        """frp_nmpc_vehicle_message: msg <- the odometry message of x for this object's odom_type."""
        _check(lib().frp_nmpc_vehicle_message(self.B, self.odom_type, ctypes.c_void_p(self.x.data_ptr()), ctypes.c_void_p(self.msg.data_ptr()),
                                              self._stream(stream)), "frp_nmpc_vehicle_message")

    def odometry(self, fsm, msg=None, fresh=None, stream=None):
        """odometryCallback / odometryTransCallback (nmpc_manage.cpp:421-478) into state, state_prev and fsm.have_odom.  msg None (a
        simulated fleet): the message is produced from the plant first, message(); msg [B,13] (a real fleet): the callback alone.
        fresh [B] int32: who got a message (None: everybody)."""
        t = self.torch
        if msg is None:
            self.message(stream)
            msg = self.msg
        fresh = self.fresh if fresh is None else fresh
        _check(lib().frp_nmpc_vehicle_odometry(self.B, self.odom_type, self._arg(msg, t.float64, (self.B, VEHICLE_MSG_STRIDE)), self._arg(fresh, t.int32, (self.B,)),
                                               ctypes.c_void_p(self.state.data_ptr()), ctypes.c_void_p(self.state_prev.data_ptr()),
                                               self._arg(fsm.have_odom, t.int32, (self.B,)), self._stream(stream)), "frp_nmpc_vehicle_odometry")


class ForceEstimator:
    """The force estimator of every vehicle of a Vehicle, on the device (include/frp_nmpc_estimator.h): a velocity-residual observer on the
    planner's own model that turns the thrust and the states of the samples a vehicle flew into the `force` / `force_fresh` pair of
    FleetFSM.period -- what the planner is TOLD, where vehicle.f_true is what acts.  It has no reference counterpart (the reference
    subscribes to a wrench another node publishes), and its measurements are the TRUE plant states of the vehicle's trace: noise is the
    caller's to add (update(meas=...) takes any [B,S,9] tensor).
    Attaches itself as vehicle.estimator: Vehicle.step then launches frp_nmpc_vehicle_step_observed and update(), Vehicle.reset resets
    it under the same mask.  The loop closes through arguments period() already has:
        fsm.period(planner, occmap, None, clock, force=est.force, force_fresh=est.fresh, vehicle=veh)
    -- the force callback of period p hears the estimate the end of period p - 1 left.
    Owns, float64 device tensors unless noted: meas [B,S,9] (the vehicle's trace where it keeps none of its own), thrust [B,S], f_hat [B,3],
    y_prev [B,9], count [B] int32 (-1: no previous measurement), force [B,3], fresh [B] int32 and, with residual=True, residual [B,S,3] /
    status [B,S] int32 (EST_*) of the last update().
    tau, min_samples: ESTIMATOR_DEFAULTS -- CHOSEN, not derived, as VEHICLE_DEFAULTS' gains are: a first-order filter of time constant tau
    on the residual, alpha = -expm1(-dt / tau) per sample with dt the vehicle's dt_cmd, computed here on the host; the estimate counts
    as fresh after min_samples residuals."""

    def __init__(self, vehicle, tau=None, min_samples=None, residual=False):
        import math
        t = vehicle.torch
        dev = vehicle.x.device
        k = dict(ESTIMATOR_DEFAULTS)
        k.update({n: v for n, v in (("tau", tau), ("min_samples", min_samples)) if v is not None})
        self.torch, self.vehicle, self.B, self.S = t, vehicle, vehicle.B, vehicle.S
        self.tau, self.min_samples, self.dt = float(k["tau"]), int(k["min_samples"]), float(vehicle.dt_cmd)
        if not (self.tau > 0.0 and math.isfinite(self.tau)) or self.min_samples < 1:
            raise ValueError("ForceEstimator: tau finite and > 0, min_samples >= 1")
        self.alpha = -math.expm1(-self.dt / self.tau)
        f64 = dict(dtype=t.float64, device=dev)
        i32 = dict(dtype=t.int32, device=dev)
        self.meas, self.thrust = t.zeros((self.B, self.S, VEHICLE_STATE), **f64), t.zeros((self.B, self.S), **f64)
        self.f_hat, self.y_prev, self.force = t.zeros((self.B, 3), **f64), t.zeros((self.B, VEHICLE_STATE), **f64), t.zeros((self.B, 3), **f64)
        self.count, self.fresh = t.full((self.B,), -1, **i32), t.zeros((self.B,), **i32)
        self.residual = t.zeros((self.B, self.S, 3), **f64) if residual else None
        self.status = t.zeros((self.B, self.S), **i32) if residual else None
        vehicle.estimator = self

    def update(self, meas=None, thrust=None, stream=None):
        """frp_nmpc_estimator_update: the S samples of meas [B,S,9] / thrust [B,S] (None: this object's own) absorbed in order; f_hat,
        y_prev and count in place, force and fresh written."""
        t, v = self.torch, self.vehicle
        meas = self.meas if meas is None else meas
        thrust = self.thrust if thrust is None else thrust
        p = lambda a: a.data_ptr() if a is not None else None
        e = EstimatorArgs(self.B, self.S, self.min_samples, self.dt, self.alpha, v._arg(meas, t.float64, (self.B, self.S, VEHICLE_STATE)).value,
                          v._arg(thrust, t.float64, (self.B, self.S)).value, p(self.f_hat), p(self.y_prev), p(self.count), p(self.force), p(self.fresh),
                          p(self.residual), p(self.status))
        _check(lib().frp_nmpc_estimator_update(ctypes.byref(e), v._stream(stream)), "frp_nmpc_estimator_update")

    def reset(self, mask=None, stream=None):
        """frp_nmpc_estimator_reset: where mask [B] int32 != 0 (None: everywhere) f_hat <- 0, count <- -1, force <- 0, fresh <- 0."""
        t, v = self.torch, self.vehicle
        m = v._arg(mask, t.int32, (self.B,)) if mask is not None else None
        vp = lambda a: ctypes.c_void_p(a.data_ptr())
        _check(lib().frp_nmpc_estimator_reset(self.B, m, vp(self.f_hat), vp(self.y_prev), vp(self.count), vp(self.force), vp(self.fresh), v._stream(stream)),
               "frp_nmpc_estimator_reset")


class FleetFSM:
    """NMPCManage (plan_manage/src/nmpc_manage.cpp) for the B planners of a DeviceFleet, on the device (include/frp_nmpc_fsm.h): a fleet goes
    goal -> yaw alignment -> plan -> execute -> replan on force / collision / failure -> goal reached -> next goal without the host reading
    anything back.  Owns the state tensors, [B] int32 unless noted: state (FSM_*, INIT at first), have_odom (the CALLER sets it, or a
    Vehicle's odometry callbacks do), have_target, have_traj (NMPCManage's have_traj_, not fleet.have_traj = have_mpc_traj_), trigger,
    call_init_yaw, consider_force, replan_force_surpass, surpass_count, plan_fail_count; end_pt, external_acc, last_external_acc [B,3] f64,
    init_yaw [B] f64, yaw_odom [B,9] f64, change_yaw_time / kino_start_time [B] f64 on the caller's clock, all zero at first (the reference
    leaves the doubles uninitialised); search [B], the mask of the last exec_step; mpc_start [B] f64, pre_mpc_start_time_ as period() keeps it.
    Shares exec_mpc, cmd_status and pub_end with `tick` (a TickState, made here when None) and mode with the fleet; exec_mpc is ZEROED
    here: under the state machine a planner solves only after its first successful search (the reference's exec_mpc_ = false).
    The command timer's yaw inputs are this object's: DeviceFleet.commands(..., odom=fsm.yaw_odom, init_yaw=fsm.init_yaw, t_yaw=fsm.t_yaw(...)).
    This layer is structurally unpinned: the reference has no test vectors for it; tests/fsm_oracle.py is the restatement it is held to."""

    INT_FIELDS = ("state", "have_odom", "have_target", "have_traj", "trigger", "call_init_yaw", "consider_force", "replan_force_surpass",
                  "surpass_count", "plan_fail_count")
    F64_FIELDS = (("end_pt", 3), ("external_acc", 3), ("last_external_acc", 3), ("init_yaw", 0), ("yaw_odom", 9), ("change_yaw_time", 0),
                  ("kino_start_time", 0))
    MAX_STEPS = 5   # exec steps per period: exec_timer_ runs at 100 Hz, the tick at 20 Hz
    S = 5           # command callbacks per period

    def __init__(self, fleet, tick=None, ext_noise_bound=FSM_EXT_NOISE_BOUND):
        t = fleet.torch
        dev = fleet.solver.device
        self.torch, self.fleet, self.B = t, fleet, fleet.B
        self.tick = tick if tick is not None else TickState(fleet)
        assert self.tick.B == self.B
        self.ext_noise_bound = float(ext_noise_bound)
        for n in self.INT_FIELDS + ("search",):
            setattr(self, n, t.zeros((self.B,), dtype=t.int32, device=dev))
        self.state.fill_(FSM_INIT)
        for n, w in self.F64_FIELDS:
            setattr(self, n, t.zeros((self.B, w) if w else (self.B,), dtype=t.float64, device=dev))
        self.exec_mpc, self.cmd_status, self.pub_end, self.mode = self.tick.exec_mpc, self.tick.cmd_status, self.tick.pub_end, fleet.mode
        self.exec_mpc.zero_()
        f64 = dict(dtype=t.float64, device=dev)
        self.mpc_start = t.zeros((self.B,), **f64)
        # period()'s own buffers: a capture of it allocates nothing of the caller's
        z = lambda: t.zeros((self.B,), dtype=t.int32, device=dev)
        self.safety_out = SafetyCheck(z(), z(), z(), z())
        self.ref_pos, self.ref_yaw = t.zeros((self.B, fleet.N, 3), **f64), t.zeros((self.B, fleet.N), **f64)
        self.t_step, self.toff = t.zeros((self.B,), **f64), t.zeros((self.B,), **f64)
        self.t_cmd, self.t_rot = t.zeros((self.B, self.S), **f64), t.zeros((self.B, self.S), **f64)
        self._ramp = t.arange(self.S, **f64) * FSM_EXEC_PERIOD
        self._ran = t.zeros((self.B,), dtype=t.bool, device=dev)
        self.commands_out = None

    def struct(self):
        p = lambda n: getattr(self, n).data_ptr() if getattr(self, n) is not None else None
        return Fsm(self.B, *[p(n) for n, _ in Fsm._fields_[1:]])

    def arrays(self):
        """Every state array on the host (a synchronising read-back: tests and logs)."""
        names = self.INT_FIELDS + ("exec_mpc", "cmd_status", "pub_end", "search") + tuple(n for n, _ in self.F64_FIELDS)
        return {n: getattr(self, n).cpu().numpy() for n in names}

    def _stream(self, stream):
        return stream if stream is not None else self.torch.cuda.current_stream(self.state.device)

    def _arg(self, a, dtype, shape):
        assert self.torch.is_tensor(a) and a.dtype == dtype and tuple(a.shape) == shape and a.is_contiguous() and a.device == self.state.device, \
            (tuple(a.shape), shape, a.dtype)
        return ctypes.c_void_p(a.data_ptr())

    def goal(self, goal, fresh, stream=None):
        """goalCallback (nmpc_manage.cpp:481-493): goal [B,3] f64, fresh [B] int32 (non-zero: a message for this planner)."""
        t, f = self.torch, self.struct()
        _check(lib().frp_nmpc_fsm_goal(ctypes.byref(f), self._arg(goal, t.float64, (self.B, 3)), self._arg(fresh, t.int32, (self.B,)),
                                       ctypes.c_void_p(self._stream(stream).cuda_stream)), "frp_nmpc_fsm_goal")

    def force(self, force, fresh, stream=None):
        """extforceCallback (nmpc_manage.cpp:366-418): force [B,3] f64 (mass-normalised), fresh [B] int32."""
        t, f = self.torch, self.struct()
        _check(lib().frp_nmpc_fsm_force(ctypes.byref(f), self._arg(force, t.float64, (self.B, 3)), self._arg(fresh, t.int32, (self.B,)),
                                        self.ext_noise_bound, ctypes.c_void_p(self._stream(stream).cuda_stream)), "frp_nmpc_fsm_force")

    def mpc_result(self, result=None, stream=None):
        """The switch of mpcCallback (nmpc_manage.cpp:60-97) on result [B] int32 (None: tick.result, as full_tick(tick=...) left it)."""
        f = self.struct()
        result = self.tick.result if result is None else result
        _check(lib().frp_nmpc_fsm_mpc(ctypes.byref(f), self._arg(result, self.torch.int32, (self.B,)), ctypes.c_void_p(self._stream(stream).cuda_stream)),
               "frp_nmpc_fsm_mpc")

    def safety_verdict(self, goal_blocked, first_hit, stream=None):
        """The transitions of checkReplanCallback (nmpc_manage.cpp:318-325, :333-338) for verdicts [B] int32 the caller holds."""
        t, f = self.torch, self.struct()
        _check(lib().frp_nmpc_fsm_safety(ctypes.byref(f), self._arg(goal_blocked, t.int32, (self.B,)), self._arg(first_hit, t.int32, (self.B,)),
                                         ctypes.c_void_p(self._stream(stream).cuda_stream)), "frp_nmpc_fsm_safety")

    def safety(self, occmap, planner, local_box=None, stride=5, stream=None, out=None):
        """One checkReplanCallback (nmpc_manage.cpp:285-341): OccupancyMap.safety_check on this object's end_pt (moved in place where the
        search finds a free goal) / have_target / have_traj and the planner's kino_path / kino_size, then the transitions.  Returns the
        SafetyCheck (out, or this object's own safety_out)."""
        out = out if out is not None else self.safety_out
        occmap.safety_check(self.end_pt, planner.kino_path, planner.kino_size, have_target=self.have_target, have_traj=self.have_traj,
                            local_box=local_box, stride=stride, stream=stream, out=out)
        self.safety_verdict(out.goal_blocked, out.first_hit, stream)
        return out

    def bind(self, planner):
        """Makes the planner's retry buffers exist (an allocation: period() and exec_step() call it; call it once before a capture)."""
        assert planner.B == self.B and planner.device == self.state.device
        if planner._retry is None:
            planner._retry = [self.torch.zeros_like(planner._q[0]), self.torch.zeros_like(planner._q[0])]

    def exec_step(self, planner, state, t_cur, now, local_box=None, end_vel=None, stream=None, Ts=None, mass=None, g=None):
        """One execFSMCallback (nmpc_manage.cpp:109-260) for every planner: frp_nmpc_fsm_exec_begin writes self.search and, for the planners
        that search, the start / retry state straight into the AstarPlanner's own buffers; planner.plan(active=self.search) with this
        object's end_pt and external_acc; frp_nmpc_fsm_exec_end applies the verdict (planner.status).  state [B,9] f64 odometry, t_cur [B]
        f64 seconds since pre_mpc_start_time_, now [1] f64; end_vel [B,3] or None: the planner's uploaded one (zeros at first).
        Ts / mass / g: COMMAND_DEFAULTS.  Planners that do not search keep their A* rows and their path."""
        self.bind(planner)
        s = self._stream(stream)
        self.exec_begin(state, t_cur, now, planner._q[0], planner._q[1], planner._q[2], planner._retry[0], planner._retry[1], s, Ts, mass, g)
        planner.plan(init=True, local_box=local_box, stream=s, active=self.search, end_pt=self.end_pt, end_vel=end_vel, external_acc=self.external_acc)
        self.exec_end(planner.status, now, s)

    def exec_begin(self, state, t_cur, now, start_pt, start_vel, start_acc, retry_pt, retry_vel, stream=None, Ts=None, mass=None, g=None):
        """frp_nmpc_fsm_exec_begin: the first half of exec_step, for a caller with its own search.  Writes self.search and, for the
        planners that search alone, the five [B,3] f64 start / retry tensors; reads the fleet's pre_plan and the tick's exit_code."""
        t = self.torch
        k = dict(COMMAND_DEFAULTS)
        k.update({n: float(v) for n, v in (("Ts", Ts), ("mass", mass), ("g", g)) if v is not None})
        fl, B = self.fleet, self.B
        f = self.struct()
        v = lambda a: self._arg(a, t.float64, (B, 3)).value
        i = FsmExecIn(fl.N, k["Ts"], k["mass"], k["g"], self._arg(state, t.float64, (B, 9)).value, self._arg(fl.pre_plan, t.float64, (B, fl.N, L.NZ)).value,
                      self._arg(self.tick.exit_code, t.int32, (B,)).value, self._arg(t_cur, t.float64, (B,)).value, self._arg(now, t.float64, (1,)).value,
                      self.search.data_ptr(), v(start_pt), v(start_vel), v(start_acc), v(retry_pt), v(retry_vel))
        _check(lib().frp_nmpc_fsm_exec_begin(ctypes.byref(f), ctypes.byref(i), ctypes.c_void_p(self._stream(stream).cuda_stream)), "frp_nmpc_fsm_exec_begin")

    def exec_end(self, astar_status, now, stream=None):
        """frp_nmpc_fsm_exec_end: the second half of exec_step, on self.search and astar_status [B] int32 (AstarPlanner.status)."""
        t, f = self.torch, self.struct()
        _check(lib().frp_nmpc_fsm_exec_end(ctypes.byref(f), ctypes.c_void_p(self.search.data_ptr()), self._arg(astar_status, t.int32, (self.B,)),
                                           self._arg(now, t.float64, (1,)), ctypes.c_void_p(self._stream(stream).cuda_stream)), "frp_nmpc_fsm_exec_end")

    def time_offset(self, mpc_start, out=None):
        """(mpc_start_time_ - kino_start_time_).toSec() (nmpc_solver.cpp:436) on the device: mpc_start [1] or [B] f64 -> [B]."""
        return self.torch.sub(mpc_start, self.kino_start_time, out=out)

    def t_yaw(self, now, S, out=None):
        """(now - change_yaw_time_).toSec() (nmpc_solver.cpp:885) of S command callbacks at now, now + 0.01, ...: now [1] f64 -> [B,S]."""
        t = self.torch
        ramp = self._ramp if S == self.S else t.arange(S, dtype=t.float64, device=now.device) * FSM_EXEC_PERIOD
        return t.sub((now + ramp)[None, :], self.change_yaw_time[:, None], out=out)

    def period(self, planner, occmap, state, clock, cloud=None, *, goal=None, goal_fresh=None, force=None, force_fresh=None, fsm_steps=1,
               local_box=None, end_vel=None, stream=None, vehicle=None, **tick_args):
        """One 50 ms period of the fleet, everything enqueued on `stream` (torch's current stream when None), nothing read back, in this
        fixed order:
          1. goal(goal, goal_fresh) and force(force, force_fresh), each where given;
          2. safety(occmap, planner, local_box);
          3. fsm_steps (1 ... 5) exec_step()s, step k at clock[k] with t_cur = clock[k] - mpc_start;
          4. fleet.full_tick(external_acc, planner.kino_path, time_offset, cloud, ..., kino_size=planner.kino_size, state=state, tick=self.tick,
             end_pt=self.end_pt, **tick_args) at clock[fsm_steps], with time_offset = clock[fsm_steps] - kino_start_time; mpc_start <- that
             time for the planners that got past solveNMPC's gates (tick.gate == TICK_RUN; nmpc_solver.cpp:358-359);
          5. mpc_result();
          6. fleet.commands with S = 5 callbacks at clock[fsm_steps + 1], + 0.01, ...: t_cur from mpc_start, t_yaw from change_yaw_time, the
             yaw inputs this object's; tick.reset_output <- the returned reset_output.
        clock: [fsm_steps + 2] f64 device tensor on the caller's clock (clock_for() fills the reference's timer periods in).  state [B,9]
        f64 odometry.  cloud and tick_args (grid, cut, view, cloud_count, tube_consts, corridor_consts, Ts) are full_tick's.  A
        captured period replays with new contents of goal / goal_fresh / force / force_fresh / state / clock.  Returns the Commands.
        vehicle: a Vehicle, or None.  With one, three more launches follow step 6 --
          7. vehicle.step(commands) under vehicle.f_true, vehicle.odometry(self): message, then the callback into vehicle.state and have_odom
        -- and `state` is vehicle.state (pass it, or None): the next period plans from what the vehicle flew, so K periods are one graph
        with no host in the loop.  The force estimator stays the caller's: force / force_fresh.  With None the launches are steps 1-6."""
        t = self.torch
        if vehicle is not None:
            assert vehicle.B == self.B and (state is None or state is vehicle.state), "with a vehicle the odometry is vehicle.state"
            state = vehicle.state
        assert 1 <= int(fsm_steps) <= self.MAX_STEPS and tuple(clock.shape) == (int(fsm_steps) + 2,) and clock.dtype == t.float64
        fl, tk = self.fleet, self.tick
        s = self._stream(stream)
        self.bind(planner)
        if goal is not None:
            self.goal(goal, goal_fresh, s)
        if force is not None:
            self.force(force, force_fresh, s)
        self.safety(occmap, planner, local_box=local_box, stream=s)
        with t.cuda.stream(s):
            for k in range(int(fsm_steps)):
                now = clock[k:k + 1]
                t.sub(now, self.mpc_start, out=self.t_step)
                self.exec_step(planner, state, self.t_step, now, local_box=local_box, end_vel=end_vel, stream=s, Ts=tick_args.get("Ts"))
            now = clock[fsm_steps:fsm_steps + 1]
            self.time_offset(now, out=self.toff)
            fl.full_tick(self.external_acc, planner.kino_path, self.toff, cloud, self.ref_pos, self.ref_yaw, stream=s, kino_size=planner.kino_size,
                         state=state, tick=tk, end_pt=self.end_pt, **tick_args)
            t.eq(tk.gate, TICK_RUN, out=self._ran)
            t.where(self._ran, now, self.mpc_start, out=self.mpc_start)
            self.mpc_result(stream=s)
            first = clock[fsm_steps + 1:fsm_steps + 2]
            t.sub((first + self._ramp)[None, :], self.mpc_start[:, None], out=self.t_cmd)
            self.t_yaw(first, self.S, out=self.t_rot)
            self.commands_out = fl.commands(self.t_cmd, self.cmd_status, self.pub_end, tk.cmd_end_pt, odom=self.yaw_odom, init_yaw=self.init_yaw,
                                            t_yaw=self.t_rot, out=self.commands_out, stream=s, Ts=tick_args.get("Ts"))
            tk.reset_output = self.commands_out.reset_output
        if vehicle is not None:
            vehicle.step(self.commands_out, s)
            vehicle.odometry(self, stream=s)
        return self.commands_out

    @staticmethod
    def clock_for(t0, fsm_steps):
        """The reference's timers for a period starting at t0 (host floats): exec steps at t0, t0 + 0.01, ..., the tick and the first
        command callback one exec period after the last step and after the tick."""
        return [t0 + FSM_EXEC_PERIOD * k for k in range(int(fsm_steps) + 2)]
