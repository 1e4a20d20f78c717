"""forces_resilient_planner_amd.capi against include/*.h: every ctypes mirror field by field, the signature table against the prototypes,
the mirrored macros, and solver as the whole facade of the modules behind it.  No GPU; gcc only."""
import ctypes
import inspect
import os
import re
import subprocess

from forces_resilient_planner_amd import batch, capi, fleet, flight, occmap, planning, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HEADERS = sorted(h for h in os.listdir(INC) if h.endswith(".h"))


def _compile(tmp_path, name, header, asserts):
    src = tmp_path / f"{name}.c"
    src.write_text(f'#include <stddef.h>\n#include "{header}"\n' + "".join(f"_Static_assert({a}, \"{a}\");\n" for a in asserts) + "int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I", INC, "-c", str(src), "-o", str(tmp_path / f"{name}.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _mirrors():
    return [c for _, c in inspect.getmembers(capi, inspect.isclass) if issubclass(c, ctypes.Structure) and c.__module__ == capi.__name__]


def test_every_mirror_has_the_headers_layout_field_by_field(tmp_path):
    mirrors = _mirrors()
    assert len(mirrors) >= 28
    by_header = {}
    for cls in mirrors:
        assert cls in capi.C_TYPES, f"{cls.__name__} records no C type and header in capi.C_TYPES"
        ctype, header = capi.C_TYPES[cls]
        assert header in HEADERS
        a = [f"sizeof({ctype}) == {ctypes.sizeof(cls)}"] + [f"offsetof({ctype}, {f[0]}) == {getattr(cls, f[0]).offset}" for f in cls._fields_]
        assert len(a) == 1 + len(cls._fields_)
        by_header.setdefault(header, []).extend(a)
    assert set(capi.C_TYPES) == set(mirrors)
    _compile(tmp_path, "all", "frp_nmpc.h", [a for h in sorted(by_header) for a in by_header[h]])
    for i, h in enumerate(sorted(by_header)):       # ... and through each struct's own header
        _compile(tmp_path, f"own{i}", h, by_header[h])


def _prototypes():
    """{name: (return type, parameter texts, header)} of every frp_nmpc_* / FORCESNLPsolver_*_solve function include/*.h declare, comments
    stripped first.  No prototype has an inline function-pointer parameter (the solvers' callback goes through the frp_forces_extfunc
    typedef), so a parameter list never holds a parenthesis or a comma of its own: the assert below keeps that true."""
    out = {}
    for h in HEADERS:
        s = open(os.path.join(INC, h)).read()
        s = re.sub(r"/\*.*?\*/", "", s, flags=re.S)
        s = re.sub(r"//[^\n]*", "", s)
        s = re.sub(r"(?m)^\s*#.*$", "", s)        # (FRP_NMPC_ABI_CHECK's macro body calls a function: not a declaration)
        for m in re.finditer(r"([A-Za-z_][\w \*]*?)\b((?:frp_nmpc_\w+|FORCESNLPsolver_\w+_solve))\s*\(([^;{]*?)\)\s*;", s):
            ret, name, params = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
            assert "(" not in params and ")" not in params, (name, params)
            assert name not in out, name
            out[name] = (ret, [] if params == "void" else [p.strip() for p in params.split(",")], h)
    return out


def test_the_signature_table_is_the_headers():
    protos = _prototypes()
    assert set(protos) == set(capi.SIGNATURES)
    order = {}
    scalars = {"int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
    for name, (ret, params, h) in protos.items():
        order.setdefault(h, []).append(name)
        restype, argtypes = capi.SIGNATURES[name]
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        for i, (p, a) in enumerate(zip(params, argtypes)):      # a scalar sits where the prototype has that scalar, an address everywhere else
            by_value = "*" not in p and "[" not in p and p.rsplit(" ", 1)[0] in scalars
            assert by_value or "*" in p or "[" in p or p.startswith("frp_forces_extfunc "), (name, p)
            assert (a is scalars[p.rsplit(" ", 1)[0]]) if by_value else (a not in scalars.values()), (name, i, p, a)
        assert (restype is ctypes.c_size_t) == (ret == "size_t"), (name, ret)
        assert (restype is ctypes.c_char_p) == (ret == "const char *"), (name, ret)
        assert (restype is None) == (ret == "void"), (name, ret)
        assert ret in ("int", "size_t", "const char *", "void") and (ret != "int" or restype is ctypes.c_int), (name, ret)
    # grouped by header, in each header's declaration order; the *_EXPORTS lists are those groups
    table = list(capi.SIGNATURES)
    for h, names in order.items():
        i = table.index(names[0])
        assert table[i:i + len(names)] == names, h
    views = dict(EXPORTS="frp_nmpc.h", FUSE_EXPORTS="frp_nmpc_occmap_fuse.h", FUSE_BATCH_EXPORTS="frp_nmpc_occmap_fuse_batch.h",
                 FUSE_POINTS_EXPORTS="frp_nmpc_occmap_fuse_points.h", CHECK_EXPORTS="frp_nmpc_occmap_check.h", DISTANCE_EXPORTS="frp_nmpc_occmap_distance.h",
                 RENDER_EXPORTS="frp_nmpc_occmap_render.h", RENDER_SCAN_EXPORTS="frp_nmpc_occmap_render_scan.h", VIEW_EXPORTS="frp_nmpc_occmap_view.h",
                 LARGE_EXPORTS="frp_nmpc_corridor_large.h", COMMAND_EXPORTS="frp_nmpc_command.h", OUTCOME_EXPORTS="frp_nmpc_outcome.h",
                 FSM_EXPORTS="frp_nmpc_fsm.h", VEHICLE_EXPORTS="frp_nmpc_vehicle.h", ESTIMATOR_EXPORTS="frp_nmpc_estimator.h")
    assert set(views.values()) == set(order) == set(HEADERS)
    for view, h in views.items():
        assert getattr(capi, view) == order[h] and getattr(solver, view) is getattr(capi, view), view
    lib = solver.lib()
    for name, (restype, argtypes) in capi.SIGNATURES.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name


def test_every_mirrored_macro_has_the_headers_value(tmp_path):
    assert len(capi.MACROS) >= 60 and capi.FRP_ERR_ARG == -1003 and capi.FRP_ERR_NO_DEVICE == -1001
    asserts = []
    for name, macro in capi.MACROS.items():
        value = getattr(capi, name)
        assert type(value) is int and getattr(solver, name) == value, name
        asserts.append(f"{macro} == {value}")
    _compile(tmp_path, "macros", "frp_nmpc.h", asserts)
    text = {h: open(os.path.join(INC, h)).read() for h in HEADERS}
    by_own = {}
    for name, macro in capi.MACROS.items():                             # ... and through the one header that defines it
        own = [h for h in HEADERS if re.search(rf"#define {macro}\b", text[h])]
        assert len(own) == 1, (macro, own)
        by_own.setdefault(own[0], []).append(f"{macro} == {getattr(capi, name)}")
    for i, h in enumerate(sorted(by_own)):
        _compile(tmp_path, f"macros{i}", h, by_own[h])


# what `solver` exposed before it became a facade: sorted(n for n in vars(solver) if not n.startswith("__")) without the imported modules
FACADE = """ABI_VERSION ASTAR_MAX_PATH ASTAR_NO_PATH ASTAR_REACH_END ASTAR_REACH_END_BUT_SHOT_FAILS ASTAR_REACH_HORIZON Astar AstarPlanner Batch CHECK_EXPORTS
CMD_INIT_POSITION CMD_PUB_END CMD_PUB_TRAJ CMD_ROTATE_YAW CMD_WAIT COMMAND_DEFAULTS COMMAND_END COMMAND_EXPORTS COMMAND_NONE COMMAND_NO_YAW_INPUT
COMMAND_STRIDE COMMAND_TRAJ COMMAND_YAW CORRIDOR_DEFAULTS CORRIDOR_LARGE_GROUPS CORRIDOR_LARGE_LIST CORRIDOR_LARGE_MAX_POINTS CORRIDOR_MAX_CELLS
CORRIDOR_MAX_F CORRIDOR_MAX_POINTS CloudGrid Command Commands Corridor CorridorCut CorridorLarge DISTANCE_EXPORTS DeviceFleet DeviceSolver
DistanceField ESTIMATOR_DEFAULTS ESTIMATOR_EXPORTS EST_ABSORBED EST_FIRST EST_SKIPPED EXPORTS EXTFUNC EstimatorArgs FSM_EXEC_PERIOD FSM_EXEC_TRAJ
FSM_EXPORTS FSM_EXT_NOISE_BOUND FSM_GEN_NEW_TRAJ FSM_INIT FSM_INIT_YAW FSM_REPLAN_TRAJ FSM_WAIT_TARGET FUSE_BATCH_EXPORTS FUSE_EXPORTS
FUSE_POINTS_EXPORTS FleetFSM FlightClearance ForceEstimator ForcesInfo ForcesOutput ForcesParams Fsm FsmExecIn INFO_STRIDE LARGE_EXPORTS LIB_PATH
LocalView OCCMAP_BODY OCCMAP_DEFAULTS OCCMAP_DIST_DEFAULT_R OCCMAP_DIST_FAR OCCMAP_DIST_MAX_R OCCMAP_FUSE_DEFAULTS OCCMAP_FUSE_DEFAULT_ROUNDS
OCCMAP_FUSE_MAX_FRAMES OCCMAP_FUSE_POINTS_MAX_SCANS OCCMAP_FUSE_POINTS_PARAMS OCCMAP_FUSE_REFUSED OCCMAP_VIEW_LAUNCHES OCCMAP_VIEW_MAX_GROUPS
ODOM_BODY ODOM_WORLD OUTCOME_EXPORTS OccMap OccMapBody OccMapFuse OccMapFuseBatch OccMapFusePoints OccMapRender OccMapRenderScan OccMapSharedView
OccMapView OccupancyMap Options Pack REFERENCE_PI RENDER_EXPORTS RENDER_SCAN_EXPORTS Reference SAFETY_INFLATE_CHECK SAFETY_INFLATE_SEARCH SafetyCheck
SharedView SharedViewGrid TICK_AT_END TICK_ENDING TICK_IDLE TICK_RESULT_IDLE TICK_RUN TUBE_DEFAULTS Tick TickIn TickState Tube VEHICLE_DEFAULTS
VEHICLE_EXPORTS VEHICLE_HOLD_STRIDE VEHICLE_MAX_SUB VEHICLE_MSG_STRIDE VEHICLE_SAT_PITCH VEHICLE_SAT_RATE0 VEHICLE_SAT_ROLL VEHICLE_SAT_THRUST_HI
VEHICLE_SAT_THRUST_LO VEHICLE_SAT_YAW_WRAP VEHICLE_SAT_ZERO_ACC VEHICLE_STATE VIEW_EXPORTS Vehicle VehicleArgs _PKG _check _lib _registered c_double_p
c_int_p command_batch_device command_snapshot_device corridor_batch_device corridor_batch_host default_options goal_search_table host_register
host_unregister host_unregister_all kernel_timing_begin kernel_timing_end lib lidar_beams reference_batch_device reference_batch_host solve_batch_host
solve_batch_host_begin solve_batch_host_wait solver_variant stage_eval_host tube_batch_device tube_batch_host""".split()


def test_solver_is_the_whole_facade():
    assert len(FACADE) == 163 == len(set(FACADE))
    homes = {m.__name__: m for m in (capi, batch, occmap, planning, fleet, flight)}
    for name in FACADE:
        assert hasattr(solver, name), name
        obj = getattr(solver, name)
        if inspect.isclass(obj) or inspect.isfunction(obj):
            home = homes.get(obj.__module__, capi)      # (EXTFUNC is a class ctypes made: capi holds it)
            assert getattr(home, name) is obj, name
    assert solver._registered is batch._registered and solver.lib is capi.lib and solver._check is capi._check
    # the direction of the imports: no module names a later one
    later = ["capi", "batch", "occmap", "planning", "fleet", "flight", "solver"]
    pkg = os.path.dirname(capi.__file__)
    for i, m in enumerate(later[:-1]):
        src = open(os.path.join(pkg, m + ".py")).read()
        for n in later[i:]:
            assert not re.search(rf"(?m)^\s*(from \.{n} import|from \. import .*\b{n}\b|import .*\b{n}\b)", src), (m, n)
    src = open(os.path.join(pkg, "capi.py")).read()
    assert not re.search(r"(?m)^(import torch|from torch)", src) and re.findall(r"(?m)^from \.(\w*) import|^from \. import (\w+)", src) in ([], [("", "layout")])
    assert "import *" not in open(os.path.join(pkg, "solver.py")).read()
