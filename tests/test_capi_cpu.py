"""CPU tests of the boundary: the C-ABI library loads and exports every symbol include/frp_nmpc.h declares,
the drop-in structs have the reference's sizes, the host-side adapter mirrors pack identically in Python
and C++, and -- with no GPU -- every compute entry point fails loudly instead of falling back."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from forces_resilient_planner_amd import adapter, layout as L, solver, workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _has_gpu():
    try:
        return solver.lib().frp_nmpc_device_count() > 0
    except Exception:
        return False


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(frp_nmpc_\w+|FORCESNLPsolver_\w+_solve)\s*\(", hdr))
    declared -= {"frp_nmpc_options", "frp_nmpc_batch"}
    assert {"FORCESNLPsolver_normal_solve", "FORCESNLPsolver_final_solve", "frp_nmpc_solve_batch"} <= declared
    lib = solver.lib()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/frp_nmpc.h but not exported"
    assert set(solver.EXPORTS) <= declared
    assert b"gfx950" in lib.frp_nmpc_version()


def test_dropin_struct_layouts_match_reference_sizes():
    # FORCESNLPsolver_normal.h:153-301 ([probed] sizes in SURVEY 8b): params 23600, output 2720, info 136
    assert ctypes.sizeof(solver.ForcesParams) == 23600
    assert solver.ForcesParams.x0.offset == 72 and solver.ForcesParams.all_parameters.offset == 2792
    assert solver.ForcesParams.num_of_threads.offset == 23592
    assert ctypes.sizeof(solver.ForcesOutput) == 2720
    assert ctypes.sizeof(solver.ForcesInfo) == 136
    assert solver.ForcesInfo.res_eq.offset == 8 and solver.ForcesInfo.solvetime.offset == 120


REFERENCE_ABI = os.path.join(ROOT, "tests", "golden", "reference_abi.json")
OWN = {"params": "frp_forces_params", "output": "frp_forces_output", "info": "frp_forces_info"}
OWN_EXIT = {"OPTIMAL": "FRP_EXIT_OPTIMAL", "MAXITREACHED": "FRP_EXIT_MAXIT", "FACTORIZATION_ERROR": "FRP_EXIT_FACTORIZATION",
            "BADFUNCEVAL": "FRP_EXIT_BADFUNCEVAL", "NOPROGRESS": "FRP_EXIT_NOPROGRESS", "PARAM_VALUE_ERROR": "FRP_EXIT_PARAM_VALUE"}


@pytest.mark.parametrize("m", ["normal", "final"])
def test_dropin_matches_the_references_own_header(m, tmp_path):
    """Against the header plan_manage compiles with (FORCESNLPsolver_normal.h:153-323, included by forces_normal.cpp:2-3), as
    recorded in tests/golden/reference_abi.json (tests/tools/gen_reference_abi.py: what a compiler sees in it): one translation
    unit compares every struct field, the callback type, the solve prototype and the exit codes of include/frp_nmpc.h with the
    recorded ones, and then links the reference's symbol against libfrp_nmpc_amd.so."""
    import json
    ref = json.load(open(REFERENCE_ABI))["models"][m]
    R = f"FORCESNLPsolver_{m}"
    asserts = []
    for s, own in OWN.items():
        asserts.append(f'static_assert(sizeof({own}) == {ref[s]["size"]}, "{s}");')
        for f, (off, size) in ref[s]["fields"].items():
            if s == "output":  # x01 .. x20: the rows of this header's one array
                k = int(f[1:]) - 1
                asserts.append(f"static_assert(offsetof({own}, x) + {k} * sizeof(((({own} *)0)->x[0])) == {off} && sizeof((({own} *)0)->x[{k}]) == {size}, \"{f}\");")
            else:
                asserts.append(f"static_assert(offsetof({own}, {f}) == {off} && sizeof((({own} *)0)->{f}) == {size}, \"{f}\");")
    # exit codes the caller distinguishes (nmpc_solver.cpp:398-421); "no usable device" is reported with the reference's own
    # "solver not valid on this machine" value; the runtime-fault code is outside the reference's set
    codes = ref["exit_codes"]
    asserts += [f'static_assert({own} == {codes[c]}, "{c}");' for c, own in OWN_EXIT.items()]
    asserts.append(f'static_assert(FRP_EXIT_NO_DEVICE == {codes["LICENSE_ERROR"]} && FRP_EXIT_DEVICE_FAULT < {codes["LICENSE_ERROR"]}, "machine-level codes");')
    asserts.append(f'static_assert(std::is_same<frp_forces_extfunc, {ref["extfunc"]}>::value, "callback type");')
    asserts.append(f'static_assert(std::is_same<decltype(&{R}_solve), {ref["solve"].replace("{solver}_", "frp_forces_")}>::value, "reference prototype");')
    src = tmp_path / "hdr.cpp"
    src.write_text("""
#include "frp_nmpc.h"
#include <cstddef>
#include <cstdio>
#include <type_traits>
""" + "\n".join(asserts) + f"""
int main() {{
    // the reference's symbol resolved by this repo's library, exactly what plan_manage's link step does
    auto solve = &{R}_solve;
    return solve ? 0 : 1;
}}
""")
    exe = tmp_path / "hdr"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
           "-L" + os.path.dirname(solver.LIB_PATH), "-l:" + os.path.basename(solver.LIB_PATH), "-Wl,-rpath," + os.path.dirname(solver.LIB_PATH),
           "-Wl,--unresolved-symbols=ignore-in-shared-libs", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert len(asserts) == 3 + 4 + 3 + 19 + 6 + 1 + 2


def test_abi_check_rejects_a_caller_built_against_another_header():
    """FRP_INFO_STRIDE went 8 -> 12 and frp_nmpc_options grew with only the version string bumped.  The header now
    carries FRP_NMPC_ABI_VERSION; frp_nmpc_abi_check compares version, struct sizes and info stride with the library's own,
    the Python loader and the C++ adapter call it before anything else."""
    import ctypes, re
    lib = solver.lib()
    hdr = open(os.path.join(ROOT, "include", "frp_nmpc.h")).read()
    ver = int(re.search(r"#define FRP_NMPC_ABI_VERSION (\d+)", hdr).group(1))
    stride = int(re.search(r"#define FRP_INFO_STRIDE (\d+)", hdr).group(1))
    assert lib.frp_nmpc_abi_version() == ver == solver.ABI_VERSION and stride == solver.INFO_STRIDE
    so, sb = ctypes.sizeof(solver.Options), ctypes.sizeof(solver.Batch)
    assert lib.frp_nmpc_abi_check(ver, so, sb, stride) == 0
    for bad in ((ver - 1, so, sb, stride), (ver, so - 8, sb, stride), (ver, so, sb + 8, stride), (ver, so, sb, 8)):
        assert lib.frp_nmpc_abi_check(*bad) == -1003  # FRP_ERR_ARG


def test_workspace_size_formula():
    """The solver keeps its per-iteration state in LDS and registers: the device workspace is the work queue (counter 256 B,
    per-CU counters 8 KB, one key and one order entry per problem = 12 B per problem), whatever the horizon and the face
    count -- plus, for the launches the four-per-CU variants take (N <= 20, at most 6 corridor rows), the packed Riccati
    blocks S_xx of the RESIDENT workgroups (20 x 48 doubles each, at most four per CU; 128 bytes of alignment slack) and, for the launches
    the three-per-CU variant of round 6 takes (20 < N <= 30, at most 16 rows), 30 x 48 doubles for at most three workgroups per CU: bounded by
    the chip, not by B."""
    lib = solver.lib()
    ws = lib.frp_nmpc_workspace_bytes
    queue = lambda B: 8 * (32 + 1024 + B + (B + 1) // 2)
    slot = 8 * 20 * 48  # S_xx of 20 stages: 48 doubles each
    cap = (ws(10 ** 6, 20, 6) - queue(10 ** 6) - 128) // slot
    assert cap % 4 == 0 and 4 <= cap <= 4 * 1024  # four workgroups per CU (256 CUs assumed without a device)
    slot30 = 8 * 30 * 48
    cap30 = (ws(10 ** 6, 30, 15) - queue(10 ** 6) - 128) // slot30
    assert cap30 % 3 == 0 and cap30 * 4 == cap * 3
    for B in (1, 7, 4096, 10 ** 6):
        assert ws(B, 64, 30) == ws(B, 20, 7) == ws(B, 31, 6) == ws(B, 30, 17) == queue(B)
        assert ws(B, 20, 6) == queue(B) + 128 + min(B, cap) * slot
        assert ws(B, 21, 6) == ws(B, 30, 16) == queue(B) + 128 + min(B, cap30) * slot30


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_no_device_means_loud_failure_not_cpu_fallback():
    w = workloads.config2(2)
    with pytest.raises(RuntimeError):
        solver.solve_batch_host(w)
    w0 = workloads.config0()
    p = solver.ForcesParams(); o = solver.ForcesOutput(); info = solver.ForcesInfo()
    p.xinit[:] = w0["xinit"][0]; p.x0[:] = w0["x0"][0].ravel(); p.all_parameters[:] = w0["params"][0].ravel()
    flag = solver.lib().FORCESNLPsolver_normal_solve(ctypes.byref(p), ctypes.byref(o), ctypes.byref(info), None, None)
    assert flag == -100  # FRP_EXIT_NO_DEVICE = the reference's "solver not valid on this machine", not PARAM_VALUE
    assert np.all(np.array(o.x) == 0.0)


def _harness():
    exe = os.path.join(ROOT, "tests", "cpp", "adapter_harness")
    src = exe + ".cpp"
    # (rebuilt whenever the source, the C-ABI header, the C++ adapter or the library is newer: the harness sizes its buffers from the
    # header's constants -- a binary built against an older FRP_INFO_STRIDE corrupts its heap)
    deps = [src, os.path.join(ROOT, "include", "frp_nmpc.h"), os.path.join(ROOT, "forces_resilient_planner_amd", "csrc", "frp_adapter.hpp"), solver.LIB_PATH]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps if os.path.exists(d)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", src, "-o", exe, "-L" + os.path.dirname(solver.LIB_PATH),
                               "-lfrp_nmpc_amd", "-Wl,-rpath," + os.path.dirname(solver.LIB_PATH),
                               "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _write_harness_input(path, w, weights, F):
    B, N = w["B"], w["N"]
    with open(path, "wb") as f:
        np.array([B, N, F, w["model"]], dtype=np.int32).tofile(f)
        np.asarray(weights, dtype=np.float64).tofile(f)
        for key in ("mpc_output", "f_ext", "ref_pos", "ref_yaw", "E", "poly_A", "poly_b"):
            np.ascontiguousarray(w[key], dtype=np.float64).tofile(f)
        np.ascontiguousarray(w["nfaces"], dtype=np.int32).tofile(f)


def test_cpp_adapter_packs_exactly_like_python_adapter(tmp_path):
    """G2 packing vectors: forces_normal.cpp:62-136 restated twice (numpy, C++) must agree bit for bit,
    including the robust tightening b - ||E a||, zero padding and the 30-row truncation."""
    w = workloads.config2(5)
    rng = np.random.default_rng(3)
    # make it harder: 33 faces on some stages (the reference silently drops rows >= 30), ragged counts
    B, N = 5, w["N"]
    F = 33
    A = rng.normal(size=(B, N, F, 3)); b = rng.uniform(1, 3, size=(B, N, F))
    nf = rng.integers(0, F + 1, size=(B, N)).astype(np.int32)
    w = dict(w, poly_A=A, poly_b=b, nfaces=nf)
    weights = (7.0, 1.0, 80.0, 12.0, 0.5)
    ad = adapter.ForcesAdapter(B, w["model"], N, 30)
    ad.set_paras(*weights)
    xinit, x0, params, nfo = ad.pack(w["mpc_output"], w["f_ext"], w["ref_pos"], w["ref_yaw"], w["E"], A, b, nf)
    inp = tmp_path / "in.bin"; out = tmp_path / "out.bin"
    _write_harness_input(inp, w, weights, F)
    subprocess.check_call([_harness(), "pack", str(inp), str(out)])
    raw = np.fromfile(out, dtype=np.uint8)
    nd = B * 9 + B * N * 17 + B * N * 130
    d = raw[:nd * 8].view(np.float64); ni = raw[nd * 8:].view(np.int32)
    assert np.array_equal(d[:B * 9], xinit.ravel())
    assert np.array_equal(d[B * 9:B * 9 + B * N * 17], x0.ravel())
    pc = d[B * 9 + B * N * 17:]
    assert np.array_equal(pc == 0, params.ravel() == 0)            # same padding pattern
    assert np.max(np.abs(pc - params.ravel())) <= 4e-16 * 4        # b - ||E a||: summation order only
    assert np.array_equal(ni, nfo.ravel())
    assert nfo.max() == 30  # truncated
    # padded rows are exactly zero, live rows carry the tightened offsets
    p = params.reshape(B, N, 130)
    for bb in range(B):
        for k in range(N):
            m = nfo[bb, k]
            assert np.all(p[bb, k, 10 + 3 * m:100] == 0) and np.all(p[bb, k, 100 + m:] == 0)
            if m:
                Ea = w["E"][bb, k] @ A[bb, k, 0]
                assert abs(p[bb, k, 100] - (b[bb, k, 0] - np.linalg.norm(Ea))) < 1e-15


def test_adapter_shift_warm_start_and_yaw_wrap():
    st = np.array([[0.1, 0.2, 1.0, 0, 0, 0, 0, 0, 0.3]])
    mpc = adapter.init_mpc_output(st, 20)
    assert mpc.shape == (1, 21, 17) and np.all(mpc[0, :, 3] == 7.3) and np.all(mpc[0, :, 7] == 7.3)
    mpc[0, :, 16] = np.linspace(-4, 4, 21)
    mpc[0, :, 0] = np.arange(21)
    ad = adapter.ForcesAdapter(1)
    A = np.zeros((1, 20, 1, 3)); b = np.zeros((1, 20, 1)); nf = np.zeros((1, 20), np.int32)
    xinit, x0, params, _ = ad.pack(mpc, np.zeros((1, 3)), np.zeros((1, 20, 3)), np.zeros((1, 20)), np.zeros((1, 20, 3, 3)), A, b, nf)
    assert np.array_equal(x0[0, :, 0], np.arange(1, 21))          # stage i <- previous plan stage i+1
    assert np.array_equal(xinit[0], mpc[0, 1, 8:17])                # NOT row 0 / odometry (forces_normal.cpp:62-72)
    out = adapter.update_forces_results(mpc.copy())
    assert np.all(np.abs(out[0, :20, 16]) <= np.pi + 1e-12)
    assert np.array_equal(out[0, 20], out[0, 19])


def test_workloads_are_seeded_and_well_formed():
    a = workloads.config2(16); b = workloads.config2(16)
    assert np.array_equal(a["params"], b["params"]) and np.array_equal(a["xinit"], b["xinit"])
    assert a["params"].shape == (16, 20, 130) and a["nfaces"].min() == 6 == a["nfaces"].max()
    c = workloads.config3(8)
    assert c["N"] == 30 and c["M"] == 15 and c["params"].shape == (8, 30, 70) and c["nfaces"].max() <= 15
    # the stage reference point is strictly inside its tightened polytope
    p = c["params"]
    for bb in range(8):
        for k in range(30):
            m = c["nfaces"][bb, k]
            A = p[bb, k, 10:10 + 3 * m].reshape(m, 3); bt = p[bb, k, 10 + 45:10 + 45 + m]
            assert np.all(A @ c["ref_pos"][bb, k] < bt)
    d = workloads.config1(4)
    assert d["nfaces"].max() == 0 and np.all(d["params"][:, :, 10:] == 0)


def test_lds_kernel_has_no_spill_behind_a_lane_divergent_loop(tmp_path):
    """Compiler-hazard guard.  The gfx950 backend may place a VGPR spill at the exit of a lane-divergent loop, where the
    EXEC mask is empty, so the spill saves nothing and the later reload returns whatever the scratch slot held (this
    crashed a solve of the round-1 kernel through a reloaded zero offset).  The solver kernel (frp_ipm_lds.hip) has one
    lane-divergent loop (the padding-row detection): it is a function of its own and must use no scratch."""
    import re
    import subprocess
    from forces_resilient_planner_amd import build
    src = os.path.join(build.CSRC, "frp_ipm_lds.hip")
    out = tmp_path / "lds.s"
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only"] + build.PER_SOURCE_FLAGS["frp_ipm_lds.hip"] + [
                           "-I" + os.path.join(build.ROOT, "include"), src, "-o", str(out)], stderr=subprocess.DEVNULL)
    txt = out.read_text()
    scratch = {name: int(sz) for name, sz in re.findall(r"^(_ZN3frp\w+):.*?^; ScratchSize: (\d+)", txt, flags=re.M | re.S)}
    det = [n for n in scratch if "count_live_faces" in n]
    assert len(det) == 1 and scratch[det[0]] == 0, scratch
    # (every other loop of that file runs over the wave-uniform horizon length or a compile-time face count: the kernel
    # bodies, which do use scratch, contain no per-lane trip count)
    assert len([n for n in scratch if "nmpc_ipm_lds_kernel" in n]) >= 5  # (the main translation unit: the five FREG variants)
    _check_asm_lds_loads_land_before_edges(txt)


def _check_asm_lds_loads_land_before_edges(txt):
    """The vector sweeps issue their LDS loads through inline asm and wait for them with hand-counted s_waitcnt: the
    compiler believes a loaded register is valid at once.  Invariant that keeps this safe (frp_ipm_lds.hip, "the two
    vector sweeps"): between a ds_read of the sweeps and the s_waitcnt that retires it, no instruction reads the
    destination registers, and no label / branch is crossed (the register allocator may copy values on an edge).  Checked
    on the generated code: a linear scan per function with the set of registers whose load is in flight."""
    import re

    def regs(tok):
        m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
        if m:
            return set(range(int(m.group(1)), int(m.group(2)) + 1))
        m = re.fullmatch(r"v(\d+)", tok)
        return {int(m.group(1))} if m else set()

    checked = 0
    for fn in ("sweep_forward", "sweep_backvec"):
        m = re.search(r"^(_ZN3frp2lr\d+%s\w*):\s" % fn, txt, flags=re.M)
        assert m, fn
        body = txt[m.end():]
        body = body[:body.index("s_setpc_b64")]
        inflight = set()
        in_asm = False
        for line in body.splitlines():
            if "#ASMSTART" in line or "#ASMEND" in line:  # (the compiler's own LDS loads are waited for by the compiler)
                in_asm = "#ASMSTART" in line
                continue
            line = line.split(";")[0].strip()
            if not line or line.startswith("."):
                if line.startswith(".LBB"):
                    assert not inflight, (fn, "label reached with loads in flight", line, sorted(inflight))
                continue
            op, _, rest = line.partition(" ")
            toks = [t.strip() for t in rest.replace(" offset", ", offset").split(",")]
            if op == "s_waitcnt":
                m2 = re.search(r"lgkmcnt\((\d+)\)", rest)
                if m2 and int(m2.group(1)) <= 2:  # at most the two stores of the running step stay outstanding
                    inflight.clear()
                continue
            if op.startswith("s_cbranch") or op in ("s_branch", "s_setpc_b64", "s_swappc_b64"):
                assert not inflight, (fn, "branch with loads in flight", line, sorted(inflight))
                continue
            if op == "ds_read_b64" and in_asm:
                dst = regs(toks[0])
                src = set().union(*[regs(t) for t in toks[1:]])
                assert not (src & inflight), (fn, line)
                inflight |= dst
                checked += 1
                continue
            used = set().union(*[regs(t) for t in toks]) if toks else set()
            assert not (used & inflight), (fn, "register of a load in flight touched", line, sorted(used & inflight))
    assert checked > 100


def test_header_is_plain_c99(tmp_path):
    """The boundary is a C ABI: include/frp_nmpc.h must compile as strict C99 on its own (no C++, no torch types)."""
    import subprocess
    src = tmp_path / "hdr.c"
    src.write_text('#include "frp_nmpc.h"\n'
                   'int main(void) { frp_nmpc_batch b; frp_nmpc_pack p; frp_nmpc_tube t; frp_nmpc_corridor c; frp_nmpc_reference r;\n'
                   '  frp_forces_params fp; (void)b; (void)p; (void)t; (void)c; (void)r; (void)fp;\n'
                   '  return sizeof(frp_forces_params) == 23600 ? 0 : 1; }\n')
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", inc, "-fsyntax-only", str(src)])


def test_python_mirrors_of_the_c_structs_have_the_headers_layout(tmp_path):
    """solver.py drives the C-ABI through ctypes mirrors of the header's structs: their sizes, and the offsets of the fields that were
    appended last, must be the compiler's (a field added to the header only would shift every argument behind it silently)."""
    import subprocess
    pairs = [("frp_nmpc_options", solver.Options, "twist"), ("frp_nmpc_batch", solver.Batch, "order_hint"), ("frp_nmpc_astar", solver.Astar, "retry_vel"),
             ("frp_nmpc_pack", solver.Pack, None), ("frp_nmpc_tube", solver.Tube, None), ("frp_nmpc_corridor", solver.Corridor, None),
             ("frp_nmpc_reference", solver.Reference, None),
             ("frp_forces_params", solver.ForcesParams, "num_of_threads"), ("frp_forces_info", solver.ForcesInfo, None), ("frp_forces_output", solver.ForcesOutput, None)]
    src = tmp_path / "layout.c"
    body = "".join(f'  printf("%zu %zu\\n", sizeof({c}), {("offsetof(" + c + ", " + f + ")") if f else "(size_t)0"});\n' for c, _, f in pairs)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "frp_nmpc.h"\nint main(void) {\n' + body + '  return 0; }\n')
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", inc, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    for i, (cname, py, field) in enumerate(pairs):
        size, off = int(out[2 * i]), int(out[2 * i + 1])
        assert ctypes.sizeof(py) == size, (cname, ctypes.sizeof(py), size)
        if field:
            assert getattr(py, field).offset == off, (cname, field, getattr(py, field).offset, off)


def test_widened_entry_points_reject_bad_arguments_before_touching_a_device():
    """Argument checks of the f-1 .. f-4 entry points run on the host, so they are testable without a GPU: NULL
    buffers, horizons beyond 64 stages, polytope capacities outside [6, 64], oversized clouds / grids, non-positive
    physical constants all return FRP_ERR_ARG (-1003)."""
    l = solver.lib()
    ERR = -1003
    one = ctypes.c_void_p(8)  # any non-NULL address: the checks must fail before it would be dereferenced on the device
    tb = solver.Tube(4, 20, None, 0.74, 0.33, 0.27, 0.0425, (ctypes.c_double * 3)(0.5, 0.5, 0.5), 0.06, 0.05, one)
    assert l.frp_nmpc_tube_batch(ctypes.byref(tb), None) == ERR                 # no plan
    tb.mpc_output = 8; tb.N = 65
    assert l.frp_nmpc_tube_batch(ctypes.byref(tb), None) == ERR                 # horizon > 64
    tb.N = 20; tb.mass = 0.0
    assert l.frp_nmpc_tube_batch(ctypes.byref(tb), None) == ERR                 # mass
    tb.mass = 0.74; tb.noise = (ctypes.c_double * 3)(0.5, 0.0, 0.5)
    assert l.frp_nmpc_tube_batch(ctypes.byref(tb), None) == ERR                 # a zero noise bound makes tr(X) = 0
    cr = solver.Corridor()
    cr.B, cr.N, cr.F, cr.P = 4, 20, 64, 100
    for f in ("cloud", "ref_pos", "ref_yaw", "ellipsoid", "poly_A", "poly_b", "poly_nfaces", "poly_index"):
        setattr(cr, f, 8)
    cr.bbox = (ctypes.c_double * 3)(2, 2, 1); cr.seed_len = 0.1; cr.inflation = 1.1
    for field, bad in (("F", 5), ("F", 65), ("N", 0), ("N", 65), ("P", 65537), ("seed_len", 0.0), ("poly_index", None), ("cloud", None)):
        keep = getattr(cr, field)
        setattr(cr, field, bad)
        assert l.frp_nmpc_corridor_batch(ctypes.byref(cr), None) == ERR, field
        setattr(cr, field, keep)
    cr.grid_start = 8                                                            # a grid without its other arrays / cell size
    assert l.frp_nmpc_corridor_batch(ctypes.byref(cr), None) == ERR
    rf = solver.Reference(4, 20, 50, None, 0, None, 8, 8, 0.05, 3.1415926, 8, 8, None)
    assert l.frp_nmpc_reference_batch(ctypes.byref(rf), None) == ERR           # no path
    rf.kino_path = 8; rf.Ts = 0.0
    assert l.frp_nmpc_reference_batch(ctypes.byref(rf), None) == ERR
    rf.Ts = 0.05
    for field, bad in (("Ts", 0.0), ("Ts", -0.05), ("Ts", float("nan")), ("pi", 3.0), ("pi", 2.9), ("pi", float("nan")), ("N", 0), ("N", 65), ("K", 0),
                       ("B", 0), ("time_offset", None), ("mpc_output", None), ("ref_pos", None), ("ref_yaw", None)):
        keep = getattr(rf, field)
        setattr(rf, field, bad)
        assert l.frp_nmpc_reference_batch(ctypes.byref(rf), None) == ERR, (field, bad)
        setattr(rf, field, keep)
    assert l.frp_nmpc_reference_batch(None, None) == ERR
    mode_args = [4, 20, one, one, one, 0, one, 0, 0.05, 1.0, one, None]   # B, N, plan, time_offset, kino_size, per, end_pt, per, Ts, radius, mode, stream
    for at, bad in ((8, 0.0), (8, -0.05), (8, float("nan")), (0, 0), (1, 0), (2, None), (3, None), (4, None), (6, None), (10, None)):
        a = list(mode_args); a[at] = bad
        assert l.frp_nmpc_mode_batch(*a) == ERR, (at, bad)
    assert l.frp_nmpc_coldstart_batch(4, 20, None, None, 7.3, None, None) == ERR
    d3, i3 = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_int * 3)(1 << 11, 1 << 11, 2)   # 2^23 cells > FRP_CORRIDOR_MAX_CELLS
    assert l.frp_nmpc_cloud_grid_build(one, 10, d3, 0.5, i3, one, one, one, one, None) == ERR
    assert l.frp_nmpc_cloud_grid_build(one, 10, d3, 0.0, (ctypes.c_int * 3)(4, 4, 4), one, one, one, one, None) == ERR
    # the kernel-selection query: the batch checks of frp_nmpc_solve_batch, and a buffer that holds the name
    bt = solver.Batch(64, 20, 30, 6, 0, 8, 8, 8, None, 8, 8, 8, None, None)
    buf = ctypes.create_string_buffer(128)
    assert l.frp_nmpc_solver_variant(ctypes.byref(bt), None, None, 128) == ERR   # no buffer
    assert l.frp_nmpc_solver_variant(ctypes.byref(bt), None, buf, 0) == ERR      # empty buffer
    for field, bad in (("N", 65), ("N", 1), ("MF", 31), ("B", 0), ("model", 2), ("params", None)):
        keep = getattr(bt, field)
        setattr(bt, field, bad)
        assert l.frp_nmpc_solver_variant(ctypes.byref(bt), None, buf, 128) == ERR, field
        setattr(bt, field, keep)
    if not _has_gpu():  # (valid arguments: the choice needs the device's CU count -- a loud failure, no guess)
        assert l.frp_nmpc_solver_variant(ctypes.byref(bt), None, buf, 128) == -1001
        with pytest.raises(RuntimeError):
            solver.solver_variant(64, 20, 30, 6, 0)


def test_product_objects_hold_no_truncated_scalar_immediates(monkeypatch):
    """Guard against the miscompile behind round 2's "wrong objective" build: with -disable-machine-licm -disable-machine-cse alone
    this compiler emits s_mov_b64 with a 64-bit FP immediate, gfx9 encodes the low dword only, and 12.0 / 10.0 / 20.0 become 0.0
    (build.py has the whole story).  Every object of the product library is disassembled and checked; and the code-generation
    switches are dropped when hipcc is not the release they were checked on."""
    from forces_resilient_planner_amd import build
    build.build_native(force=False, verbose=False)
    checked = 0
    for n in build.SOURCES:
        obj = os.path.join(build.OBJDIR, n + ".o")
        if os.path.exists(obj):
            checked += build.check_device_code(obj)
    assert checked > 500
    import subprocess
    real = subprocess.run
    monkeypatch.setattr(build.subprocess, "run", lambda *a, **k: type("R", (), {"stdout": "HIP version: 9.9\nAMD clang version 99 (roc-9.9.0)", "returncode": 0})())
    assert not build.codegen_flags_trusted()
    monkeypatch.setattr(build.subprocess, "run", real)
    assert build.codegen_flags_trusted()


def _build_static_dropin_programs(tmp_path):
    """C++ programs linked, by plain g++, against static archives with the reference's file names (plan_manage/CMakeLists.txt:64-65,
    82-83) + the HIP runtime: tests/cpp/static_dropin_stub.cpp compiled against include/frp_nmpc.h (layout-identical to the
    reference's generated headers: test_dropin_matches_the_references_own_header) and, where the oracle recipe built it, the same
    program compiled against the REFERENCE's generated headers (oracle/_ref/static_dropin_stub.o)."""
    import subprocess
    from forces_resilient_planner_amd import build
    build.build_native(force=False, verbose=False)
    build.build_dropin_archives()
    src = os.path.join(ROOT, "tests", "cpp", "static_dropin_stub.cpp")
    rocm = "/opt/rocm/lib"
    link = ["-L" + build.DROPIN_DIR, "-l:libFORCESNLPsolver_normal.a", "-l:libFORCESNLPsolver_final.a", "-L" + rocm, "-lamdhip64", "-lpthread", "-Wl,-rpath," + rocm]
    objs = {"own_header": ["-O1", "-DFRP_STUB_OWN_HEADER", "-I" + os.path.join(ROOT, "include"), src]}
    ref_obj = os.path.join(ROOT, "oracle", "_ref", "static_dropin_stub.o")
    if os.path.exists(ref_obj):
        objs["reference_headers"] = [ref_obj]
    exes = []
    for name, inputs in objs.items():
        exe = tmp_path / ("planner_stub_" + name)
        r = subprocess.run(["g++", *inputs, *link, "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        exes.append(exe)
    return exes


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour of the statically linked stub")
def test_static_archives_with_the_references_file_names_link_and_fail_loudly_without_a_device(tmp_path):
    import subprocess
    for exe in _build_static_dropin_programs(tmp_path):
        r = subprocess.run([str(exe)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.split()[:2] == ["-100", "-100"], r.stdout + r.stderr


SOLVER_KERNEL = r"void (\S+::nmpc_ipm_lds_kernel<[^>]*>)\(frp::KernelArgs\) \(\.kd\)$"


def _kernel_instantiations(so, tmp_path, pattern=SOLVER_KERNEL):
    """Demangled names of the nmpc_ipm_lds_kernel instantiations (or of the kernels whose descriptor line matches another
    `pattern`, group 1 = the name) in the gfx950 code objects of a built library: every
    clang offload bundle of its .hip_fatbin section (one per translation unit) is unbundled here and its kernel descriptors
    listed, demangled, with the ROCm LLVM tools.  Returns {name: number of bundles that hold it}."""
    import struct
    llvm = "/opt/rocm/llvm/bin"
    fb = tmp_path / "fatbin"
    subprocess.run([f"{llvm}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", so, str(tmp_path / "discard")], check=True)
    data = fb.read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    names, bundles, pos = {}, 0, data.find(magic)
    while pos >= 0:
        n = struct.unpack_from("<Q", data, pos + 24)[0]
        off = pos + 32
        for _ in range(n):
            o, size, tl = struct.unpack_from("<QQQ", data, off)
            triple = data[off + 24:off + 24 + tl].decode()
            off += 24 + tl
            if "amdgcn" not in triple:
                continue
            assert "gfx950" in triple, triple
            co = tmp_path / f"co{bundles}.elf"
            co.write_bytes(data[pos + o:pos + o + size])
            syms = subprocess.run([f"{llvm}/llvm-readelf", "-s", "-C", "--wide", str(co)], check=True, capture_output=True, text=True).stdout
            kern = [re.search(pattern, ln) for ln in syms.splitlines()]
            kern = {m.group(1) for m in kern if m}  # (.dynsym and .symtab list each descriptor)
            for nm in kern:
                names[nm] = names.get(nm, 0) + 1
            bundles += bool(kern)
        pos = data.find(magic, pos + 1)
    return names, bundles


@pytest.mark.parametrize("lib", ["default", "default_flags"])
def test_step_parity_cases_cover_every_kernel_instantiation_that_ships(lib, tmp_path):
    """The case table of tests/test_gpu_variant_steps.py names exactly the nmpc_ipm_lds_kernel instantiations of the built
    library, read from its device code (five translation units): an instantiation added without a step-parity case, or
    a case whose instantiation is gone, fails here."""
    from forces_resilient_planner_amd import build
    from .test_gpu_variant_steps import CASES
    so = solver.LIB_PATH if lib == "default" else build.DEFAULT_FLAGS_LIB
    if not os.path.exists(so):
        build.build_native(force=False, verbose=False) if lib == "default" else build.build_default_flags_lib()
    names, bundles = _kernel_instantiations(so, tmp_path)
    assert bundles == 5, (bundles, names)
    assert all(c == 1 for c in names.values()), names
    assert set(names) == set(CASES), (sorted(set(names) - set(CASES)), sorted(set(CASES) - set(names)))


def test_slot_reuse_cases_cover_every_kernel_instantiation_that_ships(tmp_path):
    """The launches of tests/test_gpu_slot_reuse.py name exactly the nmpc_ipm_lds_kernel instantiations of the built library: a
    new variant cannot ship without a slot-reuse case."""
    from forces_resilient_planner_amd import build
    from .test_gpu_slot_reuse import LAUNCHES
    if not os.path.exists(solver.LIB_PATH):
        build.build_native(force=False, verbose=False)
    names, _ = _kernel_instantiations(solver.LIB_PATH, tmp_path)
    covered = {l[1] for l in LAUNCHES}
    assert set(names) == covered, (sorted(set(names) - covered), sorted(covered - set(names)))


def test_batch_fusion_stage_kernels_ship_once(tmp_path):
    """The seven stage kernels that depth frames and point scans share exist once in the built library, under
    frp::occmap::fuse::batch (frp_occmap_fuse_batch.hip); frp::occmap::fuse::points holds its own first stage alone.  Symbol names only."""
    from forces_resilient_planner_amd import build
    if not os.path.exists(solver.LIB_PATH):
        build.build_native(force=False, verbose=False)
    names, _ = _kernel_instantiations(solver.LIB_PATH, tmp_path, r"\s(?:void )?(frp::occmap::fuse::(?:batch|points)::\w+(?:<[^>]*>)?)\(.*\) \(\.kd\)$")
    assert all(c == 1 for c in names.values()), names
    stages = {"init", "setup", "mark", "stop", "status", "count", "update"}
    assert {n for n in names if "::batch::" in n} == {f"frp::occmap::fuse::batch::{k}_kernel" for k in stages | {"describe", "project"}}, names
    assert {n for n in names if "::points::" in n} == {"frp::occmap::fuse::points::describe_kernel", "frp::occmap::fuse::points::load_kernel<float>",
                                                       "frp::occmap::fuse::points::load_kernel<double>"}, names


def test_solver_sources_carry_no_experiment_knobs():
    """The solver kernel's experiments are frozen at the values that ship (profiles/solver_knob_freeze_identity.txt): the only FRP_*
    names its sources may test in the preprocessor are the unit selectors, the per-unit inline settings, the profile macros and the
    objective dump, and nothing is a default-define pair (#ifndef X / #define X) that a -D could override."""
    import glob
    from forces_resilient_planner_amd import build
    allowed = {"FRP_LDS_MEM_TU", "FRP_LDS_Q4_TU", "FRP_LDS_Q30_TU", "FRP_LDS_S2_TU",  # the unit selectors (none of them: the main unit)
               "FRP_LDS_TEMPLATES_ONLY",                                            # ... and the probe that wants no launcher
               "FRP_INLINE_FACTOR", "FRP_INLINE_SWEEPS",                            # set by the units' own files
               "FRP_PROFILE", "FRP_PROFILE_SEG", "FRP_PROFILE_W1", "FRP_DEBUG_OBJ"}  # tooling
    files = sorted(glob.glob(os.path.join(build.CSRC, "frp_ipm_lds*.hip")) + glob.glob(os.path.join(build.CSRC, "frp_ipm_lds*.inc")))
    assert len(files) >= 5, files
    tested, pairs = set(), []
    for f in files:
        lines = open(f).read().split("\n")
        for i, line in enumerate(lines):
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*)", line)
            if not m:
                continue
            cond = m.group(2).split("//")[0]
            tested |= set(re.findall(r"\bFRP_[A-Za-z0-9_]+", cond))
            d = re.match(r"\s*(\w+)", cond)
            nxt = next((l for l in lines[i + 1:] if l.strip()), "")
            if m.group(1) == "ifndef" and d and re.match(r"\s*#\s*define\s+" + re.escape(d.group(1)) + r"\b", nxt):
                pairs.append(f"{os.path.basename(f)}:{i + 1}: {d.group(1)}")
    assert tested == allowed, f"unexpected: {sorted(tested - allowed)}, missing: {sorted(allowed - tested)}"
    assert not pairs, pairs
