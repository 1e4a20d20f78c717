"""CPU checks of the wall-clock budget's interface (include/frp_nmpc.h: frp_nmpc_options.timeout, FRP_EXIT_TIMEOUT,
FRP_EXIT_INVALID_TIMEOUT): values, layout and defaults, no device needed."""
import ctypes
import os
import re
import subprocess

from forces_resilient_planner_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "frp_nmpc.h")


def test_exit_codes_are_the_references():
    """TIMEOUT_FORCESNLPsolver_normal (2) and INVALID_TIMEOUT_FORCESNLPsolver_normal (-12): FORCESNLPsolver_normal.h:118 and :136."""
    hdr = open(HDR).read()
    assert int(re.search(r"#define FRP_EXIT_TIMEOUT (-?\d+)", hdr).group(1)) == 2
    assert int(re.search(r"#define FRP_EXIT_INVALID_TIMEOUT \((-?\d+)\)", hdr).group(1)) == -12


def test_abi_version_seven_accepts_the_new_options():
    lib = solver.lib()
    hdr = open(HDR).read()
    assert int(re.search(r"#define FRP_NMPC_ABI_VERSION (\d+)", hdr).group(1)) == 7 == solver.ABI_VERSION == lib.frp_nmpc_abi_version()
    so, sb = ctypes.sizeof(solver.Options), ctypes.sizeof(solver.Batch)
    assert lib.frp_nmpc_abi_check(7, so, sb, solver.INFO_STRIDE) == 0
    assert lib.frp_nmpc_abi_check(7, so - 8, sb, solver.INFO_STRIDE) != 0  # (the ABI 6 options struct)


def test_timeout_offset_matches_the_c_compiler(tmp_path):
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "frp_nmpc.h"\n'
                   'int main(void) { printf("%zu %zu\\n", offsetof(frp_nmpc_options, timeout), sizeof(frp_nmpc_options)); return 0; }\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    off, size = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert solver.Options.timeout.offset == off and ctypes.sizeof(solver.Options) == size


def test_default_is_no_budget():
    assert solver.default_options().timeout == 0.0
    assert solver.default_options(timeout=0.5).timeout == 0.5
