"""The staging copies of the host-buffer batch (csrc/frp_copy_pool.hpp) on the CPU: tests/cpp/copy_pool_harness.cpp, a stand-alone
program, built once with the thread sanitizer and once with the address + undefined-behaviour sanitizers, and run.  The header is plain
C++17 without HIP, so neither build needs the GPU toolchain, and nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_copy_pool_matches_plain_loops_under_the_thread_and_address_sanitizers(tmp_path):
    """copy and pack_rows against plain loops: both sides of the 1 MiB and 4096-row thresholds, sizes that are no multiple of a slice
    (1 MiB + 8 bytes, 4097 and 12 289 rows), (M, MF) = (30, 6), (30, 0), (7, 7), from two caller threads in turn: 2 x (6 + 15) calls.
    A sanitizer report makes the program exit non-zero (-fno-sanitize-recover for the undefined-behaviour checks, which otherwise go on)."""
    src = os.path.join(ROOT, "tests", "cpp", "copy_pool_harness.cpp")
    for name, san in (("tsan", "-fsanitize=thread"), ("asan", "-fsanitize=address,undefined")):
        exe = str(tmp_path / ("copy_pool_" + name))
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", san, "-fno-sanitize-recover=all", src, "-o", exe, "-lpthread"])
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.split() == ["ok", "42"] and "Sanitizer" not in r.stderr, (name, r.stdout, r.stderr)
