"""CPU test (no GPU) of the index arithmetic every resize of the library shares, fovvideovdp_amd/csrc/resize_axis.hpp, against the
restatement of tests/resize_axis_check.cpp: ATen's `area` windows in 64-bit integers, the index ranges of the other modes, and the
reach the adjoint's candidate ranges are built from -- at the sizes of the resize tests, at the pairs beyond 2^24 where a float32
window leaves ATen's, at the largest sizes the entry points take, and on a fixed-seed sample.  The program is compiled for the host
alone, with the address and undefined-behaviour sanitizers, and runs as a child process: nothing sanitized is loaded into this
one."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_cases as rc                              # noqa: E402
from test_ingest_host_cpu import host_compiler         # noqa: E402


def test_axis_functions_against_restatement(tmp_path):
    exe = str(tmp_path / "resize_axis_check")
    cmd = host_compiler() + ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                             "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "fovvideovdp_amd", "csrc"),
                             "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "resize_axis_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    # every per-axis pair of the resize tests' sources and targets
    pairs = sorted({(s[k], t[k]) for s in rc.SOURCES for t in rc.TARGETS for k in range(2)})
    assert len(pairs) == 18 and all(a != b for a, b in pairs)
    ran = subprocess.run([exe] + ["%d:%d" % p for p in pairs], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    # both directions of: the 18 pairs above, the 9 named pairs (and 32768 -> 32768 once), the 300 sampled pairs
    assert ran.stdout.strip() == "resize_axis: %d cases pass" % (2 * 18 + 2 * 9 + 1 + 2 * 300)
