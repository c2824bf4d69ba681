"""CPU test (no GPU) of the host code the four clip backwards share for their temporal transpose,
fovvideovdp_amd/csrc/transpose_host.hpp: the fold-list and side-buffer checks (verdict and message text), the fill of the argument
block (taps, padded fold list), the ring length, the pixels per lane and the rule for the vector variant, against the restatement
of tests/transpose_host_check.cpp (the loops as they stood in the four entry points).  The program is compiled for the host
alone, with the address and undefined-behaviour sanitizers, and runs as a child process: nothing sanitized is loaded into this
one."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ingest_host_cpu import host_compiler         # noqa: E402


def test_checks_fill_and_vector_rule_against_restatement(tmp_path):
    exe = str(tmp_path / "transpose_host_check")
    cmd = host_compiler() + ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                             "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "fovvideovdp_amd", "csrc"),
                             "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "transpose_host_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    # cases: fl = 1 ... 64, the frame counts 1, 2, fl - 1, fl, fl + 1, 2 fl + 3 that are at least 1, the three paddings
    cases, lists = 0, 0
    for fl in range(1, 65):
        n_counts = sum(1 for N in (1, 2, fl - 1, fl, fl + 1, 2 * fl + 3) if N >= 1)
        cases += 3 * n_counts
        # per case: the valid list twice, and per entry 3 frames and 3 positions out of range, the position of the first / previous /
        # next / last entry (those that exist and are another entry), the swap with the next and with the last entry
        per_case = 2
        for i in range(fl):
            per_case += 6 + sum(1 for k in (0, i - 1, i + 1, fl - 1) if k != i and 0 <= k < fl)
            per_case += sum(1 for k in (i + 1, fl - 1) if i < k < fl)
        lists += 3 * n_counts * per_case
    # vector rule: 4 ring lengths x 5 sizes x 4 frame strides x 5 channel strides x 4 x 4 offsets of the fp32 buffers x 2 sample
    # sizes x 5 offsets of the samples, each under the four entry points' wordings
    rules = 4 * 5 * 4 * 5 * 4 * 4 * 2 * 5
    assert ran.stdout.strip() == "transpose_host: %d cases, %d fold lists, %d vector rules pass" % (cases, lists, rules)
