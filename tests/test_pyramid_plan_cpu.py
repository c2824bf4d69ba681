"""CPU test (no GPU) of the host code the three pyramid forward passes share, fovvideovdp_amd/csrc/pyramid_host.hpp: the launch plans
against the restatement of tests/pyramid_plan_check.cpp (the functions as they stood in fvvdp_hip.hip), every plan under every
override against the bound that sizes its partial sums -- the proof that the library's "internal: partial buffer too small" cannot
fire --, the strips and chunks as an exact cover, and the workspace rows.  The program is compiled for the host alone, with the
address and undefined-behaviour sanitizers, and runs as a child process: nothing sanitized is loaded into this one.

The dense range of level heights is thinned from every value 1 ... 300 to every value 1 ... 100 and every seventh from 107 on, with
300 itself: a search costs as many steps as the level has rows, and the whole program is to take a few seconds.  The boundary
cases (the widths around every strip boundary, the heights of 1080p ... 8K levels, 2161) are all there."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ingest_host_cpu import host_compiler         # noqa: E402


def test_plans_bounds_cover_and_rows(tmp_path):
    exe = str(tmp_path / "pyramid_plan_check")
    cmd = host_compiler() + ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                             "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "fovvideovdp_amd", "csrc"),
                             "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "pyramid_plan_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    # plans: 134 level heights x 6 frame counts x 4 capacities, each with the 8 strip counts of either pitch that the 27 level widths
    # have (1 ... 5 and those of 1920, 3840, 7680 columns)
    heights = list(range(1, 101)) + list(range(107, 300, 7)) + [300, 540, 1080, 2160, 2161, 4320]
    plans = len(heights) * 6 * 4 * (8 + 8)
    # frames: 13 x 13 sizes, each with 1 ... the most bands whose levels are all at least 2 x 2
    sides = (4, 5, 7, 8, 63, 64, 65, 125, 248, 249, 1920, 3840, 7680)
    def most_bands(s):
        k = 0
        while s >= 2 and k < 16:
            s, k = (s + 1) // 2, k + 1
        return k
    frames = sum(most_bands(min(w, h)) for w in sides for h in sides)
    # and the five rows whose byte counts test_multitest_cpu.py and test_gazes_cpu.py assert
    assert len(heights) == 134 and ran.stdout.strip() == "pyramid_host: %d cases pass" % (plans + frames + 5)
