"""CPU test (no GPU) of the host code the clip ingests share, fovvideovdp_amd/csrc/ingest_host.hpp: the launch windows of a call and
the filler of a window's part of an argument block, against the direct restatement of tests/ingest_windows_check.cpp.  The program
is compiled for the host alone, with the address and undefined-behaviour sanitizers, and runs as a child process: nothing
sanitized is loaded into this one."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_compiler():
    """A C++17 host compiler and what makes it link the sanitizers' runtimes INTO the program (a runtime that is a shared library
    of its own refuses to start wherever the environment preloads another library): the clang that hipcc drives, else the
    system's clang or gcc."""
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    rocm_clang = os.path.join(os.path.dirname(hipcc), "..", "llvm", "bin", "clang++")
    for cxx, static in ((rocm_clang, []), ("clang++", []), ("g++", ["-static-libasan", "-static-libubsan"])):
        path = shutil.which(cxx)
        if path:
            return [path] + static
    raise RuntimeError("no C++ host compiler found (clang++ or g++)")


def test_window_filler_against_restatement(tmp_path):
    exe = str(tmp_path / "ingest_windows_check")
    cmd = host_compiler() + ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                             "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "fovvideovdp_amd", "csrc"),
                             "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "ingest_windows_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    # 11 filter lengths x 6 call lengths, each with one list for both streams and with a list per stream
    assert ran.stdout.strip() == "ingest_host: 132 cases pass"
