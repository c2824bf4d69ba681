"""Many tests per reference under a gaze without a GPU: the C header fvvdp_hip_tests_fov.h and its binding, the argument checks
that need no context, the code objects of the new kernel, and the refusals of fvvdp.predict_tests_foveated that come before any
device work.  (The checks that need a context are in tests/test_gpu_tests_fov.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# registers of multitest_fov_kernel<NQ, RX> as DESIGN.md section 4, "Many tests per reference under a gaze", states them: the
# code object's vector register count (on gfx950 it includes the accumulation registers) and the accumulation registers in it
REGS = {(1, True): (169, 0), (2, False): (237, 0), (2, True): (249, 0), (3, False): (364, 108), (3, True): (406, 150)}
NAMES = ["fvvdp_bands_forward_tests_fov", "fvvdp_bands_forward_tests_fov_pool", "fvvdp_tests_fov_covered"]


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def test_header_is_exported_and_bound():
    nat.build()
    assert declared("fvvdp_hip_tests_fov.h") == NAMES
    assert sorted(nat.TESTS_FOV_SYMBOLS) == NAMES
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
    tables = {k: v for k, v in vars(nat).items() if k.endswith("SYMBOLS") and isinstance(v, dict)}
    for k, v in tables.items():
        if k != "TESTS_FOV_SYMBOLS":
            assert not set(NAMES) & set(v), k
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "fvvdp_hip_tests_fov.h":
            assert not set(NAMES) & set(declared(h)), h
    lib = nat.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    exports = open(os.path.join(ROOT, "fovvideovdp_amd", "csrc", "exports.map")).read()
    assert "global: fvvdp_*;" in exports and all(n in exports for n in NAMES)
    assert "fvvdp_hip_tests_fov.h" in open(os.path.join(ROOT, "fovvideovdp_amd", "_native.py")).read()      # a dependency of build()
    # the group constant is the plain tests pass's
    assert nat.TESTS_GROUP_MAX == max(k[0] for k in REGS)


def test_a_null_context_is_refused_without_a_device():
    lib = nat.lib()
    pp = nat.PoolParams(1, 0.67, 1, 0.25, -0.016, 0.6)
    geom = nat.Geom()
    fix = np.zeros((2, 2), np.float32)
    covered = ctypes.c_int(7)
    assert lib.fvvdp_bands_forward_tests_fov(None, 2, 3, None, 2, 0, nat.fptr(fix), ctypes.byref(geom), None, 0, None) == -1
    assert b"null" in lib.fvvdp_last_error()
    assert lib.fvvdp_bands_forward_tests_fov_pool(None, 2, 3, None, 2, 0, nat.fptr(fix), ctypes.byref(geom), None, 0, ctypes.byref(pp),
                                                  None, None) == -1
    assert b"null" in lib.fvvdp_last_error()
    assert lib.fvvdp_bands_forward_tests_fov_pool(None, 2, 3, None, 2, 0, None, None, None, 0, None, None, None) == -1
    assert b"null" in lib.fvvdp_last_error()
    assert lib.fvvdp_tests_fov_covered(None, ctypes.byref(geom), ctypes.byref(covered), None) == -1
    assert b"null" in lib.fvvdp_last_error() and covered.value == 7


def test_new_kernels_do_not_spill_and_hold_the_stated_registers():
    import codeobj
    nat.build()
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    names = list(md)
    nice = codeobj.demangle(names)
    counted = ("band_kernel<", "band2_kernel<", "band2_fov_kernel<", "temporal_vec_kernel<", "temporal_ring_kernel<", "temporal_yuv",
               "still_ingest_kernel<", "pu21_sse_kernel<", "multigaze_kernel<", "multitest_kernel<")   # substrings other tests count by
    seen = {}
    for m, n in zip(names, nice):
        if "multitest_fov_kernel<" not in n:
            continue
        x = md[m]
        assert (x["sgpr_spill_count"], x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), n
        assert not any(h in n for h in counted), n
        k = re.search(r"multitest_fov_kernel<(\d+), (true|false)>", n)
        seen[(int(k.group(1)), k.group(2) == "true")] = (x["vgpr_count"], x.get("agpr_count", 0))
        assert x["vgpr_count"] <= 512 and x["max_flat_workgroup_size"] == 256          # four waves, one per SIMD at the least
        assert x["group_segment_fixed_size"] == 768                                  # the axis knots; the LUT slice is dynamic
        if int(k.group(1)) <= 2:
            assert x["vgpr_count"] <= 256 and x.get("agpr_count", 0) == 0             # two waves per SIMD
    assert seen == REGS                                              # five instantiations
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("Many tests per reference under a gaze"):]
    for (nq, rx), (v, acc) in REGS.items():
        assert re.search(r"\|\s*%d\s*\|\s*%s\s*\|\s*%d\s*\|\s*%d\s*\|" % (nq, "yes" if rx else "no", v, acc), sec), (nq, rx, v, acc)


class _UserGeometry(fv.fvvdp_display_geometry):
    pass


class _UserPhotometry(fv.fvvdp_display_photometry):
    def forward(self, V):
        return 100.0 * V + 0.5

    def get_peak_luminance(self):
        return 100.5

    def get_black_level(self):
        return 0.5


def test_refusals_before_any_device_work():
    a = np.zeros((1, 1, 3, 64, 64), np.float32)
    cpu = fv.fvvdp(display_name="standard_4k", foveated=True, device=torch.device("cpu"))
    call = cpu.predict_tests_foveated
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # past every check, to the device check
        call([a, a], a, frames_per_second=30, fixation_point=[3, 4])
    with pytest.raises(RuntimeError, match="foveated metric.*predict_tests\\(\\)"):
        fv.fvvdp(display_name="standard_4k", device=torch.device("cpu")).predict_tests_foveated([a], a, frames_per_second=30)
    with pytest.raises(RuntimeError, match="heat maps"):
        fv.fvvdp(display_name="standard_4k", foveated=True, heatmap="raw", device=torch.device("cpu")).predict_tests_foveated(
            [a], a, frames_per_second=30)
    geo = _UserGeometry([3840, 2160], diagonal_size_inches=30, distance_m=0.6)
    with pytest.raises(RuntimeError, match="stock display geometry"):
        fv.fvvdp(display_name="standard_4k", display_geometry=geo, foveated=True, device=torch.device("cpu")).predict_tests_foveated(
            [a], a, frames_per_second=30)
    one = np.zeros((1, 1, 1, 64, 64), np.float32)
    with pytest.raises(RuntimeError, match="predict_images"):
        call([one], one, frames_per_second=30)
    with pytest.raises(RuntimeError, match="shape or dtype.*predict\\(\\)"):
        call([a, np.zeros((1, 1, 3, 64, 66), np.float32)], a, frames_per_second=30)
    with pytest.raises(RuntimeError, match="shape or dtype.*predict\\(\\)"):
        call([a.astype(np.float16)], a, frames_per_second=30)
    for bad in ([], (), a, None):
        with pytest.raises(RuntimeError, match="list or tuple"):
            call(bad, a, frames_per_second=30)
    x = torch.zeros((1, 1, 3, 64, 64), requires_grad=True)
    with pytest.raises(RuntimeError, match="Gradients"):
        call([x.detach(), x], x.detach(), frames_per_second=30)
    with pytest.raises(RuntimeError, match="Gradients"):
        call([x.detach()], x, frames_per_second=30)
    vs = fv.fvvdp_video_source_array(a, a, 30, display_photometry=cpu.display_photometry)
    for tests, ref in (([vs], a), (vs, a), ([a], vs)):
        with pytest.raises(RuntimeError, match="predict_video_source"):
            call(tests, ref, frames_per_second=30)
    for bad in ([1, 2, 3], np.zeros((2, 2), np.float32), np.zeros((3, 3), np.float32)):      # 3 frames: [x, y] or [3, 2]
        with pytest.raises(RuntimeError, match="fixation_point must be"):
            call([a], a, frames_per_second=30, fixation_point=bad)
    user = fv.fvvdp(display_name="standard_4k", display_photometry=_UserPhotometry(), foveated=True, device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="user photometry"):
        user.predict_tests_foveated([a], a, frames_per_second=30)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # integer input goes through the class's code-value table
        user.predict_tests_foveated([a.astype(np.uint8)], a.astype(np.uint8), frames_per_second=30)
    # the sentences of the plain pass name the new call for a foveated metric
    with pytest.raises(RuntimeError, match="predict_tests_foveated"):
        cpu.predict_tests([a], a, frames_per_second=30)
