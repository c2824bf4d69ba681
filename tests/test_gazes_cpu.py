"""Many gazes per clip without a GPU: the fifth C header and its binding, the argument checks that need no context, the
workspace layout, the code objects of the new kernels, and the refusals of fvvdp.predict_gazes that come before any device
work.  (The checks that need a context -- not foveated, view maps set, small or misaligned workspace -- need a device to
create one: tests/test_gpu_gazes.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# VGPRs of multigaze_kernel<P, NG> as DESIGN.md section 4, "Many gazes per clip", states them
VGPRS = {(4, 1): 154, (4, 2): 168, (4, 4): 190, (4, 8): 234, (2, 1): 111, (2, 2): 125, (2, 4): 141, (2, 8): 172}


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def test_gaze_header_is_exported_and_bound():
    nat.build()
    names = declared("fvvdp_hip_gaze.h")
    assert names == ["fvvdp_bands_forward_gazes", "fvvdp_bands_forward_gazes_pool", "fvvdp_gaze_workspace"]
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert sorted(nat.GAZE_SYMBOLS) == names
    others = set(nat.SYMBOLS) | set(nat.IMAGE_SYMBOLS) | set(nat.GRAD_SYMBOLS) | set(nat.VIDEO_GRAD_SYMBOLS)
    assert not set(names) & others
    # the four existing headers keep their function lists
    assert [len(declared(h)) for h in ("fvvdp_hip.h", "fvvdp_hip_images.h", "fvvdp_hip_grad.h", "fvvdp_hip_video_grad.h")] == [24, 3, 2, 3]
    lib = nat.lib()
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    txt = open(os.path.join(ROOT, "include", "fvvdp_hip_gaze.h")).read()
    assert int(re.search(r"#define FVVDP_GAZE_GROUP_MAX (\d+)", txt).group(1)) == nat.GAZE_GROUP_MAX == max(ng for _, ng in VGPRS)


def test_a_null_context_is_refused_without_a_device():
    """Every other argument check of the forward entry points needs a real context to get past this one, and a context needs
    a device: they are in tests/test_gpu_gazes.py::test_argument_checks_that_need_a_context."""
    lib = nat.lib()
    g, pp = nat.Geom(), nat.PoolParams(1, 0.67, 1, 0.25, -0.016, 0.6)
    assert lib.fvvdp_bands_forward_gazes(None, 2, 3, None, 4, None, 2, 0, ctypes.byref(g), None, 0, None) == -1
    assert b"null" in lib.fvvdp_last_error()
    assert lib.fvvdp_bands_forward_gazes_pool(None, 2, 3, None, 4, None, 2, 0, ctypes.byref(g), None, 0, ctypes.byref(pp), None, None) == -1
    assert b"null" in lib.fvvdp_last_error()
    assert lib.fvvdp_bands_forward_gazes_pool(None, 2, 3, None, 4, None, 2, 0, ctypes.byref(g), None, 0, None, None, None) == -1
    assert b"null" in lib.fvvdp_last_error()


def test_workspace_matches_its_documented_layout():
    lib = nat.lib()
    nbytes = ctypes.c_size_t(0)
    assert lib.fvvdp_gaze_workspace(64, 48, 4, 5, 3, None) == -1 and b"null" in lib.fvvdp_last_error()
    for bad in ((0, 48, 4, 5, 3), (64, 0, 4, 5, 3), (64, 48, 0, 5, 3), (64, 48, 17, 5, 3), (64, 48, 4, 0, 3), (64, 48, 4, 5, 0)):
        assert lib.fvvdp_gaze_workspace(*bad, ctypes.byref(nbytes)) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert lib.fvvdp_gaze_workspace(64, 48, 4, 5, 3, ctypes.byref(nbytes)) == 0
    # coarse levels of bands 0..3: 32x24, 16x12, 8x6, 4x3 -- one strip each (wc <= 62), ceil(hc / 2) chunks at the most;
    # per gaze n * blk_b * 2 floats per band, the row rounded up to 64 floats
    blk = [1 * ((hc + 1) // 2) for hc in (24, 12, 6, 3)]
    assert blk == [12, 6, 3, 2]
    row = (sum(3 * b * 2 for b in blk) + 63) // 64 * 64
    assert nbytes.value == 5 * row * 4
    # a level wider than one strip: 3840 -> wc 1920 -> 1 + ceil((1920 - 62) / 60) = 32 strips
    assert lib.fvvdp_gaze_workspace(3840, 2160, 1, 2, 1, ctypes.byref(nbytes)) == 0
    assert nbytes.value == 2 * ((32 * 540 * 2 + 63) // 64 * 64) * 4


def test_new_kernels_do_not_spill_and_hold_the_stated_registers():
    import codeobj
    nat.build()
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    names = list(md)
    nice = codeobj.demangle(names)
    counted = ("band_kernel<", "band2_kernel<", "band2_fov_kernel<", "temporal_vec_kernel<", "temporal_ring_kernel<", "temporal_yuv",
               "still_ingest_kernel<", "pu21_sse_kernel<")          # substrings other tests count kernels by
    seen = {}
    for m, n in zip(names, nice):
        if "multigaze_kernel<" not in n and "finalize_gazes_kernel" not in n:
            continue
        x = md[m]
        assert (x["sgpr_spill_count"], x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), n
        assert not any(h in n for h in counted), n
        k = re.search(r"multigaze_kernel<(\d+), (\d+)>", n)
        if k:
            seen[(int(k.group(1)), int(k.group(2)))] = x["vgpr_count"]
            assert x["vgpr_count"] <= 256                       # two waves per SIMD at the least
    assert seen == VGPRS
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("Many gazes per clip"):]
    for (P, ng), v in VGPRS.items():
        assert re.search(r"\|\s*%d\s*\|\s*%d\s*\|\s*%d\s*\|" % (P, ng, v), sec), (P, ng, v)
    assert sum(1 for n in nice if "finalize_gazes_kernel" in n) == 1


def test_refusals_before_any_device_work():
    a = np.zeros((1, 1, 3, 64, 64), np.float32)
    fp = np.array([[10.0, 10.0], [20.0, 30.0]], np.float32)
    cpu = fv.fvvdp(display_name="standard_4k", foveated=True, device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpu.predict_gazes(a, a, fp, frames_per_second=30)
    with pytest.raises(RuntimeError, match="foveated"):
        fv.fvvdp(display_name="standard_4k", device=torch.device("cpu")).predict_gazes(a, a, fp, frames_per_second=30)
    with pytest.raises(RuntimeError, match="heat maps"):
        fv.fvvdp(display_name="standard_4k", foveated=True, heatmap="raw", device=torch.device("cpu")).predict_gazes(
            a, a, fp, frames_per_second=30)
    for bad in (np.zeros(2), np.zeros((2, 3)), np.zeros((2, 4, 2)), np.zeros((0, 2)), np.zeros((2, 3, 2, 1))):
        with pytest.raises(RuntimeError, match="fixation_points"):
            cpu.predict_gazes(a, a, bad, frames_per_second=30)
    x = torch.zeros((1, 1, 3, 64, 64), requires_grad=True)
    with pytest.raises(RuntimeError, match="Gradients"):
        cpu.predict_gazes(x, x.detach(), fp, frames_per_second=30)
    with pytest.raises(RuntimeError, match="Gradients"):
        cpu.predict_gazes(x.detach(), x, fp, frames_per_second=30)

    class Geometry(fv.fvvdp_display_geometry):
        pass

    user = fv.fvvdp(display_name="standard_4k", foveated=True, device=torch.device("cpu"),
                    display_geometry=Geometry((3840, 2160), diagonal_size_inches=30, distance_m=0.6))
    with pytest.raises(RuntimeError, match="display_geometry"):
        user.predict_gazes(a, a, fp, frames_per_second=30)
    # a valid [G, N, 2] trace array passes the shape check (and then meets the device check)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpu.predict_gazes(a, a, np.zeros((2, 3, 2), np.float32), frames_per_second=30)
