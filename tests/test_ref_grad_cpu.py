"""Gradients with respect to the reference without a GPU: the header and its binding, the argument checks of its entry points,
the code objects of the new kernels and of the map-writing pyramid variants, the memory accounting per `wrt`, the goldens
g21 / g22 and their clamp-coverage cases, and the handling of `wrt` that comes before any device work."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd import image_grad, video_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_grad_cases as rc                # noqa: E402


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def test_ref_grad_header_is_exported_and_bound():
    nat.build()
    names = declared("fvvdp_hip_ref_grad.h")
    assert names == ["fvvdp_ctx_set_slope_maps", "fvvdp_images_ref_grad", "fvvdp_ref_grad_workspace", "fvvdp_video_ref_grad_frames"]
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert sorted(nat.REF_GRAD_SYMBOLS) == names
    others = set(nat.SYMBOLS) | set(nat.IMAGE_SYMBOLS) | set(nat.GRAD_SYMBOLS) | set(nat.VIDEO_GRAD_SYMBOLS) | \
        set(nat.GAZE_SYMBOLS) | set(nat.GAZE_GRAD_SYMBOLS)
    assert not set(names) & others
    lib = nat.lib()
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    # internal launch helpers stay internal
    assert not hasattr(L, "grad_input_launch") and not hasattr(L, "grad_coef_launch")


def test_workspace_matches_its_documented_layout():
    lib = nat.lib()
    nbytes = ctypes.c_size_t(0)
    assert lib.fvvdp_ref_grad_workspace(64, 48, 4, 3, 2, None) == -1
    assert lib.fvvdp_ref_grad_workspace(64, 48, 4, 3, 3, ctypes.byref(nbytes)) == -1 and b"planes" in lib.fvvdp_last_error()
    assert lib.fvvdp_ref_grad_workspace(64, 48, 17, 3, 2, ctypes.byref(nbytes)) == -1
    assert lib.fvvdp_ref_grad_workspace(64, 48, 4, 0, 1, ctypes.byref(nbytes)) == -1
    sizes = [(64, 48), (32, 24), (16, 12), (8, 6), (4, 3)]
    al = lambda x: (x + 63) // 64 * 64
    for planes in (1, 2):
        assert lib.fvvdp_ref_grad_workspace(64, 48, 4, 3, planes, ctypes.byref(nbytes)) == 0
        n = 3 * planes
        # coef | GLR of levels 0..3 | GG of levels 1..4 | GX of levels 0..3, each part 256-byte aligned
        expect = al(n * 4) + 2 * sum(al(n * w * h) for w, h in sizes[:4]) + sum(al(n * w * h) for w, h in sizes[1:])
        assert nbytes.value == 4 * expect
        test_side = ctypes.c_size_t(0)
        ws = lib.fvvdp_video_grad_workspace if planes == 2 else lib.fvvdp_images_grad_workspace
        assert ws(64, 48, 4, 3, ctypes.byref(test_side)) == 0
        assert nbytes.value == test_side.value + 4 * sum(al(n * w * h) for w, h in sizes[:4])


def test_argument_checks_need_no_device():
    lib = nat.lib()
    assert lib.fvvdp_ctx_set_slope_maps(None, None) == -1 and b"null context" in lib.fvvdp_last_error()
    prm, pp = nat.Params(), nat.PoolParams(1, 0.67, 1, 0.25, -0.016, 0.6)
    prm.beta = 0.96
    maps = (nat.BandMaps * 4)()
    for b in range(4):
        maps[b].d_D = maps[b].d_contrast = maps[b].d_lbkg = maps[b].d_S = 256
    p = ctypes.c_void_p(256)
    slopes = (ctypes.c_void_p * 4)(256, 256, 256, 256)
    holes = (ctypes.c_void_p * 4)(256, 256, None, 256)

    def frames(n_bands=4, n=2, n_frames=5, f0=0, work=1 << 30, work_ptr=256, sl=slopes):
        return lib.fvvdp_video_ref_grad_frames(64, 48, n_bands, n, ctypes.byref(prm), ctypes.byref(pp), p, n_frames, f0, p, maps, sl,
                                               p, ctypes.c_void_p(work_ptr), work, None)

    assert lib.fvvdp_video_ref_grad_frames(64, 48, 4, 2, None, None, None, 5, 0, None, None, None, None, None, 0, None) == -1
    assert frames(n_bands=17) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert frames(f0=4) == -1 and b"outside the clip" in lib.fvvdp_last_error()
    assert frames(work=16) == -1 and b"workspace" in lib.fvvdp_last_error()
    assert frames(work_ptr=260) == -1 and b"aligned" in lib.fvvdp_last_error()
    assert frames(sl=holes) == -1 and b"slope plane" in lib.fvvdp_last_error()
    assert frames(sl=None) == -1 and b"null" in lib.fvvdp_last_error()

    e = nat.Eotf()
    e.kind = nat.EOTF_SRGB
    w = np.array([0.2126, 0.7152, 0.0722], np.float32)
    imgs = (ctypes.c_void_p * 2)(256, 256)

    def images(C=3, kind=nat.EOTF_SRGB, sl=slopes, work=1 << 30, q_col0=0):
        e.kind = kind
        return lib.fvvdp_images_ref_grad(64, 48, 4, 2, ctypes.byref(prm), ctypes.byref(pp), p, 2, q_col0, p, maps, sl, imgs, C, 64 * 48,
                                         ctypes.byref(e), nat.fptr(w), imgs, p, work, None)

    assert images(C=2) == -1 and b"colour channels" in lib.fvvdp_last_error()
    assert images(kind=nat.EOTF_LUT) == -1 and b"closed-form" in lib.fvvdp_last_error()
    assert images(sl=holes) == -1 and b"slope plane" in lib.fvvdp_last_error()
    assert images(work=16) == -1 and b"workspace" in lib.fvvdp_last_error()
    assert images(q_col0=1) == -1 and b"Q columns" in lib.fvvdp_last_error()


def test_new_kernels_do_not_spill_and_the_map_writing_variants_stay_out_of_scratch():
    import codeobj
    nat.build()
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    names = list(md)
    nice = codeobj.demangle(names)
    found = {"void ref_layer_kernel<1>": 0, "void ref_layer_kernel<2>": 0}
    map_writing = {}
    for m, n in zip(names, nice):
        base = n.split("(")[0]
        x = md[m]
        if base in found:
            found[base] += 1
            assert (x["sgpr_spill_count"], x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), n
        if "band_kernel<" in base and ", true, " in base:
            map_writing[base] = x
    assert found == {k: 1 for k in found}
    # the variants that gained the optional slope plane: P = 2 / 4, plain and foveated; nothing in scratch, the foveated ones
    # keep their few scalars in vector lanes as before (test_host_cpu.py allows 24)
    assert sorted(map_writing) == ["void band_kernel<2, true, 0>", "void band_kernel<2, true, 2>", "void band_kernel<4, true, 0>",
                                   "void band_kernel<4, true, 2>"]
    for base, x in map_writing.items():
        assert x["private_segment_fixed_size"] == 0 and x["vgpr_spill_count"] == 0, (base, x)
        assert x["sgpr_spill_count"] <= 24, (base, x)
    # the kernels the reference's backward shares with the test's are still defined once
    for k in ("grad_coef_kernel", "adj_layer_kernel", "adj_sweep_kernel", "grad_input_kernel", "video_coef_kernel",
              "video_layer_kernel", "video_level0_kernel"):
        assert sum(1 for n in nice if n.split("(")[0] == k) == 1, k


def test_memory_accounting_counts_the_extra_planes_per_wrt():
    # images: maps 7, test workspace GL + GG = 2; reference: slope 2 + GLR + GX + GG = 3
    assert [image_grad.grad_planes(w) for w in image_grad.WRT] == [9, 12, 14]
    # video: maps 9, test workspace 2 x 2; reference: slope 2 + 3 x 2
    assert [video_grad.video_grad_planes(w) for w in image_grad.WRT] == [13, 17, 21]
    assert image_grad.grad_planes("test") == image_grad.GRAD_PLANES and video_grad.video_grad_planes("test") == video_grad.GRAD_PLANES

    class M:
        grad_batch = None
        _level_sizes = staticmethod(fv.fvvdp._level_sizes)

    W, H, nb = 3840, 2160, 9
    px = sum(w * h for w, h in M._level_sizes(W, H, nb))
    sizes = [image_grad.grad_batch_size(M, W, H, nb, 1000, video_grad.video_grad_planes(w)) for w in image_grad.WRT]
    assert sizes == [int(image_grad.GRAD_BYTES_BUDGET // (px * 4 * k)) for k in (13, 17, 21)] and sizes[0] > sizes[1] > sizes[2] >= 1
    M.grad_batch = 5
    assert image_grad.grad_batch_size(M, W, H, nb, 1000, 21) == 5
    # the check against free memory: per differentiated input a clip-long g0 and a result, the slope planes with the maps
    N, HW, numel, fl, gb, bpx = 60, W * H, 3 * 60 * W * H, 8, 4, 11_000_000
    one = video_grad.backward_bytes(gb, bpx, 1000, N, HW, numel, fl)
    ref = video_grad.backward_bytes(gb, bpx, 1500, N, HW, numel, fl, 1, True)
    both = video_grad.backward_bytes(gb, bpx, 2500, N, HW, numel, fl, 2, True)
    assert one == gb * bpx * 36 + 1000 + fl * HW * 4 + N * HW * 8 + numel * 4
    assert ref - one == gb * bpx * 8 + 500
    assert both - ref == 1000 + N * HW * 8 + numel * 4


def test_goldens_are_small_and_finite():
    files = {rc.IMAGE_FILE} | set(rc.VIDEO_FILES.values())
    for f in files:
        path = os.path.join(rc.GOLDEN, f)
        assert os.path.getsize(path) < 1 << 20, f
        z = np.load(path)
        assert all(k.endswith("_jod") or k.endswith("_gref") for k in z.files), z.files        # outputs only
        for k in z.files:
            assert np.isfinite(z[k]).all(), (f, k)
    for name, (C, H, W, _, _) in rc.IMAGE_CASES.items():
        assert rc.load_image_golden(name)[1].shape == (C, H, W), name
        assert rc.image_inputs(name)[1].shape == (C, H, W)
    for name, (C, N, H, W) in ((k, v[:4]) for k, v in rc.VIDEO_CASES.items()):
        assert rc.load_video_golden(name)[1].shape == (C, N, H, W), name
    # the identical pair has an all-zero gradient; the clip in which no window shows frame 0 has zeros there only
    assert (rc.load_image_golden("g_identical")[1] == 0).all()
    g = rc.load_video_golden("c_gray_30_circular")[1]
    assert (g[:, 0] == 0).all() and (g[:, 1:] != 0).any()
    # reference samples outside [0, 1] get exact zeros
    for load, inputs, name in ((rc.load_image_golden, rc.image_inputs, "b_rgb_4k_oob"), (rc.load_video_golden, rc.video_inputs, "e_rgb_pq_oob")):
        r = inputs(name)[1]
        oob = (r < 0) | (r > 1)
        assert oob.any() and (load(name)[1][oob] == 0).all()


def test_clamp_coverage_cases_bind_every_clamp():
    """The oracle's maps of the two dark cases: the L_bkg clamp and the contrast clamp of the test bind in both; the contrast
    clamp of the reference binds in the clip (transient plane) and cannot in a still image (ref_grad_cases._dark_frame)."""
    img = rc.clamp_counts("i_hdr_linear_dark")
    vid = rc.clamp_counts("s_hdr_linear_dark")
    print(img, vid)
    assert img["lbkg"] > 0 and img["t"] > 0 and img["r"] == 0
    assert vid["lbkg"] > 0 and vid["t"] > 0 and vid["r"] > 0


def test_wrt_handling_without_device():
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    x, r = torch.rand((1, 3, 4, 32, 48)), torch.rand((1, 3, 4, 32, 48))
    xg, rg = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    for call in (lambda a, b, **kw: m.jod_video(a, b, frames_per_second=30, **kw), lambda a, b, **kw: m.jod_images(a[:, :, 0], b[:, :, 0], **kw)):
        with pytest.raises(RuntimeError, match=r"gradients with respect to the reference are not supported.*wrt="):
            call(xg, rg)
        with pytest.raises(RuntimeError, match='"both"'):
            call(xg, rg, wrt="reference")
        with pytest.raises(ValueError, match="wrt must be"):
            call(x, r, wrt="Reference")
        with pytest.raises(ValueError):
            call(x, r, wrt=None)
        for wrt in ("reference", "both"):                       # accepted: the next refusal is the missing device
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call(x, rg, wrt=wrt)
        with torch.no_grad():                                   # grad mode off: nothing to refuse
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call(xg, rg)
    fm = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True, foveated=True)
    with pytest.raises(RuntimeError, match="reference are not supported.*jod_images and jod_video only"):
        fm.jod_gazes(x, rg, [[1.0, 2.0]], frames_per_second=30)
    with pytest.raises(TypeError):
        fm.jod_gazes(x, r, [[1.0, 2.0]], frames_per_second=30, wrt="both")
