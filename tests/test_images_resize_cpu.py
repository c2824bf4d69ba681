"""Mixed-resolution still images without a GPU: the header and its binding, the argument checks of its three entry points, every
refusal of fvvdp.predict_images_resized / jod_images_resized / predict_image_pairs_resized that comes before any device work, the
code objects of the new kernels, the case table and the goldens, and -- in numpy alone -- that the bounds of the GPU tests see a
wrong kernel."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import images_resize_cases as ic             # noqa: E402
import pyramid_grad_ref as pgr               # noqa: E402
import resize_cases as rc                    # noqa: E402
import resize_ref as rref                    # noqa: E402
import yuv_channels_ref as yref              # noqa: E402

NEW_KERNELS = ["void still_resized_kernel<%d, %d>" % (2 if m <= 1 else 1, m) for m in range(4)] + ["images_level0_kernel"]
NAMES = ["fvvdp_images_channels_resized", "fvvdp_images_grad_luminance", "fvvdp_images_grad_luminance_workspace"]


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def rgb2y():
    return np.asarray(yref.orc.load_defaults()["color_spaces.json"]["sRGB"]["RGB2Y"], np.float32)


def test_images_resize_header_is_exported_and_bound():
    nat.build()
    names = declared("fvvdp_hip_images_resize.h")
    assert names == NAMES
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert sorted(nat.IMAGES_RESIZE_SYMBOLS) == names
    lib = nat.lib()
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    txt = open(os.path.join(ROOT, "include", "fvvdp_hip_resize.h")).read()
    assert int(re.search(r"#define FVVDP_RESIZE_MAX_AXIS (\d+)", txt).group(1)) == nat.RESIZE_MAX_AXIS
    for fn in ("predict_images_resized", "jod_images_resized", "predict_image_pairs_resized"):
        assert callable(getattr(fv.fvvdp, fn))
    # the unit is built without contraction of multiplies and adds, as resize_launch.hip
    src = open(os.path.join(ROOT, "fovvideovdp_amd", "_native.py")).read()
    assert re.search(r'"images_resize_launch\.hip"\), \["-ffp-contract=off"\]', src)


def test_argument_checks_need_no_device():
    lib = nat.lib()
    p = ctypes.c_void_p
    e = nat.Eotf()
    w = np.ones(3, np.float32)
    B = 3

    def stream(data=256, dtype=nat.FVVDP_F32, C=3, width=60, height=34, fs=None, ps=None):
        hw = width * height
        return nat.ResizeStream(data, dtype, C, width, height, C * hw if fs is None else fs, hw if ps is None else ps)

    # the ingest: everything that is checked before the context is looked at (a context needs a device)
    def ing(ctx=256, t=None, r=None, mode=1, kind=nat.EOTF_SRGB, n=B):
        e.kind = kind
        return lib.fvvdp_images_channels_resized(p(ctx), ctypes.byref(t or stream()), ctypes.byref(r or stream(dtype=nat.FVVDP_U8)), n,
                                                 mode, ctypes.byref(e), nat.fptr(w), 0, None)

    out_of_range = b"frame size out of range (1..32768 per axis)"
    assert ing(ctx=None) == -1 and b"null" in lib.fvvdp_last_error()
    assert lib.fvvdp_images_channels_resized(p(256), None, None, B, 1, None, None, 0, None) == -1 and b"null" in lib.fvvdp_last_error()
    assert ing(mode=4) == -1 and b"unknown resize mode" in lib.fvvdp_last_error()
    assert ing(mode=-1) == -1 and b"unknown resize mode" in lib.fvvdp_last_error()
    assert ing(kind=nat.EOTF_LUT) == -1 and b"closed-form" in lib.fvvdp_last_error()
    assert ing(kind=nat.EOTF_NONE) == -1 and b"closed-form" in lib.fvvdp_last_error()
    assert ing(t=stream(data=0)) == -1 and b"null data pointer (test)" in lib.fvvdp_last_error()
    assert ing(r=stream(dtype=nat.FVVDP_U16)) == -1 and b"the reference must be float32 or uint8" in lib.fvvdp_last_error()
    assert ing(t=stream(dtype=nat.FVVDP_F16)) == -1 and b"the test must be float32 or uint8" in lib.fvvdp_last_error()
    assert ing(r=stream(data=258)) == -1 and b"aligned to 4 bytes (reference)" in lib.fvvdp_last_error()
    assert ing(t=stream(C=2)) == -1 and b"1 or 3 colour channels" in lib.fvvdp_last_error()
    assert ing(r=stream(C=1)) == -1 and b"differ in their channel counts (3 and 1)" in lib.fvvdp_last_error()
    assert ing(t=stream(height=-3)) == -1 and b"bad frame size" in lib.fvvdp_last_error()
    assert ing(t=stream(width=1, height=32769)) == -1 and out_of_range + b": 1x32769 (test)" in lib.fvvdp_last_error()
    assert ing(r=stream(dtype=nat.FVVDP_U8, width=40000, height=2)) == -1 and out_of_range + b": 40000x2 (reference)" in lib.fvvdp_last_error()
    assert ing(t=stream(ps=60 * 34 - 1)) == -1 and b"plane_stride" in lib.fvvdp_last_error()
    assert ing(r=stream(fs=60 * 34 - 1)) == -1 and b"frame_stride" in lib.fvvdp_last_error()
    # the largest size passes this check: the call is refused by a later one
    assert ing(t=stream(width=32768, height=2), r=stream(C=1)) == -1 and b"channel counts" in lib.fvvdp_last_error()

    # the adjoint both sides go through takes float32 stacks only: a differentiated stack of another type is refused there
    def adj(t):
        e.kind = nat.EOTF_SRGB
        return lib.fvvdp_resize_grad(120, 68, B, p(256), ctypes.byref(t), p(512), 1, ctypes.byref(e), nat.fptr(w), p(1024), 1 << 30, None)

    assert adj(stream(dtype=nat.FVVDP_U8)) == -1 and b"must be float32 (" in lib.fvvdp_last_error()

    # the workspace: the test side's is fvvdp_images_grad's, the reference side's fvvdp_ref_grad's for image pairs
    nbytes, other = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.fvvdp_images_grad_luminance_workspace(64, 48, 4, 2, 0, None) == -1 and b"null" in lib.fvvdp_last_error()
    assert lib.fvvdp_images_grad_luminance_workspace(64, 48, 0, 2, 0, ctypes.byref(nbytes)) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert lib.fvvdp_images_grad_luminance_workspace(64, 48, 4, 0, 1, ctypes.byref(nbytes)) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert lib.fvvdp_images_grad_luminance_workspace(64, 48, 4, 2, 0, ctypes.byref(nbytes)) == 0
    assert lib.fvvdp_images_grad_workspace(64, 48, 4, 2, ctypes.byref(other)) == 0 and nbytes.value == other.value
    assert lib.fvvdp_images_grad_luminance_workspace(64, 48, 4, 2, 1, ctypes.byref(nbytes)) == 0
    assert lib.fvvdp_ref_grad_workspace(64, 48, 4, 2, 1, ctypes.byref(other)) == 0 and nbytes.value == other.value
    need_ref = nbytes.value

    # the level-0 step: a complete argument list with a bad shape, map, slope plane or workspace is refused before any launch
    prm, pp = nat.Params(), nat.PoolParams(1, 1, 1, 1, -0.016, 0.6)
    prm.beta = 1.5
    maps = (nat.BandMaps * 4)()
    for b in range(4):
        maps[b].d_D = maps[b].d_contrast = maps[b].d_lbkg = maps[b].d_S = 256
    slopes = (ctypes.c_void_p * 4)(256, 256, 256, 256)

    def lum(n_bands=4, n=2, q_col0=0, gL=256, work=1024, bytes_=1 << 30, sl=None, mp=maps):
        return lib.fvvdp_images_grad_luminance(64, 48, n_bands, n, ctypes.byref(prm), ctypes.byref(pp), p(256), 2, q_col0, p(256), mp,
                                               sl, p(gL), p(work), bytes_, None)

    assert lib.fvvdp_images_grad_luminance(64, 48, 4, 2, None, None, None, 2, 0, None, None, None, None, None, 0, None) == -1
    assert b"null" in lib.fvvdp_last_error()
    assert lum(gL=None) == -1 and b"null" in lib.fvvdp_last_error()
    assert lum(n_bands=17) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert lum(n=0) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert lum(q_col0=1) == -1 and b"Q columns" in lib.fvvdp_last_error()
    assert lum(gL=258) == -1 and b"d_gL must be aligned" in lib.fvvdp_last_error()
    assert lum(work=1025) == -1 and b"256-byte aligned" in lib.fvvdp_last_error()
    assert lum(bytes_=16) == -1 and b"workspace of 16 bytes is below" in lib.fvvdp_last_error()
    # (the reference side needs the larger workspace: what suffices for the test side does not)
    assert lum(bytes_=need_ref - 1, sl=slopes) == -1 and b"is below the %d needed" % need_ref in lib.fvvdp_last_error()
    assert lum(sl=(ctypes.c_void_p * 4)(256, 256, None, 256)) == -1 and b"band 2: the slope plane is required" in lib.fvvdp_last_error()
    holed = (nat.BandMaps * 4)()
    for b in range(4):
        holed[b].d_D = holed[b].d_contrast = holed[b].d_lbkg = holed[b].d_S = 256
    holed[1].d_S = None
    assert lum(mp=holed) == -1 and b"band 1: every map" in lib.fvvdp_last_error()
    prm.beta = 0.0
    assert lum() == -1 and b"pooling exponents" in lib.fvvdp_last_error()


CALLS = ("predict_images_resized", "jod_images_resized")


def test_refusals_without_device():
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    t, r = torch.rand(2, 3, 17, 30), torch.rand(2, 3, 34, 60)
    kw = dict(resize_resolution=(60, 34))
    for name in CALLS:
        call = getattr(m, name)
        with pytest.raises(RuntimeError, match="Unknown resize method 'lanczos'"):
            call(t, r, full_screen_resize="lanczos", **kw)
        with pytest.raises(RuntimeError, match="Unknown resize method 'None'"):
            call(t, r, full_screen_resize=None, **kw)
        for bad in (torch.float64, torch.int16):
            with pytest.raises(RuntimeError, match="the test is .*loat64 and uint16 samples are not supported"):
                call(t.to(bad), r, **kw)
            with pytest.raises(RuntimeError, match="the reference is .*loat64 and uint16 samples are not supported"):
                call(t, r.to(bad), **kw)
        with pytest.raises(RuntimeError, match="the reference is uint16"):
            call(t, (r.numpy() * 65535).astype(np.uint16), **kw)
        with pytest.raises(RuntimeError, match="differ in their image counts \\(2 and 1\\)"):
            call(t, r[:1], **kw)
        with pytest.raises(RuntimeError, match="differ in their channel counts \\(3 and 1\\)"):
            call(t, r[:, :1], **kw)
        with pytest.raises(RuntimeError, match="either 1 or 3 colour channels"):
            call(t[:, :2], r[:, :2], **kw)
        with pytest.raises(RuntimeError, match="F axis must have size 1 .*predict_resized"):
            call(torch.rand(2, 3, 4, 17, 30), torch.rand(2, 3, 4, 34, 60), dim_order="BCFHW", **kw)
        with pytest.raises(RuntimeError, match="needs a B axis"):
            call(t[0], r[0], dim_order="CHW", **kw)
        with pytest.raises(RuntimeError, match="exactly as many dimensions"):
            call(t, r, dim_order="CHW", **kw)
        for bad in ((0, 34), (60, 32769), (-1, 5)):
            with pytest.raises(RuntimeError, match="frame size out of range \\(1..32768 per axis\\): .* \\(resize_resolution\\)"):
                call(t, r, resize_resolution=bad)
        with pytest.raises(RuntimeError, match="frame size out of range \\(1..32768 per axis\\): 32769x1 \\(test\\)"):
            call(torch.zeros(1, 1, 1, 32769), torch.zeros(1, 1, 2, 2), **kw)
        with pytest.raises(RuntimeError, match="frame size out of range \\(1..32768 per axis\\): 1x32769 \\(reference\\)"):
            call(torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 32769, 1), **kw)
        # everything accepted: the first device work is refused on a CPU metric (the default target is the display's resolution)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(t, r, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(t, (r * 255).to(torch.uint8), full_screen_resize="area")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(t[:, :, None], r[:, :, None], dim_order="BCFHW", **kw)               # F == 1
        with pytest.raises(RuntimeError, match="no CPU fallback"):                    # both at the target size: predict_images / jod_images
            call(r, r.clone(), **kw)
    # half precision: refused by the forward-only calls, upcast by the differentiable one
    for bad in (torch.float16, torch.bfloat16):
        with pytest.raises(RuntimeError, match="the test is .*Half-precision, float64 and uint16 samples are not supported"):
            m.predict_images_resized(t.to(bad), r, **kw)
        with pytest.raises(RuntimeError, match="the reference is .*Half-precision"):
            m.predict_image_pairs_resized([(t[0], r[0].to(bad))], dim_order="CHW", **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.jod_images_resized(t.to(bad).requires_grad_(True), r, **kw)
    # inputs that require grad
    for x, y in ((t.clone().requires_grad_(True), r), (t, r.clone().requires_grad_(True))):
        with pytest.raises(RuntimeError, match="predict_images_resized is forward-only"):
            m.predict_images_resized(x, y, **kw)
        with pytest.raises(RuntimeError, match="predict_image_pairs_resized is forward-only"):
            m.predict_image_pairs_resized([(x[0], y[0])], dim_order="CHW", **kw)
    with pytest.raises(RuntimeError, match="gradients with respect to the reference are not supported; detach the reference, or ask"):
        m.jod_images_resized(t, r.clone().requires_grad_(True), **kw)
    with pytest.raises(RuntimeError, match='wrt="reference" treats the test as a constant'):
        m.jod_images_resized(t.clone().requires_grad_(True), r, wrt="reference", **kw)
    # a differentiated side is float32 (or a half type, upcast); the constant side may be uint8
    with pytest.raises(RuntimeError, match='wrt="test" differentiates the test, which must be float32'):
        m.jod_images_resized((t * 255).to(torch.uint8), r, **kw)
    with pytest.raises(RuntimeError, match='wrt="reference" differentiates the reference, which must be float32'):
        m.jod_images_resized(t, (r * 255).to(torch.uint8), wrt="reference", **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.jod_images_resized((t * 255).to(torch.uint8), r.clone().requires_grad_(True), wrt="reference", **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.jod_images_resized(t.clone().requires_grad_(True), (r * 255).to(torch.uint8), wrt="both", **kw)
    # the list form: one pair per entry, one gaze per pair
    with pytest.raises(RuntimeError, match="one image pair per list entry"):
        m.predict_image_pairs_resized([(t, r)], dim_order="BCHW", **kw)
    with pytest.raises(RuntimeError, match="one \\[x, y\\] \\(or None\\) per image pair"):
        m.predict_image_pairs_resized([(t[0], r[0])], dim_order="CHW", fixation_points=[None, None], **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict_image_pairs_resized([(t[0].permute(1, 2, 0), r[0].permute(1, 2, 0)), (r[1].permute(1, 2, 0), t[1].permute(1, 2, 0))], **kw)


@pytest.mark.parametrize("wrt", ["tests", "", None, "Test", ("test",)])
def test_wrt_values_other_than_the_three_raise(wrt):
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    with pytest.raises(ValueError, match='wrt must be "test", "reference" or "both"'):
        m.jod_images_resized(torch.rand(1, 3, 17, 30), torch.rand(1, 3, 34, 60), resize_resolution=(60, 34), wrt=wrt)


def test_refuses_user_photometry():
    class MyDisplay(fv.fvvdp_display_photometry):
        def forward(self, V):
            return 100.0 * V + 0.5

        def get_peak_luminance(self):
            return 100.5

        def get_black_level(self):
            return 0.5

    m = fv.fvvdp(display_name="standard_4k", display_photometry=MyDisplay(), device="cpu", quiet=True)
    t, r = torch.rand(2, 3, 17, 30), torch.rand(2, 3, 34, 60)
    for name in CALLS:
        with pytest.raises(RuntimeError, match="%s needs a display model with a closed form .*fractional after the resize" % name):
            getattr(m, name)(t, r, resize_resolution=(60, 34))
    with pytest.raises(RuntimeError, match="predict_image_pairs_resized needs a display model with a closed form"):
        m.predict_image_pairs_resized([(t[0], r[0])], dim_order="CHW", resize_resolution=(60, 34))


def test_new_kernels_do_not_spill():
    import codeobj
    nat.build()
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    names = list(md)
    nice = codeobj.demangle(names)
    found = {k: 0 for k in NEW_KERNELS}
    for mname, n in zip(names, nice):
        base = n.split("(")[0]
        if base in found:
            found[base] += 1
            x = md[mname]
            assert (x["vgpr_spill_count"], x["sgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), n
            assert x["max_flat_workgroup_size"] == 256, n
    assert found == {k: 1 for k in found}
    # none of the names the other tests count by substring
    for n in NEW_KERNELS:
        assert not any(s in n for s in ("temporal_vec_kernel<", "band2_kernel<", "band_kernel<", "temporal_ring_kernel<",
                                        "temporal_yuv_kernel<", "temporal_yuv_vec_kernel<", "video_input_kernel<",
                                        "yuvplanes_ring_kernel<", "video_lum_input_kernel<", "resized_ring_kernel<",
                                        "resize_adjoint_d_kernel<", "resize_adjoint_gather_kernel<", "still_ingest_kernel<",
                                        "video_level0_kernel", "grad_input_kernel", "pool_jod_cols_kernel"))


# ---- the case table and the goldens ---------------------------------------------------------------------------------------------------
def test_rotation_covers_the_matrix():
    R = ic.rotation()
    assert len(R) >= 8 and len({ic.case_id(c) for c in R}) == len(R)
    assert {(c["mode"], c["C"]) for c in R} == {(m, C) for m in rref.MODES for C in (1, 3)}
    assert {c["ref_dtype"] for c in R} == {"float32", "uint8"} and {c["display"] for c in R} == set(rc.DISPLAYS)
    assert {c["target"] for c in R} == set(rc.TARGETS) and set(rc.SOURCES) <= {c["source"] for c in R}
    # the reference at the target's size, at the test's size and at a third size; the test at the target's size
    assert any(c["ref_source"] is None for c in R) and any(c["ref_source"] == c["source"] != c["target"] for c in R)
    assert any(c["ref_source"] not in (None, c["source"]) and c["source"] != c["target"] for c in R)
    assert any(c["source"] == c["target"] and c["ref_source"] is not None for c in R)
    assert any(c["mode"] == "nearest" and c["source"] == (240, 136) for c in R)


def test_case_inputs_keep_their_margin():
    for c in ic.rotation():
        test, ref = ic.rotation_inputs(c)
        again, _ = ic.rotation_inputs(c)
        assert test.dtype == np.float32 and str(ref.dtype) == c["ref_dtype"] and again is test
        assert test.shape == (ic.B, c["C"], *c["source"][::-1]) and ref.shape == (ic.B, c["C"], *(c["ref_source"] or c["target"])[::-1])
        for x, src in ((test, c["source"]), (ref, c["ref_source"])):
            if src is not None and src != c["target"]:
                assert not rref.margin(x, c["target"], c["mode"]).any(), ic.case_id(c)
    for name in ic.CASES:
        C, tsize, rsize, target, mode = ic.CASES[name][:5]
        test, ref = ic.case_inputs(name)
        assert test.shape == (ic.B, C, *tsize[::-1]) and ref.shape == (ic.B, C, *rsize[::-1])
        assert test.dtype == ref.dtype == np.float32
        for x, size in ((test, tsize), (ref, rsize)):
            if size != target:
                assert not rref.margin(x, target, mode).any(), name


@pytest.mark.parametrize("name", sorted(ic.CASES))
def test_goldens_load(name):
    C, tsize, rsize, target, mode, display, wrt, opt = ic.CASES[name]
    path = os.path.join(ic.GOLDEN, ic.FILES[name])
    largest_g25 = max(os.path.getsize(os.path.join(ic.GOLDEN, f)) for f in os.listdir(ic.GOLDEN) if f.startswith("g25_"))
    assert os.path.getsize(path) <= largest_g25
    jod, gt, gr = ic.load_golden(name)
    assert jod.shape == (ic.B,) and ((0 < jod) & (jod < 10)).all()
    assert (gt is not None) == (wrt in ("test", "both")) and (gr is not None) == (wrt in ("reference", "both"))
    for g, size in ((gt, tsize), (gr, rsize)):
        if g is not None:
            assert g.shape == (ic.B, C, *size[::-1]) and np.isfinite(g).all() and g.any()
    want = {name + "_jod"} | {name + "_grad_" + k for k, g in (("test", gt), ("reference", gr)) if g is not None}
    assert set(np.load(path).files) == want                                          # outputs only


# ---- the bounds see a wrong kernel ---------------------------------------------------------------------------------------------------
def _luminance(frame, size, ph, wgt, F, resize):
    """resize_ref.luminance with the resize handed in."""
    v = np.clip(resize(rref.unit(frame, F)), F(0), F(1)).astype(F)
    L, _ = ph.forward(v[None, :, None])
    if v.shape[0] == 3:
        L = L[:, 0:1] * F(wgt[0]) + L[:, 1:2] * F(wgt[1]) + L[:, 2:3] * F(wgt[2])
    return L[0, 0, 0].astype(F)


def _bilinear_without_the_half(x, size):
    """Bilinear with the source coordinate scale * (o + 0.5) in the place of scale * (o + 0.5) - 0.5."""
    def matrix(n_in, n_out):
        src = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out), 0.0)
        i0 = np.minimum(np.floor(src).astype(int), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        A = np.zeros((n_out, n_in))
        np.add.at(A, (np.arange(n_out), i0), 1.0 - (src - i0))
        np.add.at(A, (np.arange(n_out), i1), src - i0)
        return A
    h, w = x.shape[-2:]
    return np.matmul(np.matmul(matrix(h, size[1]), x), matrix(w, size[0]).T)


def test_ingest_bound_sees_a_shifted_source_coordinate():
    """The bound of the GPU test of the ingest (4 x the float32 restatement's own error) against a restatement whose bilinear
    source coordinate misses its -0.5."""
    import copy
    c = next(c for c in ic.rotation() if c["mode"] == "bilinear" and c["source"] != c["target"])
    test, _ = ic.rotation_inputs(c)
    ph64, ph32 = copy.copy(yref.photometry_for(c["display"])), copy.copy(yref.photometry_for(c["display"]))
    ph64.dtype, ph32.dtype = np.float64, np.float32
    a = (test[0], c["target"], c["mode"])
    R64 = rref.luminance(*a, ph64, rgb2y(), np.float64)
    R32 = rref.luminance(*a, ph32, rgb2y(), np.float32)
    same = _luminance(test[0], c["target"], ph64, rgb2y(), np.float64, lambda x: rref.resize(x, c["target"], c["mode"]))
    assert np.array_equal(same, R64)                                                  # the local copy is the restatement
    wrong = _luminance(test[0], c["target"], ph64, rgb2y(), np.float64, lambda x: _bilinear_without_the_half(x, c["target"]))
    e_ref = yref.channel_error(R32, R64, R64)
    err = yref.channel_error(wrong, R64, R64)
    print("\ningest %s: e_ref %.3g bound %.3g, without the -0.5: %.3g" % (ic.case_id(c), e_ref, yref.error_bound(e_ref), err))
    assert e_ref <= 1e-4 and err > 100 * yref.error_bound(e_ref)


def test_level0_bound_sees_a_missing_reduce_term():
    """The bound of the GPU test of the level-0 luminance gradient against a gL without Reduce^T(GG_1): fixed GL_0 and GG_1 from a
    seeded generator, the sweep's restatement of tests/pyramid_grad_ref.py, and the comparison that test makes -- the pointwise
    adjoint of the candidate gL against the gradient of the true one, per sample and relative to the absolute term."""
    Wo, Ho = 122, 68
    rng = np.random.default_rng(2626)
    GL0 = torch.from_numpy(rng.standard_normal((ic.B, Ho, Wo)))
    GG1 = torch.from_numpy(rng.standard_normal((ic.B, (Ho + 1) // 2, (Wo + 1) // 2)))
    g_true = pgr.level0(GL0, GG1)[0].numpy()
    image = rng.uniform(0.05, 1.0, (3, Ho, Wo)).astype(np.float32)
    kind, kw = rref.eotf_args(yref.photometry_for("standard_fhd"))

    def adjoint(gL, dtype=np.float64, absolute=False):
        return rref.resize_adjoint(gL, image, (Wo, Ho), "bilinear", rgb2y(), kind, dtype=dtype, absolute=absolute, **kw)

    existing = adjoint(g_true[0].astype(np.float32), np.float32)                     # what the existing entry point returns
    for name, gL, must_pass in (("the true gL", g_true[0], True), ("GL_0 alone", GL0[0].numpy(), False)):
        gL = gL.astype(np.float32)
        g64, g32, S = adjoint(gL), adjoint(gL, np.float32), adjoint(gL, absolute=True)
        assert (S > 0).all()
        e_ref = float((np.abs(g32 - g64) / S).max())
        err = float((np.abs(existing - g64) / S).max())
        print("\nlevel 0, %s: err %.3g e_ref %.3g bound %.3g" % (name, err, e_ref, yref.error_bound(e_ref)))
        assert (err <= yref.error_bound(e_ref)) == must_pass
        if not must_pass:
            assert err > 100 * yref.error_bound(e_ref)
