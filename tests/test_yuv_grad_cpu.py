"""Differentiable planar-YUV clips without a GPU: the header and its binding, the argument checks of its entry points, every refusal
of fvvdp.jod_video_yuv that comes before any device work, the float64 restatement of the unpack's adjoint (tests/yuv_grad_ref.py)
against the inner-product identity and against torch autograd, the margin of the golden inputs, the code objects of the new
kernels, and the goldens."""
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
import yuv_channels_ref as yref              # noqa: E402
import yuv_grad_cases as yc                  # noqa: E402
import yuv_grad_ref as gref                  # noqa: E402

# both sides float64 and analytic (test_diff_map_cpu.py's bound for the same purpose)
ADJOINT_BOUND = 1e-12
NEW_KERNELS = ["yuv_adjoint_420_kernel", "yuv_adjoint_444_kernel"] + \
    ["void yuvplanes_ring_kernel<%d, %d>" % c for c in ((8, 2), (16, 2), (32, 1))] + \
    ["void yuvplanes_vec_kernel<%d, %s>" % (fl, c) for fl in (8, 16) for c in ("true", "false")] + \
    ["void video_lum_input_kernel<%d, %d>" % c for c in ((8, 4), (8, 1), (16, 4), (16, 1), (32, 2), (32, 1), (64, 2), (64, 1))]


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def test_yuv_grad_header_is_exported_and_bound():
    nat.build()
    names = declared("fvvdp_hip_yuv_grad.h")
    assert names == ["fvvdp_temporal_channels_yuv_planes", "fvvdp_video_grad_luminance", "fvvdp_yuv_grad_planes"]
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert sorted(nat.YUV_GRAD_SYMBOLS) == names
    assert len(declared("fvvdp_hip.h")) == 24
    lib = nat.lib()
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    assert not hasattr(L, "fvvdp_ctx_ingest_begin")                         # the context's side of the ingest stays internal
    txt = open(os.path.join(ROOT, "include", "fvvdp_hip_yuv_grad.h")).read()
    assert int(re.search(r"#define FVVDP_YUV_GRAD_MAX_TAPS (\d+)", txt).group(1)) == nat.YUV_GRAD_MAX_TAPS
    assert ctypes.sizeof(nat.YuvPlanes) == 40 and ctypes.sizeof(nat.YuvFormat) == 44      # fvvdp_yuv_format keeps its layout
    assert callable(fv.fvvdp.jod_video_yuv)


def _fmt(bd=8, c420=1):
    fmt = nat.YuvFormat()
    fmt.bit_depth, fmt.chroma_420 = bd, c420
    return fmt


def test_argument_checks_need_no_device():
    lib = nat.lib()
    p = ctypes.c_void_p
    i32p = ctypes.POINTER(ctypes.c_int32)
    e = nat.Eotf()
    e.kind = nat.EOTF_SRGB
    w = np.ones(3, np.float32)
    W, H, N = 64, 48, 5
    HW, UV = W * H, W * H // 4

    def planes(y=256, u=512, v=768, ls=HW, cs=UV):
        return nat.YuvPlanes(y, u, v, ls, cs)

    # the adjoint of the unpack
    def adj(gL=256, t=None, g=None, fmt=None, kind=nat.EOTF_SRGB, width=W, height=H, n=N):
        e.kind = kind
        return lib.fvvdp_yuv_grad_planes(width, height, n, p(gL), ctypes.byref(t or planes()), ctypes.byref(g or planes()),
                                         ctypes.byref(fmt or _fmt()), ctypes.byref(e), nat.fptr(w), None)

    assert lib.fvvdp_yuv_grad_planes(W, H, N, None, None, None, None, None, None, None) == -1 and b"null" in lib.fvvdp_last_error()
    assert adj(width=0) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert adj(n=0) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert adj(fmt=_fmt(7)) == -1 and b"bit depth" in lib.fvvdp_last_error()
    assert adj(fmt=_fmt(17)) == -1 and b"bit depth" in lib.fvvdp_last_error()
    assert adj(width=63) == -1 and b"even frame dimensions" in lib.fvvdp_last_error()
    assert adj(height=47) == -1 and b"even frame dimensions" in lib.fvvdp_last_error()
    assert adj(kind=nat.EOTF_LUT) == -1 and b"closed-form" in lib.fvvdp_last_error()
    assert adj(kind=nat.EOTF_NONE) == -1 and b"closed-form" in lib.fvvdp_last_error()
    assert adj(t=planes(u=0)) == -1 and b"null plane pointer (test)" in lib.fvvdp_last_error()
    assert adj(g=planes(v=0)) == -1 and b"null plane pointer (gradient)" in lib.fvvdp_last_error()
    assert adj(t=planes(y=258)) == -1 and b"aligned to 4 bytes (test)" in lib.fvvdp_last_error()
    assert adj(g=planes(u=514)) == -1 and b"aligned to 4 bytes (gradient)" in lib.fvvdp_last_error()
    assert adj(t=planes(ls=HW - 1)) == -1 and b"luma_stride" in lib.fvvdp_last_error()
    assert adj(g=planes(cs=UV - 1)) == -1 and b"chroma_stride" in lib.fvvdp_last_error()
    assert adj(fmt=_fmt(8, 0), t=planes(cs=HW - 1)) == -1 and b"chroma_stride" in lib.fvvdp_last_error()      # 4:4:4: full-size chroma
    assert adj(gL=258) == -1 and b"d_gL" in lib.fvvdp_last_error()

    # the luminance transpose: the checks of fvvdp_video_grad_input
    def lum(fl=8, n=N, head=1 << 30, ff=None, fp=None, width=W, gL=256):
        k = max(1, min(fl, 256))
        ff = np.zeros(k, np.int32) if ff is None else np.asarray(ff, np.int32)
        fp = np.arange(k, dtype=np.int32) if fp is None else np.asarray(fp, np.int32)
        taps = np.ones((2, k), np.float32)
        return lib.fvvdp_video_grad_luminance(width, H, n, p(256), ff.ctypes.data_as(i32p), fp.ctypes.data_as(i32p), nat.fptr(taps), fl,
                                              p(gL), p(256), head, None)

    assert lib.fvvdp_video_grad_luminance(W, H, N, None, None, None, None, 8, None, None, 0, None) == -1 and b"null" in lib.fvvdp_last_error()
    assert lum(width=0) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert lum(fl=0) == -1 and b"filter length" in lib.fvvdp_last_error()
    assert lum(fl=257) == -1 and b"filter length" in lib.fvvdp_last_error()
    assert lum(fl=65) == nat.FVVDP_EUNSUPPORTED and b"64" in lib.fvvdp_last_error()
    assert lum(head=8 * HW * 4 - 1) == -1 and b"side buffer" in lib.fvvdp_last_error()
    assert lum(ff=[0] * 7 + [5]) == -1 and b"outside [0, 5)" in lib.fvvdp_last_error()
    assert lum(fp=[0, 1, 2, 3, 4, 5, 6, 6]) == -1 and b"listed twice" in lib.fvvdp_last_error()
    assert lum(ff=[1] + [0] * 7) == -1 and b"sorted" in lib.fvvdp_last_error()
    assert lum(gL=258) == -1 and b"aligned to 4 bytes" in lib.fvvdp_last_error()

    # the ingest: everything that is checked before the context is looked at (a context needs a device)
    taps = np.ones((2, 40), np.float32)
    idx = np.zeros(64, np.int32)

    def ing(ctx=256, t=None, r=None, fmt=None, kind=nat.EOTF_SRGB, fl=8, oob=256):
        e.kind = kind
        return lib.fvvdp_temporal_channels_yuv_planes(p(ctx), ctypes.byref(t or planes()), ctypes.byref(r or planes()),
                                                      ctypes.byref(fmt or _fmt()), ctypes.byref(e), nat.fptr(w),
                                                      idx.ctypes.data_as(i32p), nat.fptr(taps), fl, 4, 0, p(oob), None)

    assert ing(ctx=None) == -1 and b"null" in lib.fvvdp_last_error()
    assert ing(fmt=_fmt(20)) == -1 and b"bit depth" in lib.fvvdp_last_error()
    assert ing(fl=0) == -1 and b"filter length" in lib.fvvdp_last_error()
    assert ing(fl=33) == nat.FVVDP_EUNSUPPORTED and b"up to 32 taps" in lib.fvvdp_last_error()
    assert ing(kind=nat.EOTF_LUT) == -1 and b"closed-form" in lib.fvvdp_last_error()
    assert ing(kind=nat.EOTF_NONE) == -1 and b"closed-form" in lib.fvvdp_last_error()
    assert ing(oob=258) == -1 and b"d_oob_flag" in lib.fvvdp_last_error()
    assert ing(t=planes(y=0)) == -1 and b"null plane pointer (test)" in lib.fvvdp_last_error()
    assert ing(r=planes(v=770)) == -1 and b"aligned to 4 bytes (reference)" in lib.fvvdp_last_error()


def test_refusals_without_device():
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    N, H, W = 4, 32, 48
    Y, U, V = torch.rand(N, H, W) * 200 + 20, torch.rand(N, H // 2, W // 2) * 200 + 20, torch.rand(N, H // 2, W // 2) * 200 + 20
    t, r = (Y, U, V), (Y.clone(), U.clone(), V.clone())
    packed = torch.rand(N, H * W * 3 // 2) * 200 + 20
    call = m.jod_video_yuv
    with pytest.raises(RuntimeError, match="frame rate too high: its temporal filter has 33 taps"):
        call(t, r, frames_per_second=130)
    for bad in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(RuntimeError, match="needs float32 planes.*Half-precision and float64 planes are not supported"):
            call((Y.to(bad), U, V), r, frames_per_second=30)
        with pytest.raises(RuntimeError, match="needs float32 planes"):
            call(t, (Y, U.to(bad), V), frames_per_second=30)
    with pytest.raises(RuntimeError, match="needs float32 planes"):             # integer codes are for the reference only
        call(packed.to(torch.uint8), packed, frames_per_second=30, width=W, height=H)
    with pytest.raises(RuntimeError, match="4:2:0 video needs even width and height"):
        call((torch.rand(N, 33, W), U, V), r, frames_per_second=30)
    with pytest.raises(RuntimeError, match="4:2:0 video needs even width and height"):
        call(packed, packed, frames_per_second=30, width=47, height=H)
    with pytest.raises(RuntimeError, match="full_screen_resize is not differentiable"):
        call(t, r, frames_per_second=30, full_screen_resize="bilinear")
    with pytest.raises(RuntimeError, match="chroma planes of the test must be"):
        call((Y, U[:, :, :-1], V), r, frames_per_second=30)
    with pytest.raises(RuntimeError, match="chroma planes of the test must be"):
        call((Y, U, V), r, frames_per_second=30, chroma_ss="444")
    with pytest.raises(RuntimeError, match="exactly the same shape"):
        call(t, (Y[:3], U[:3], V[:3]), frames_per_second=30)
    with pytest.raises(RuntimeError, match="three planes"):
        call((Y, U), r, frames_per_second=30)
    with pytest.raises(RuntimeError, match="packed tensor needs width= and height="):
        call(packed, packed, frames_per_second=30)
    with pytest.raises(RuntimeError, match=r"packed test must be \[N, 2304\]"):
        call(packed[:, :-1], packed, frames_per_second=30, width=W, height=H)
    with pytest.raises(RuntimeError, match="not the width=50"):
        call(t, r, frames_per_second=30, width=50, height=H)
    with pytest.raises(RuntimeError, match="gradients with respect to the reference are not supported"):
        call(t, (Y.clone().requires_grad_(True), U, V), frames_per_second=30)
    with pytest.raises(RuntimeError, match="at least 2 frames"):
        call((Y[:1], U[:1], V[:1]), (Y[:1], U[:1], V[:1]), frames_per_second=30)
    with pytest.raises(RuntimeError, match="frames_per_second"):
        call(t, r)
    with pytest.raises(RuntimeError, match="4:2:2 is not"):
        call(t, r, frames_per_second=30, chroma_ss="422")
    with pytest.raises(RuntimeError, match="bit depth must be 8..16"):
        call(t, r, frames_per_second=30, bit_depth=7)
    # everything accepted (tuple, packed, integer reference codes): the first device work is refused on a CPU metric
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call((Y.clone().requires_grad_(True), U, V), r, frames_per_second=30)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(packed, packed.to(torch.uint8), frames_per_second=120, width=W, height=H)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(packed, (packed * 4).to(torch.int32).numpy().astype(np.uint16), frames_per_second=30, width=W, height=H, bit_depth=10)


def test_refuses_user_photometry():
    class MyDisplay(fv.fvvdp_display_photometry):
        def forward(self, V):
            return 100.0 * V + 0.5

        def get_peak_luminance(self):
            return 100.5

        def get_black_level(self):
            return 0.5

    m = fv.fvvdp(display_name="standard_4k", display_photometry=MyDisplay(), device="cpu", quiet=True)
    with pytest.raises(RuntimeError, match="jod_video_yuv needs a display model with a closed form"):
        m.jod_video_yuv(torch.rand(4, 48 * 32 * 3 // 2), torch.rand(4, 48 * 32 * 3 // 2), frames_per_second=30, width=48, height=32)


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uvh,uvw", [(1, 1), (2, 3), (5, 7)])
def test_chroma_transpose_is_the_adjoint_of_the_upsampling(uvh, uvw):
    """<A x, y> = <x, A^T y> on luma sizes 2x2, 4x6 and 10x14."""
    H, W = 2 * uvh, 2 * uvw
    rng = np.random.default_rng(H * W)
    x = rng.standard_normal((2, uvh, uvw))
    y = rng.standard_normal((2, H, W))
    lhs = float((yref.upsample_x2(x, H, W, np.float64) * y).sum())
    rhs = float((x * gref.upsample_t(y, uvh, uvw)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    # every column of the transpose sums the weights of one source sample: the upsampling of ones is ones
    assert np.allclose(gref.upsample_t(np.ones((1, H, W)), uvh, uvw).sum(), H * W, rtol=1e-14)


def _torch_luminance(Y, U, V, bd, css, M, rgb2y, ph):
    """fvvdp_video_source_yuv_frames.unpack's arithmetic on one frame of planes, then the oracle's photometry and luminance, in
    torch float64."""
    sc = 2 ** (bd - 8)
    Yf = torch.clip(Y * (1 / (sc * 219)) - 16 / 219, 0, 1)
    uv = torch.clip(torch.stack((U, V))[None] * (1 / (sc * 224)) - 128 / 224, -0.5, 0.5)
    if css == "420":
        uv = torch.nn.functional.interpolate(uv, scale_factor=2, mode='bilinear')
    Yuv = torch.cat((Yf[None], uv[0]), 0).permute(1, 2, 0)
    rgb = (Yuv @ torch.tensor(np.asarray(M, np.float64)).T).clip(0, 1)
    Yb = ph.get_black_level()
    if ph.EOTF == "sRGB":
        lin = torch.where(rgb > 0.04045, ((rgb + 0.055) / 1.055) ** 2.4, rgb / 12.92)
        L = (ph.Y_peak - Yb) * lin + Yb
    elif ph.EOTF == "gamma":
        L = (ph.Y_peak - Yb) * rgb ** ph.gamma + Yb
    else:
        n, m_ = gref.PQ_N, gref.PQ_M
        t = rgb ** (1 / m_)
        L = (10000 * (torch.clamp(t - gref.PQ_C1, min=0) / (gref.PQ_C2 - gref.PQ_C3 * t)) ** (1 / n)).clip(0.005, ph.Y_peak) + Yb
    return L[..., 0] * rgb2y[0] + L[..., 1] * rgb2y[1] + L[..., 2] * rgb2y[2]


@pytest.mark.parametrize("css,H,W,model,bd,matrix", [("420", 10, 14, "standard_fhd", 8, "bt709"), ("420", 4, 6, "standard_hdr_pq", 10, "bt2020nc"),
                                                    ("444", 5, 7, "gamma2.4", 8, "dense"), ("420", 2, 2, "gamma2.4", 12, "bt709"),
                                                    ("444", 9, 11, "standard_hdr_pq", 16, "bt2020nc")])
def test_adjoint_is_the_autograd_of_the_unpack(css, H, W, model, bd, matrix):
    test, _, _ = yc.fractional_clip(3, H, W, bd, css, matrix, [5, H, W])
    M = np.asarray(yref.MATRICES[matrix], np.float32)
    ph = yref.photometry_for(model, dtype=np.float64)
    rgb2y = np.asarray([0.2126, 0.7152, 0.0722], np.float32).astype(np.float64)
    kind, _ = gref.eotf_args(ph)
    kw = dict(Y_peak=float(ph.Y_peak), Y_black=float(ph.get_black_level()), gamma=float(ph.gamma))      # unrounded: both sides float64
    rng = np.random.default_rng(H + W)
    clamped = 0
    for f in range(3):
        Y, U, V = (p[f].astype(np.float64) for p in yc.split(test, H, W, css))
        gL = rng.standard_normal((H, W))
        planes = [torch.tensor(a, requires_grad=True) for a in (Y, U, V)]
        (_torch_luminance(*planes, bd, css, M.astype(np.float64), rgb2y, ph) * torch.tensor(gL)).sum().backward()
        got = gref.unpack_adjoint(gL, Y, U, V, bd, css, M.astype(np.float64), rgb2y, kind, dtype=np.float64, **kw)
        for g, p in zip(got, planes):
            want = p.grad.numpy()
            assert np.abs(g - want).max() <= ADJOINT_BOUND * max(np.abs(want).max(), 1e-300)
            assert np.array_equal(g == 0, want == 0)                               # exact zeros where a clamp binds, and only there
            clamped += int((want == 0).sum())
    assert clamped > 0 or H * W <= 4


def test_golden_inputs_keep_their_margin_and_rebuild():
    for name, (N, H, W, bd, css, cs, display, fps, padding, opt) in yc.CASES.items():
        test, ref = yc.case_inputs(name)
        again, ref2, _ = yc.fractional_clip(N, H, W, bd, css, cs, yc.SEEDS[name])
        assert test.dtype == np.float32 and test.shape == ref.shape and np.array_equal(ref, ref2)
        if opt.get("identical"):
            assert np.array_equal(test, ref.astype(np.float32))
            continue
        assert np.array_equal(test, again)
        frac = test.astype(np.float64) - np.floor(test.astype(np.float64))
        assert frac.min() >= 0.25 - 1e-3 and frac.max() <= 0.75 + 1e-3          # (float32 codes of up to 10 bits carry the fraction to 6e-5)
        M = np.asarray(yref.MATRICES[cs], np.float32)
        planes = yc.split(test, H, W, css)
        margin = min(float(gref.rgb_margin(planes[0][f], planes[1][f], planes[2][f], bd, css, M).min()) for f in range(N))
        print("%s: smallest distance of a pre-clip RGB value from 0, 1 and the sRGB toe: %.3g" % (name, margin))
        assert margin >= yc.RGB_MARGIN                                         # no sample is ever left out of a comparison
        top = (1 << bd) - 1
        assert (test[::3] < 16 * 2 ** (bd - 8)).any() and (test[::3] > min(240 * 2 ** (bd - 8), top)).any()     # the clamps do bind


@pytest.mark.parametrize("name", sorted(yc.CASES))
def test_goldens_load(name):
    N, H, W, bd, css = yc.CASES[name][:5]
    path = os.path.join(yc.GOLDEN, yc.FILES[name])
    assert os.path.getsize(path) < 1 << 20
    jod, dy, du, dv = yc.load_golden(name)
    (_, _), (uvh, uvw) = yc.plane_shapes(H, W, css)
    assert dy.shape == (N, H, W) and du.shape == dv.shape == (N, uvh, uvw)
    assert all(np.isfinite(g).all() for g in (dy, du, dv)) and 0 < jod <= 10
    if yc.CASES[name][9].get("identical"):
        assert jod == 10 and not dy.any() and not du.any() and not dv.any()
    else:
        assert dy.any() and du.any() and dv.any() and (dy == 0).any()          # illegal codes: exact zeros in the reference too


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
            assert (x["sgpr_spill_count"], x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), n
    assert found == {k: 1 for k in found}
    # none of the names the other tests count by substring
    for n in NEW_KERNELS:
        assert not any(s in n for s in ("temporal_vec_kernel<", "band2_kernel<", "band_kernel<", "temporal_ring_kernel<",
                                        "temporal_yuv_kernel<", "temporal_yuv_vec_kernel<", "video_input_kernel<"))
