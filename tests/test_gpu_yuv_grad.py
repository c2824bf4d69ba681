"""GPU: planar YUV clips of float32 code values (include/fvvdp_hip_yuv_grad.h, fvvdp.jod_video_yuv).

  1. the ingest, per pixel: level 0 after fvvdp_temporal_channels_yuv_planes against yuv_channels_ref.yuv_temporal_channels in
     float64, with the bound of the integer YUV pixel test (4 x the float32 chain's own error);
  2. the unpack's adjoint alone: fvvdp_yuv_grad_planes against yuv_grad_ref in float64 on a random gL, the same construction of
     the bound relative to the sum of the absolute terms of every output sample;
  3. the luminance transpose: fvvdp_video_grad_luminance against video_grad_input_ref.dlum with its derived bound;
  4. end to end: the value under no_grad, against predict_video_source on the integer codes, the gradients against the g24
     goldens of the reference's autograd, the identical clip;
  5. invariance: grad_batch, tuple and packed forms, host-resident inputs, requires_grad on Y only.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd.fvvdp import window_frame_indices
from fovvideovdp_amd.grad_passes import _fold_arrays, fold_list

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_grad_input_ref as vref          # noqa: E402
import yuv_channels_ref as yref              # noqa: E402
import yuv_grad_cases as yc                  # noqa: E402
import yuv_grad_ref as gref                  # noqa: E402
from lowlevel import Pipeline                # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U24 = 2.0 ** -24
I32P = C.POINTER(C.c_int32)


def product_photometry(model):
    if model == "gamma2.4":
        return dict(display_photometry=fv.fvvdp_display_photo_eotf(200, contrast=1000, EOTF="gamma", gamma=2.4, E_ambient=250,
                                                                   k_refl=0.005))
    return dict(display_name=model)


def stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def yuv_format(bd, css, M):
    fmt = nat.YuvFormat()
    fmt.bit_depth, fmt.chroma_420 = bd, 1 if css == "420" else 0
    for i, v in enumerate(np.asarray(M, np.float32).reshape(-1)):
        fmt.ycbcr2rgb[i] = float(v)
    return fmt


def device_planes(packed, H, W, css, form):
    """(fvvdp_yuv_planes, tensors to keep alive) of a packed float32 [N, frame_elems] clip laid out as `form`: "packed" (three
    pointers into one tensor), "planes" (three tensors), "padded" (three tensors, frames 8 / 4 / 12 samples further apart than the
    plane)."""
    (_, _), (uvh, uvw) = yc.plane_shapes(H, W, css)
    hw, uv = H * W, uvh * uvw
    if form == "packed":
        t = torch.from_numpy(np.ascontiguousarray(packed)).to(DEV)
        return nat.YuvPlanes(t.data_ptr(), t.data_ptr() + 4 * hw, t.data_ptr() + 4 * (hw + uv), t.shape[1], t.shape[1]), [t]
    pad = (8, 4) if form == "padded" else (0, 0)
    keep = []
    for part, n, extra in ((packed[:, :hw], hw, pad[0]), (packed[:, hw:hw + uv], uv, pad[1]), (packed[:, hw + uv:], uv, pad[1])):
        buf = torch.full((packed.shape[0], n + extra), float("nan"), dtype=torch.float32, device=DEV)
        buf[:, :n] = torch.from_numpy(np.ascontiguousarray(part)).to(DEV)
        keep.append(buf)
    return nat.YuvPlanes(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), hw + pad[0], uv + pad[1]), keep


# ---- 1. the ingest, per pixel ------------------------------------------------------------------------------------------------
# {4:2:0, 4:4:4} x {sRGB, PQ, gamma} x rings 8 / 16 / 32; the sizes, paddings, layouts and matrices rotate through them
# (a context has no band below 4 x 4 pixels -- fvvdp_ctx_create refuses 2 x 2 --, so 4 x 4 is the smallest frame an ingest can see;
# the adjoint, which needs no context, is run at 2 x 2 below)
INGEST_SIZES = {"420": [(4, 4), (8, 16), (68, 120), (68, 122)], "444": [(4, 6), (8, 16), (67, 121), (68, 120)]}
INGEST = []
for ci, css in enumerate(("420", "444")):
    for mi, model in enumerate(("standard_fhd", "standard_hdr_pq", "gamma2.4")):
        for fi, fps in enumerate((30, 60, 120)):
            k = 9 * ci + 3 * mi + fi
            H, W = INGEST_SIZES[css][(mi + fi + ci) % 4]
            INGEST.append(pytest.param(css, model, fps, H, W, (8, 10)[(mi + fi) % 2], ("bt709", "bt2020nc")[k % 2],
                                       ("replicate", "circular", "pingpong")[k % 3], ("packed", "planes", "padded")[(k // 2) % 3],
                                       id="%s-%s-%dfps-%dx%d-%s-%s" % (css, model, fps, H, W, ("replicate", "circular", "pingpong")[k % 3],
                                                                       ("packed", "planes", "padded")[(k // 2) % 3])))


def test_ingest_cases_cover_the_matrix():
    v = [p.values for p in INGEST]
    assert {(c[0], c[1], c[2]) for c in v} == {(s, m, f) for s in ("420", "444") for m in ("standard_fhd", "standard_hdr_pq", "gamma2.4")
                                               for f in (30, 60, 120)}
    assert {c[7] for c in v} == {"replicate", "circular", "pingpong"} and {c[8] for c in v} == {"packed", "planes", "padded"}
    assert {(c[0], c[3], c[4]) for c in v} >= {("420", 4, 4), ("420", 8, 16), ("420", 68, 120), ("420", 68, 122), ("444", 67, 121)}


@pytest.mark.parametrize("css,model,fps,H,W,bd,matrix,padding,form", INGEST)
def test_ingest_per_pixel(css, model, fps, H, W, bd, matrix, padding, form):
    m = fv.fvvdp(temp_padding=padding, quiet=True, device=DEV, **product_photometry(model))
    fl, taps = m._temporal_taps(fps)
    N = (8 if fl <= 8 else 16 if fl <= 16 else 32) + 3
    test, ref, _ = yc.fractional_clip(N, H, W, bd, css, matrix, [H, W, bd, int(css), fps])
    M = np.asarray(yref.MATRICES[matrix], np.float32)
    ph = yref.photometry_for(model)
    rgb2y = yref.orc.load_defaults()["color_spaces.json"]["BT.2020" if matrix == "bt2020nc" else "sRGB"]["RGB2Y"]
    idx = yref.orc.window_frame_indices(N, fl, padding)
    args = (test, ref, W, H, bd, css, M, ph, rgb2y, taps, idx)
    R64, S64 = yref.yuv_temporal_channels(*args, dtype=np.float64)
    R32, _ = yref.yuv_temporal_channels(*args, dtype=np.float32)
    pipe = Pipeline(m, W, H, 4, N)
    try:
        tp, keep_t = device_planes(test, H, W, css, form)
        rp, keep_r = device_planes(ref.astype(np.float32), H, W, css, "packed" if form == "planes" else "planes")
        fmt = yuv_format(bd, css, M)
        _, e = m._image_eotf(torch.float32)
        w = np.asarray(rgb2y, np.float32)
        widx = np.ascontiguousarray(window_frame_indices(N, fl, padding), dtype=np.int32)
        assert np.array_equal(np.stack([widx[f:f + fl] for f in range(N)]), idx)
        oob = torch.zeros(1, dtype=torch.int32, device=DEV)
        nat.check(nat.lib().fvvdp_temporal_channels_yuv_planes(pipe.handle, C.byref(tp), C.byref(rp), C.byref(fmt), C.byref(e),
                                                               nat.fptr(w), widx.ctypes.data_as(I32P), nat.fptr(taps), fl, N, 0,
                                                               C.c_void_p(oob.data_ptr()), stream()))
        R = pipe.export_level(0, N).cpu().numpy()
    finally:
        pipe.close()
    assert int(oob.item()) == 0                              # RGB is clipped before the display model
    err, e_ref = yref.assert_channels_close(R, R32, R64, S64, label="%s %s %d fps %dx%d" % (css, model, fps, H, W))
    print("\nyuv-planes ingest %s %s fl %d %dx%d %s: err %.3g e_ref %.3g bound %.3g" % (css, model, fl, H, W, form, err, e_ref,
                                                                                         yref.error_bound(e_ref)))


# ---- 2. the unpack's adjoint alone ---------------------------------------------------------------------------------------------
# 4:2:0: 2x2; smaller than one 64 x 32 tile; W and H one chroma sample below and above a tile multiple in each axis; 4:4:4 at odd sizes
ADJOINT = [("420", 2, 2, "standard_fhd", "planes"), ("420", 20, 30, "standard_hdr_pq", "packed"),
           ("420", 30, 62, "gamma2.4", "planes"), ("420", 34, 66, "standard_fhd", "padded"),
           ("420", 62, 130, "standard_hdr_pq", "planes"), ("420", 66, 126, "standard_fhd", "packed"),
           ("444", 33, 67, "standard_fhd", "planes"), ("444", 5, 3, "gamma2.4", "padded"), ("444", 31, 65, "standard_hdr_pq", "packed")]


@pytest.mark.parametrize("css,H,W,model,form", ADJOINT, ids=["%s-%dx%d-%s-%s" % c for c in ADJOINT])
def test_unpack_adjoint_per_sample(css, H, W, model, form):
    """Bound, per output sample and relative to the sum of the absolute values of its terms as the float64 reference gives it:
    4 x max(the same error of the float32 restatement, 4 x 2^-24) -- yuv_channels_ref.error_bound's construction."""
    N, bd, matrix = 3, 10 if "pq" in model else 8, "bt2020nc" if "pq" in model else "bt709"
    m = fv.fvvdp(quiet=True, device=DEV, **product_photometry(model))
    test, _, _ = yc.fractional_clip(N, H, W, bd, css, matrix, [7, H, W, int(css)])
    M = np.asarray(yref.MATRICES[matrix], np.float32)
    rgb2y = np.asarray(yref.orc.load_defaults()["color_spaces.json"]["BT.2020" if matrix == "bt2020nc" else "sRGB"]["RGB2Y"], np.float32)
    kind, kw = gref.eotf_args(yref.photometry_for(model))
    rng = np.random.default_rng(H * W)
    gL = (rng.uniform(0.25, 2.0, (N, H, W)) * rng.choice([-1.0, 1.0], (N, H, W))).astype(np.float32)
    planes = yc.split(test, H, W, css)
    ref64, ref32, scale = [], [], []
    for f in range(N):
        a = (gL[f], planes[0][f], planes[1][f], planes[2][f], bd, css, M, rgb2y, kind)
        ref64.append(gref.unpack_adjoint(*a, dtype=np.float64, **kw))
        ref32.append(gref.unpack_adjoint(*a, dtype=np.float32, **kw))
        scale.append(gref.unpack_adjoint(*a, dtype=np.float64, absolute=True, **kw))
    tp, keep = device_planes(test, H, W, css, form)
    (_, _), (uvh, uvw) = yc.plane_shapes(H, W, css)
    _, e = m._image_eotf(torch.float32)
    fmt = yuv_format(bd, css, M)
    gLd = torch.from_numpy(gL).to(DEV)

    def run():
        out = [torch.full((N, H * W + 4), float("nan"), device=DEV), torch.full((N, uvh * uvw + 8), float("nan"), device=DEV),
               torch.full((N, uvh * uvw + 8), float("nan"), device=DEV)]
        gp = nat.YuvPlanes(out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), H * W + 4, uvh * uvw + 8)
        nat.check(nat.lib().fvvdp_yuv_grad_planes(W, H, N, C.c_void_p(gLd.data_ptr()), C.byref(tp), C.byref(gp), C.byref(fmt),
                                                  C.byref(e), nat.fptr(rgb2y), stream()))
        res = [o.cpu().numpy() for o in out]
        assert all(np.isnan(r[:, n:]).all() for r, n in zip(res, (H * W, uvh * uvw, uvh * uvw)))    # the padding is not written
        return [res[0][:, :H * W].reshape(N, H, W), res[1][:, :uvh * uvw].reshape(N, uvh, uvw), res[2][:, :uvh * uvw].reshape(N, uvh, uvw)]

    got = run()
    again = run()
    for p in range(3):
        assert np.array_equal(got[p].view(np.uint32), again[p].view(np.uint32))                     # equal bits on a second run
        g64 = np.stack([ref64[f][p] for f in range(N)])
        g32 = np.stack([ref32[f][p] for f in range(N)])
        S = np.stack([scale[f][p] for f in range(N)])
        assert np.isfinite(got[p]).all()
        zero = S == 0                                       # a bound clamp (or every RGB value clipped): exact zeros
        assert (got[p][zero] == 0).all() and (g64[zero] == 0).all()
        assert zero.any() or H * W <= 16
        e_ref = float((np.abs(g32.astype(np.float64) - g64)[~zero] / S[~zero]).max())
        err = float((np.abs(got[p].astype(np.float64) - g64)[~zero] / S[~zero]).max())
        bound = yref.error_bound(e_ref)
        print("\nyuv adjoint %s %dx%d %s plane %s: err %.3g e_ref %.3g bound %.3g, %d exact zeros" % (css, H, W, model, "YUV"[p], err, e_ref,
                                                                                                      bound, int(zero.sum())))
        assert err <= bound, "plane %s: %.3g > %.3g" % ("YUV"[p], err, bound)


# ---- 3. the luminance transpose ---------------------------------------------------------------------------------------------------
LUM = [(8, 11, "replicate", 16, 8), (9, 12, "circular", 16, 8), (16, 5, "pingpong", 30, 20), (17, 20, "replicate", 30, 20),
       (32, 35, "circular", 16, 8), (33, 7, "pingpong", 16, 8), (64, 66, "replicate", 10, 6), (15, 19, "circular", 11, 7),
       (30, 9, "pingpong", 9, 13), (6, 9, "replicate", 7, 5), (60, 5, "circular", 7, 5)]


@pytest.mark.parametrize("fl,N,padding,W,H", LUM, ids=["fl%d-N%d-%s-%dx%d" % c for c in LUM])
def test_luminance_transpose(fl, N, padding, W, H):
    """video_grad_input_ref.dlum is the float64 reference with C = 1 and a display derivative of one; its derived bound
    (3 fl + 6) 2^-24 sum |tap g0| applies (test_gpu_video_grad_input.test_transpose_per_sample)."""
    HW = W * H
    rng = np.random.default_rng(100 * fl + N)
    taps = rng.standard_normal((2, fl)).astype(np.float32)
    g0 = rng.standard_normal((N, 2, HW)).astype(np.float32)
    idx = window_frame_indices(N, fl, padding)
    ff, fp = _fold_arrays(fold_list(idx, fl, N))
    g0d = torch.from_numpy(g0).to(DEV)
    gL = torch.full((N * HW + 64,), float("nan"), device=DEV)
    head = torch.full((fl * HW + 64,), float("nan"), device=DEV)
    nat.check(nat.lib().fvvdp_video_grad_luminance(W, H, N, C.c_void_p(g0d.data_ptr()), ff.ctypes.data_as(I32P), fp.ctypes.data_as(I32P),
                                                   nat.fptr(taps), fl, C.c_void_p(gL.data_ptr()), C.c_void_p(head.data_ptr()),
                                                   fl * HW * 4, stream()))
    out = gL.cpu().numpy()
    assert np.isnan(out[N * HW:]).all() and bool(torch.isnan(head[fl * HW:]).all())
    got = out[:N * HW].reshape(N, HW)
    ref, S = vref.dlum(idx, taps, g0), vref.dlum(idx, taps, g0, absolute=True)
    assert np.isfinite(got).all()
    zero = S == 0
    assert (got[zero] == 0).all()
    if padding == "circular" and N > fl + 1:
        assert zero[0].all()
    err = np.abs(got.astype(np.float64) - ref)
    bound = (3 * fl + 6) * U24 * S
    print("\nluminance transpose fl %d N %d %s: worst err / bound %.3f" % (fl, N, padding, float((err[~zero] / bound[~zero]).max())))
    assert (err <= bound).all()


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------
def case_metric(name, **kw):
    N, H, W, bd, css, cs, display, fps, padding, opt = yc.CASES[name]
    extra = {}
    if "photometry" in opt:
        extra["display_photometry"] = fv.fvvdp_display_photo_eotf(**opt["photometry"])
    return fv.fvvdp(display_name=display, foveated=bool(opt.get("foveated")), temp_padding=padding, quiet=True, device=DEV, **extra, **kw)


def case_call(m, name, test, ref, **kw):
    N, H, W, bd, css, cs, display, fps, padding, opt = yc.CASES[name]
    gaze = yc.case_gaze(name)
    return m.jod_video_yuv(test, ref, frames_per_second=fps, bit_depth=bd, chroma_ss=css, color_space=cs,
                           fixation_point=None if gaze is None else torch.from_numpy(gaze), **kw)


def case_planes(name, requires_grad=True, device=DEV):
    N, H, W, bd, css = yc.CASES[name][:5]
    test, ref = yc.case_inputs(name)
    t = tuple(torch.from_numpy(np.ascontiguousarray(p)).to(device).requires_grad_(requires_grad) for p in yc.split(test, H, W, css))
    return t, torch.from_numpy(ref.astype(np.int32)).to(device)


# max |g - g_ref| / max |g_ref| per plane against the reference's autograd: 3 x the value MEASURED on MI355X
# measured, worst plane: a 3.7e-5, b 6.1e-5, c 2.1e-5, d 2.6e-4 (the foveated case, as in the video path), e 1.4e-5
GOLDEN_TOL = {"a_420_srgb_30": 1.1e-4, "b_420_pq_60_circular": 1.8e-4, "c_444_gamma_24_pingpong": 6.3e-5, "d_420_fov": 7.8e-4,
              "e_420_120": 4.3e-5}
# |JOD - predict_video_source's| on the integer codes: 3 x the value MEASURED on MI355X
# measured: 0 (sRGB 4:2:0), 1.9e-6 (PQ 10 bit), 9.5e-7 (gamma 4:4:4)
PARITY_TOL = 5.7e-6


@pytest.mark.parametrize("name", sorted(GOLDEN_TOL))
def test_gradients_against_the_reference(name):
    N, H, W, bd, css = yc.CASES[name][:5]
    m = case_metric(name)
    t, r = case_planes(name)
    jod = case_call(m, name, t, r, width=W, height=H)
    assert jod.dim() == 0 and jod.dtype is torch.float32 and jod.grad_fn is not None
    with torch.no_grad():
        again = case_call(m, name, tuple(p.detach() for p in t), r, width=W, height=H)
    assert again.grad_fn is None and torch.equal(jod.detach(), again)               # the value does not depend on grad mode
    jod.backward()
    want_jod, *want = yc.load_golden(name)
    print("\n%s: JOD %.6f reference %.6f" % (name, float(jod), want_jod))
    assert abs(float(jod) - want_jod) <= 1e-3                                       # the project's parity bound
    for p, g, gr in zip("YUV", (x.grad for x in t), want):
        g = g.cpu().numpy()
        assert np.isfinite(g).all() and g.shape == gr.shape
        rel = float(np.abs(g - gr).max() / np.abs(gr).max())
        print("%s d%s: max|g - g_ref| / max|g_ref| = %.3e (max|g_ref| %.3e)" % (name, p, rel, float(np.abs(gr).max())))
        assert rel <= GOLDEN_TOL[name], (p, rel)
        assert (g[gr == 0] == 0).all()              # bound clamps and frames no window shows: exact zeros on both sides


def test_value_against_the_integer_source():
    """The same clip as integer codes through predict_video_source: the two ingest kernels share a contract, not a summation
    order, so this is a measured difference."""
    worst = 0.0
    for name in ("a_420_srgb_30", "b_420_pq_60_circular", "c_444_gamma_24_pingpong"):
        N, H, W, bd, css, cs, display, fps, padding, opt = yc.CASES[name]
        _, ref = yc.case_inputs(name)
        codes, _ = yref.yuv_clip(N, H, W, bd, css, 991)
        m = case_metric(name)
        vs = fv.fvvdp_video_source_yuv_frames(codes.copy(), ref.copy(), fps, W, H, bit_depth=bd, chroma_ss=css, color_space=cs,
                                              display_photometry=m.display_photometry)
        q, _ = m.predict_video_source(vs)
        jod = m.jod_video_yuv(torch.from_numpy(codes.astype(np.float32)), torch.from_numpy(ref.astype(np.int32)), frames_per_second=fps,
                              width=W, height=H, bit_depth=bd, chroma_ss=css, color_space=cs)
        d = abs(float(q) - float(jod))
        print("\n%s: predict_video_source %.7f jod_video_yuv %.7f difference %.3g" % (name, float(q), float(jod), d))
        worst = max(worst, d)
    assert worst <= PARITY_TOL


def test_identical_clip_gives_zeros():
    name = "f_identical"
    t, r = case_planes(name)
    jod = case_call(case_metric(name), name, t, r)
    jod.backward()
    assert float(jod) == 10.0
    for p in t:
        assert bool(torch.isfinite(p.grad).all()) and bool((p.grad == 0).all())


# ---- 5. invariance -----------------------------------------------------------------------------------------------------------------
def test_grad_batch_forms_and_placement_give_equal_bits():
    name = "a_420_srgb_30"
    N, H, W, bd, css = yc.CASES[name][:5]
    test, ref = yc.case_inputs(name)
    grads = {}
    for gb in (None, 1, 2):
        m = case_metric(name)
        m.grad_batch = gb
        t, r = case_planes(name)
        case_call(m, name, t, r).backward()
        grads[gb] = torch.cat([p.grad.reshape(N, -1) for p in t], 1)
    assert torch.equal(grads[None], grads[1]) and torch.equal(grads[None], grads[2])
    # the packed form: one tensor, one gradient with the same bits
    m = case_metric(name)
    packed = torch.from_numpy(test.copy()).to(DEV).requires_grad_(True)
    jp = case_call(m, name, packed, torch.from_numpy(ref.astype(np.int32)), width=W, height=H)
    jp.backward()
    assert packed.grad.shape == packed.shape and torch.equal(packed.grad, grads[None])
    # a host-resident input gets its gradient on the host
    th, rh = case_planes(name, device="cpu")
    jh = case_call(m, name, th, rh)
    jh.backward()
    assert torch.equal(jh, jp) and all(p.grad.device.type == "cpu" for p in th)
    assert torch.equal(torch.cat([p.grad.reshape(N, -1) for p in th], 1), grads[None].cpu())
    # requires_grad on Y only
    ty, _ = case_planes(name)
    planes = (ty[0], ty[1].detach(), ty[2].detach())
    case_call(m, name, planes, rh).backward()
    assert planes[1].grad is None and planes[2].grad is None
    assert torch.equal(planes[0].grad.reshape(N, -1), grads[None][:, :H * W])
    # planes whose rows are not contiguous are made contiguous inside autograd
    wide = torch.zeros((N, H, W + 3), device=DEV)
    wide[:, :, :W] = ty[0].detach()
    wide.requires_grad_(True)
    case_call(m, name, (wide[:, :, :W], planes[1], planes[2]), rh).backward()
    assert torch.equal(wide.grad[:, :, :W], planes[0].grad) and bool((wide.grad[:, :, W:] == 0).all())
    # double backward is refused: the gradient carries no graph (once_differentiable)
    t2, _ = case_planes(name)
    j2 = case_call(m, name, t2, rh)
    (gy,) = torch.autograd.grad(j2, t2[0], create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):
        gy.sum().backward()
