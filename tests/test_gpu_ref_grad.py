"""wrt="reference" / wrt="both" of fvvdp.jod_images and fvvdp.jod_video on the GPU: gradients with respect to the reference
against the reference implementation's autograd (goldens g21 / g22) and against finite differences of the float64 CPU oracle,
exact zeros, the test gradient untouched by wrt="both", invariance (backward batch, run to run, layout, upstream weight), the
handling of `wrt`, host synchronisation and a short optimisation.

Tolerances are 3x the worst error measured on MI355X (the convention of test_gpu_video_grad.py); a measured reference-side
error above 5e-3 (3x the project's widest gradient tolerance, 1.6e-3 for foveated images) would be a bug, not a tolerance.
Measured max|g - gref| / max|gref|:
  images  a 3.9e-5, b 2.2e-5, c 3.6e-4, f 5.7e-4, g 0 (exact), i 7.1e-6
  clips   a 3.2e-5, b 2.0e-5, c 1.8e-5, d 5.5e-4, e 1.7e-4, h 7.5e-5, j 5.9e-5, k 2.1e-5, s 1.4e-5
The foveated cases (f, d) are the widest, as on the test side (5.1e-4 and 3.9e-4 there)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_cases as ic                    # noqa: E402
import video_grad_cases as vc              # noqa: E402
import ref_grad_cases as rc                # noqa: E402
from test_gpu_image_grad import GOLDEN_TOL as IMAGE_TEST_TOL        # noqa: E402   the existing g18 / g19 tolerances
from test_gpu_video_grad import GOLDEN_TOL as VIDEO_TEST_TOL       # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

IMAGE_TOL = {"a_gray_fhd": 1.2e-4, "b_rgb_4k_oob": 6.6e-5, "c_rgb_hdr_pq": 1.1e-3, "f_rgb_foveated": 1.72e-3, "g_identical": 0.0,
             "i_hdr_linear_dark": 2.2e-5}
VIDEO_TOL = {"a_gray_30_replicate": 9.6e-5, "b_rgb_60_circular": 5.9e-5, "c_gray_30_circular": 5.3e-5,
             "d_rgb_30_pingpong_fov": 1.64e-3, "e_rgb_pq_oob": 5.3e-4, "h_rgb_2f_120": 2.3e-4, "j_partly_identical": 1.8e-4,
             "k_gray_30_odd": 6.4e-5, "s_hdr_linear_dark": 4.3e-5}
# |<gref, d> - (JOD64(r+) - JOD64(r-))| / |JOD64(r+) - JOD64(r-)| with the REFERENCE perturbed: 3x the worst measured on MI355X
# (7.1e-5: the rgb 135x240 image; clips 6.0e-5 at most); the test side's bound, for comparison, is FD_TOL = 8.3e-4
# (test_gpu_video_grad.py)
REF_FD_TOL = 2.2e-4


def _metric(display, padding="replicate", opt=None):
    opt = opt or {}
    kw = {}
    if "photometry" in opt:
        kw["display_photometry"] = fv.fvvdp_display_photo_eotf(**opt["photometry"])
    return fv.fvvdp(display_name=display, foveated=bool(opt.get("foveated")), temp_padding=padding, quiet=True, device=DEV, **kw)


def _igrad(m, test, ref, wrt, fix=None, weights=None, dim_order="BCHW"):
    """(jod, dJOD/dtest or None, dJOD/dreference or None) of image stacks."""
    x = test.clone().requires_grad_(wrt != "reference")
    y = ref.clone().requires_grad_(wrt != "test")
    jod = m.jod_images(x, y, dim_order=dim_order, fixation_point=fix, wrt=wrt)
    (jod.sum() if weights is None else (weights * jod).sum()).backward()
    return jod.detach(), x.grad, y.grad


def _vgrad(m, test, ref, fps, wrt, fix=None, weight=None, dim_order="CFHW"):
    x = test.clone().requires_grad_(wrt != "reference")
    y = ref.clone().requires_grad_(wrt != "test")
    jod = m.jod_video(x, y, dim_order=dim_order, frames_per_second=fps, fixation_point=fix, wrt=wrt)
    (jod if weight is None else weight * jod).backward()
    return jod.detach(), x.grad, y.grad


def _against_golden(name, g, g_ref, tol, identical):
    g = g.cpu().numpy()
    assert g.shape == g_ref.shape and np.isfinite(g).all()
    gmax = float(np.abs(g_ref).max())
    err = float(np.abs(g - g_ref).max())
    print("%s: max|g - gref| = %.3e, max|gref| = %.3e, rel %.3e" % (name, err, gmax, err / max(gmax, 1e-30)))
    if identical:
        assert (g == 0).all() and (g_ref == 0).all()
    else:
        assert err <= tol * gmax
    return g


@pytest.mark.parametrize("name", sorted(rc.IMAGE_CASES))
def test_image_goldens(name):
    C, H, W, display, opt = rc.IMAGE_CASES[name]
    t, r = rc.image_inputs(name)
    jod_ref, g_ref = rc.load_image_golden(name)
    m = _metric(display, opt=opt)
    fix = opt.get("fix")
    T, R = torch.from_numpy(t[None]).to(DEV), torch.from_numpy(r[None]).to(DEV)
    jod, none, gr = _igrad(m, T, R, "reference", fix=fix)
    assert none is None and jod.requires_grad is False
    q_pi, _ = m.predict_images(T, R, fixation_point=fix)
    assert torch.equal(jod, q_pi) and abs(float(jod[0]) - jod_ref) < 2e-3, (jod, q_pi, jod_ref)
    g = _against_golden(name, gr[0], g_ref, IMAGE_TOL[name], bool(opt.get("identical")))
    # wrt="both": the same reference gradient and the test gradient of wrt="test", bit for bit
    jod_b, gt_b, gr_b = _igrad(m, T, R, "both", fix=fix)
    _, gt, _ = _igrad(m, T, R, "test", fix=fix)
    assert torch.equal(jod_b, jod) and torch.equal(gr_b, gr) and torch.equal(gt_b, gt)
    if name in rc.SHARED_IMAGE and not opt.get("identical"):          # still inside the existing g18 tolerance
        _, g18 = ic.load_golden(name)
        assert np.abs(gt_b[0].cpu().numpy() - g18).max() <= IMAGE_TEST_TOL[name] * np.abs(g18).max()
    if opt.get("oob"):                      # reference samples the display model clamps: exact zeros, here and in the golden
        oob = (r < 0) | (r > 1)
        assert oob.any() and (g[oob] == 0).all() and (g_ref[oob] == 0).all() and (g[~oob] != 0).any()
    if opt.get("identical"):
        assert (gt_b == 0).all()


@pytest.mark.parametrize("name", sorted(rc.VIDEO_CASES))
def test_video_goldens(name):
    C, N, H, W, fps, padding, display, opt = rc.VIDEO_CASES[name]
    t, r = rc.video_inputs(name)
    jod_ref, g_ref = rc.load_video_golden(name)
    m = _metric(display, padding, opt)
    fix = rc.video_gaze(name)
    T, R = torch.from_numpy(t).to(DEV), torch.from_numpy(r).to(DEV)
    jod, none, gr = _vgrad(m, T, R, fps, "reference", fix=fix)
    assert none is None and jod.dim() == 0
    q_p, _ = m.predict(T, R, dim_order="CFHW", frames_per_second=fps, fixation_point=fix)
    assert torch.equal(jod, q_p) and abs(float(jod) - jod_ref) < 2e-3, (jod, q_p, jod_ref)
    g = _against_golden(name, gr, g_ref, VIDEO_TOL[name], False)
    jod_b, gt_b, gr_b = _vgrad(m, T, R, fps, "both", fix=fix)
    _, gt, _ = _vgrad(m, T, R, fps, "test", fix=fix)
    assert torch.equal(jod_b, jod) and torch.equal(gr_b, gr) and torch.equal(gt_b, gt)
    if name in rc.SHARED_VIDEO:             # still inside the existing g19 tolerance
        _, g19 = vc.load_golden(name)
        assert np.abs(gt_b.cpu().numpy() - g19).max() <= VIDEO_TEST_TOL[name] * np.abs(g19).max()
    if opt.get("oob"):
        oob = (r < 0) | (r > 1)
        assert oob.any() and (g[oob] == 0).all() and (g_ref[oob] == 0).all()
    if name == "c_gray_30_circular":        # no temporal window shows frame 0
        assert (g_ref[:, 0] == 0).all() and (g[:, 0] == 0).all() and (g[:, 1:] != 0).any()
    # exact zeros wherever the reference implementation has them (j_partly_identical: output frames 0..2 see no difference and
    # send nothing back, but the reference's frames 0..2 still collect from the later output frames' windows: no zeros there)
    assert (g[g_ref == 0] == 0).all()


def test_identical_inputs_give_exact_zeros():
    for display, foveated in (("standard_4k", False), ("standard_4k", True)):
        m = _metric(display, opt={"foveated": foveated})
        t, _ = vc.case_inputs("j_partly_identical")
        T = torch.from_numpy(t).to(DEV)
        _, gt, gr = _vgrad(m, T, T.clone(), 30, "both")
        assert (gt == 0).all() and (gr == 0).all()
        _, gt, gr = _igrad(m, T[:, 0][None], T[:, 0][None].clone(), "both")
        assert (gt == 0).all() and (gr == 0).all()


def _synth_clip(C, N, H, W, seed):
    from fovvideovdp_amd.synth import synth_video_pair
    t8, r8 = synth_video_pair(N, H, W, C=C, seed_ref=seed, seed_test=seed + 7)
    return (t8[0].numpy().astype(np.float32) / np.float32(255.0), r8[0].numpy().astype(np.float32) / np.float32(255.0))


def _fd(g, t, r, predict, n_dirs, eps=3e-5, seed=0):
    """<gref, d> against a central difference of the float64 oracle with the REFERENCE perturbed, d = the realised r+ - r-."""
    assert np.isfinite(g).all()
    rng = np.random.default_rng(seed)
    worst = 0.0
    for _ in range(n_dirs):
        d = rng.standard_normal(r.shape)
        d[(r < 4 * eps) | (r > 1 - 4 * eps)] = 0.0          # stay clear of the display model's clamps
        rp = (r + eps * d).astype(np.float32)
        rm = (r - eps * d).astype(np.float32)
        dj = predict(t, rp) - predict(t, rm)
        lin = float((g * (rp.astype(np.float64) - rm.astype(np.float64))).sum())
        rel = abs(lin - dj) / abs(dj)
        worst = max(worst, rel)
        print("%s: <gref,d> %.6e  dJOD64 %.6e  rel %.3e" % (r.shape, lin, dj, rel))
    return worst


@pytest.mark.parametrize("C,N,H,W,display,padding,fps,n_dirs", [
    (1, 6, 68, 121, "standard_fhd", "replicate", 30, 2), (3, 5, 68, 121, "standard_4k", "circular", 60, 2),
    (3, 4, 135, 240, "standard_4k", "pingpong", 30, 1)])
def test_video_finite_differences_fp64_oracle(C, N, H, W, display, padding, fps, n_dirs):
    from oracle import fvvdp_oracle as orc
    t, r = _synth_clip(C, N, H, W, seed=H + W + N)
    m = _metric(display, padding)
    _, _, gr = _vgrad(m, torch.from_numpy(t).to(DEV), torch.from_numpy(r).to(DEV), fps, "reference")
    o = orc.Oracle(display, dtype=np.float64, temp_padding=padding)
    worst = _fd(gr.double().cpu().numpy(), t, r, lambda a, b: o.predict(a, b, dim_order="CFHW", frames_per_second=fps)[0], n_dirs)
    assert worst <= REF_FD_TOL


@pytest.mark.parametrize("C,H,W,display,n_dirs", [(1, 68, 121, "standard_fhd", 2), (3, 135, 240, "standard_4k", 2)])
def test_image_finite_differences_fp64_oracle(C, H, W, display, n_dirs):
    from oracle import fvvdp_oracle as orc
    t, r = _synth_clip(C, 1, H, W, seed=H + W)
    t, r = t[:, 0], r[:, 0]
    m = _metric(display)
    _, _, gr = _igrad(m, torch.from_numpy(t[None]).to(DEV), torch.from_numpy(r[None]).to(DEV), "reference")
    o = orc.Oracle(display, dtype=np.float64)
    worst = _fd(gr[0].double().cpu().numpy(), t, r, lambda a, b: o.predict(a[:, None], b[:, None], dim_order="CFHW")[0], n_dirs)
    assert worst <= REF_FD_TOL


def test_video_invariance():
    """The reference gradient does not depend on the backward batch, repeats bit for bit, reaches the caller's tensor whatever
    its layout or device, and scales linearly with the upstream weight."""
    t, r = _synth_clip(3, 7, 64, 96, seed=31)
    T, R = torch.from_numpy(t).to(DEV), torch.from_numpy(r).to(DEV)
    for padding in ("replicate", "circular", "pingpong"):
        m = _metric("standard_4k", padding)
        j0, _, g0 = _vgrad(m, T, R, 30, "reference")
        j1, _, g1 = _vgrad(m, T, R, 30, "reference")
        assert torch.equal(g0, g1) and torch.equal(j0, j1) and torch.isfinite(g0).all() and (g0 != 0).any()
        _, gt0, gb0 = _vgrad(m, T, R, 30, "both")
        for gb in (1, 3):
            m.grad_batch = gb
            _, _, gs = _vgrad(m, T, R, 30, "reference")
            _, gtb, gsb = _vgrad(m, T, R, 30, "both")
            assert torch.equal(gs, g0) and torch.equal(gsb, g0) and torch.equal(gtb, gt0), (padding, gb)
    m = _metric("standard_4k")
    _, _, g = _vgrad(m, T, R, 30, "reference")
    _, _, g4 = _vgrad(m, T, R, 30, "reference", weight=4.0)
    _, _, gh = _vgrad(m, T, R, 30, "reference", weight=-0.5)
    _, _, gz = _vgrad(m, T, R, 30, "reference", weight=0.0)
    assert torch.equal(g4, 4.0 * g) and torch.equal(gh, -0.5 * g) and (gz == 0).all()
    # host FHWC reference: the gradient lands on the host, in FHWC
    yh = torch.from_numpy(r).permute(1, 2, 3, 0).contiguous().requires_grad_(True)
    m.jod_video(torch.from_numpy(t).permute(1, 2, 3, 0).contiguous(), yh, dim_order="FHWC", frames_per_second=30,
                wrt="reference").backward()
    assert yh.grad.device.type == "cpu" and yh.grad.shape == yh.shape and torch.equal(yh.grad.permute(3, 0, 1, 2).to(DEV), g)
    # non-contiguous device view of a larger leaf
    base = torch.zeros((1, 3, 7, 64, 104), device=DEV)
    base[..., 4:100] = R
    base.requires_grad_(True)
    m.jod_video(T[None], base[..., 4:100], frames_per_second=30, wrt="reference").backward()
    assert torch.equal(base.grad[0, ..., 4:100], g) and (base.grad[..., :4] == 0).all() and (base.grad[..., 100:] == 0).all()


def test_image_invariance():
    m = _metric("standard_4k")
    t, r = _synth_clip(3, 5, 64, 96, seed=32)
    T = torch.from_numpy(np.ascontiguousarray(t.transpose(1, 0, 2, 3))).to(DEV)         # 5 pairs
    R = torch.from_numpy(np.ascontiguousarray(r.transpose(1, 0, 2, 3))).to(DEV)
    _, gt0, g0 = _igrad(m, T, R, "both")
    _, _, g1 = _igrad(m, T, R, "reference")
    assert torch.equal(g0, g1) and torch.isfinite(g0).all() and (g0 != 0).any()
    _, _, gk = _igrad(m, T[3:4], R[3:4], "reference")
    assert torch.equal(gk[0], g0[3])
    for gb in (1, 3):
        m.grad_batch = gb
        _, gtb, gs = _igrad(m, T, R, "both")
        assert torch.equal(gs, g0) and torch.equal(gtb, gt0), gb
    m.grad_batch = None
    w = torch.tensor([1.0, 2.0, 0.5, 0.0, -4.0], device=DEV)
    _, _, gw = _igrad(m, T, R, "reference", weights=w)
    assert torch.equal(gw, g0 * w[:, None, None, None])
    # channels-last device reference and a host BHWC reference
    ycl = R.clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    m.jod_images(T, ycl, wrt="reference").sum().backward()
    assert torch.equal(ycl.grad, g0)
    yh = R.cpu().permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    m.jod_images(T.cpu().permute(0, 2, 3, 1).contiguous(), yh, dim_order="BHWC", wrt="reference").sum().backward()
    assert yh.grad.device.type == "cpu" and torch.equal(yh.grad.permute(0, 3, 1, 2).to(DEV), g0)


def test_wrt_handling():
    m = _metric("standard_4k")
    t, r = _synth_clip(3, 4, 64, 96, seed=33)
    T, R = torch.from_numpy(t).to(DEV), torch.from_numpy(r).to(DEV)
    Tg, Rg = T.clone().requires_grad_(True), R.clone().requires_grad_(True)
    for call in (lambda **kw: m.jod_video(kw.pop("t"), kw.pop("r"), dim_order="CFHW", frames_per_second=30, **kw),
                 lambda **kw: m.jod_images(kw.pop("t")[:, 0][None], kw.pop("r")[:, 0][None], **kw)):
        with pytest.raises(RuntimeError, match="reference are not supported"):
            call(t=Tg, r=Rg)
        with pytest.raises(RuntimeError, match="reference are not supported"):
            call(t=Tg, r=Rg, wrt="test")
        with pytest.raises(RuntimeError, match='"both"'):
            call(t=Tg, r=Rg, wrt="reference")
        with pytest.raises(ValueError):
            call(t=Tg, r=Rg, wrt="ref")
        # no grad_fn where nothing asks for a gradient; a constant reference under "both" is the test side alone
        assert call(t=T, r=R, wrt="reference").grad_fn is None and call(t=T, r=R, wrt="both").grad_fn is None
        assert call(t=Tg, r=R, wrt="both").grad_fn is not None and call(t=T, r=Rg, wrt="both").grad_fn is not None
        jod = call(t=T, r=Rg, wrt="reference")
        (g,) = torch.autograd.grad(jod.sum(), Rg, create_graph=True)
        with pytest.raises(RuntimeError):
            g.sum().backward()
    fm = _metric("standard_4k", opt={"foveated": True})
    with pytest.raises(RuntimeError, match="reference are not supported.*jod_images and jod_video only"):
        fm.jod_gazes(Tg, Rg, [[10.0, 20.0]], dim_order="CFHW", frames_per_second=30)
    with pytest.raises(RuntimeError, match="Gradients through the metric are not supported"):
        m.predict(T, Rg, dim_order="CFHW", frames_per_second=30)


def _call_stats(m):
    out = (ctypes.c_int64 * 3)()
    nat.check(nat.lib().fvvdp_ctx_call_stats(m._ctx.handle, out))
    return [int(v) for v in out]


def test_backward_adds_no_host_sync():
    """As test_gpu_video_grad.py counts it: the backward with respect to the reference, or to both, adds no host
    synchronisation, allocation or free inside the context's entry points to what the forward left."""
    m = _metric("standard_4k")
    t, r = _synth_clip(3, 6, 64, 96, seed=34)
    T, R = torch.from_numpy(t).to(DEV), torch.from_numpy(r).to(DEV)
    y = R.clone().requires_grad_(True)
    jod = m.jod_video(T, y, dim_order="CFHW", frames_per_second=30, wrt="reference")
    after_fwd = _call_stats(m)
    jod.backward()
    assert _call_stats(m) == after_fwd
    _vgrad(m, T, R, 30, "both")
    assert _call_stats(m) == after_fwd


def test_gradient_ascent_on_the_reference_raises_jod():
    m = _metric("standard_fhd")
    t, _ = _synth_clip(3, 4, 64, 96, seed=35)
    rng = np.random.default_rng(4)
    T = torch.from_numpy(t).to(DEV)
    y = torch.from_numpy(np.clip(t + 0.06 * rng.standard_normal(t.shape), 0, 1).astype(np.float32)).to(DEV)
    prev = None
    for step in range(20):
        yg = y.clone().requires_grad_(True)
        jod = m.jod_video(T, yg, dim_order="CFHW", frames_per_second=30, wrt="reference")
        jod.backward()
        q = float(jod.detach())
        if prev is not None:
            assert q > prev, (step, q, prev)
        prev = q
        with torch.no_grad():
            y = (y + 0.004 * yg.grad / yg.grad.abs().max()).clamp(0, 1)
    print("JOD after 20 steps: %.4f" % prev)
