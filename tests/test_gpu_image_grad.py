"""fvvdp.jod_images on the GPU: values against predict_images, gradients against the reference's autograd (goldens g18) and
against finite differences of the float64 CPU oracle, batch invariance, determinism, layouts, interleaving, refusals and a
short optimisation.  Tolerances are 3x the worst error measured on MI355X."""
import os
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grad_cases import CASES, case_inputs, load_golden          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# max|g - g_ref| / max|g_ref| against the reference's autograd, per case
# (measured on MI355X: 3.4e-5, 5.5e-5, 2.9e-4, 9.6e-5, 4.9e-5, 5.1e-4, 0, 3.0e-5)
GOLDEN_TOL = {"a_gray_fhd": 1.1e-4, "b_rgb_4k_oob": 1.7e-4, "c_rgb_hdr_pq": 9e-4, "d_gray_hdr_linear": 3e-4,
              "e_rgb_gamma22": 1.5e-4, "f_rgb_foveated": 1.6e-3, "g_identical": 0.0, "h_g1_crop256": 1e-4}
# |<g, d> - (JOD64(x+) - JOD64(x-))| / |JOD64(x+) - JOD64(x-)|: worst measured 2.9e-3 (1920x1080, where the sum
# <g, d> over 6.2 M samples cancels to 1/40 of its terms' magnitude); the CPU probe of the reference saw 2.4e-4 on small images
FD_TOL = 9e-3


def _metric(display, opt=None):
    opt = opt or {}
    kw = {}
    if "photometry" in opt:
        kw["display_photometry"] = fv.fvvdp_display_photo_eotf(**opt["photometry"])
    return fv.fvvdp(display_name=display, foveated=bool(opt.get("foveated")), quiet=True, device=DEV, **kw)


def _grad(m, test, ref, fix=None, dim_order="BCHW", weights=None):
    x = test.clone().requires_grad_(True)
    jod = m.jod_images(x, ref, dim_order=dim_order, fixation_point=fix)
    (jod.sum() if weights is None else (weights * jod).sum()).backward()
    return jod.detach(), x.grad


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_gradients(name):
    C, H, W, display, opt = CASES[name]
    t, r = case_inputs(name)
    jod_ref, g_ref = load_golden(name)
    m = _metric(display, opt)
    fix = opt.get("fix")
    test, ref = torch.from_numpy(t[None]).to(DEV), torch.from_numpy(r[None]).to(DEV)
    jod, g = _grad(m, test, ref, fix=fix)
    q_pi, _ = m.predict_images(test, ref, fixation_point=fix)
    assert torch.equal(jod, q_pi), (jod, q_pi)
    assert abs(float(jod[0]) - jod_ref) < 2e-3, (float(jod[0]), jod_ref)
    g = g[0].cpu().numpy()
    assert np.isfinite(g).all()
    gmax = float(np.abs(g_ref).max())
    err = float(np.abs(g - g_ref).max())
    print("%s: max|g - g_ref| = %.3e, max|g_ref| = %.3e, rel %.3e" % (name, err, gmax, err / max(gmax, 1e-30)))
    if opt.get("identical"):
        assert (g == 0).all()
    else:
        assert err <= GOLDEN_TOL[name] * gmax
    if opt.get("oob"):
        oob = (t < 0) | (t > 1)
        assert oob.any() and (g[oob] == 0).all() and (g_ref[oob] == 0).all()


def _fd_check(display, t, r, n_dirs, eps=3e-5, seed=0):
    """<g, d> against a central difference of the float64 oracle, d = the realised x+ - x-."""
    from oracle import fvvdp_oracle as orc
    m = _metric(display)
    test, ref = torch.from_numpy(t[None]).to(DEV), torch.from_numpy(r[None]).to(DEV)
    _, g = _grad(m, test, ref)
    g = g[0].double().cpu().numpy()
    assert np.isfinite(g).all()
    o = orc.Oracle(display, dtype=np.float64)
    rng = np.random.default_rng(seed)
    worst = 0.0
    for _ in range(n_dirs):
        d = rng.standard_normal(t.shape)
        d[(t < 4 * eps) | (t > 1 - 4 * eps)] = 0.0          # stay clear of the display model's clamps
        xp = (t + eps * d).astype(np.float32)
        xm = (t - eps * d).astype(np.float32)
        dj = o.predict(xp[:, None], r[:, None], dim_order="CFHW")[0] - o.predict(xm[:, None], r[:, None], dim_order="CFHW")[0]
        lin = float((g * (xp.astype(np.float64) - xm.astype(np.float64))).sum())
        rel = abs(lin - dj) / abs(dj)
        worst = max(worst, rel)
        scale = float(np.abs(g * (xp.astype(np.float64) - xm.astype(np.float64))).sum())
        print("%s %s: <g,d> %.6e  dJOD64 %.6e  rel %.3e  (of sum|g d|: %.3e)" % (display, t.shape, lin, dj, rel,
                                                                                abs(lin - dj) / scale))
    assert worst <= FD_TOL


def _synth(C, H, W, seed):
    from fovvideovdp_amd.synth import synth_frame_pair
    t8, r8 = synth_frame_pair(1, H, W, C=C, seed_ref=seed, seed_test=seed + 7)
    return (t8.numpy().astype(np.float32) / np.float32(255.0), r8.numpy().astype(np.float32) / np.float32(255.0))


@pytest.mark.parametrize("C,H,W,display,n_dirs", [(1, 68, 121, "standard_fhd", 3), (3, 135, 240, "standard_4k", 3),
                                                  (3, 512, 512, "standard_4k", 3), (3, 1080, 1920, "standard_4k", 3),
                                                  (3, 2160, 3840, "standard_4k", 1)])
def test_finite_differences_fp64_oracle(C, H, W, display, n_dirs):
    t, r = _synth(C, H, W, seed=H + W)
    _fd_check(display, t, r, n_dirs)


def test_batch_invariance_and_determinism():
    m = _metric("standard_4k")
    t, r = _synth(3, 64, 96, seed=11)
    rng = np.random.default_rng(1)
    ts = np.stack([np.clip(t + 0.02 * rng.standard_normal(t.shape), 0, 1).astype(np.float32) for _ in range(130)])
    rs = np.stack([r] * 130)
    T, R = torch.from_numpy(ts).to(DEV), torch.from_numpy(rs).to(DEV)
    _, g_all = _grad(m, T, R)
    _, g_all2 = _grad(m, T, R)
    assert torch.equal(g_all, g_all2)
    for k in (0, 5, 129):
        _, g1 = _grad(m, T[k:k + 1], R[k:k + 1])
        assert torch.equal(g1[0], g_all[k]), k
    _, g3 = _grad(m, T[127:130], R[127:130])
    assert torch.equal(g3, g_all[127:130])
    m.grad_batch = 7                                          # several backward batches
    _, g_small = _grad(m, T, R)
    assert torch.equal(g_small, g_all)
    assert torch.isfinite(g_all).all() and (g_all != 0).any()


def test_upstream_weights():
    m = _metric("standard_4k")
    t, r = _synth(3, 64, 96, seed=12)
    T = torch.from_numpy(np.stack([t, t[:, ::-1].copy(), 1 - t, t])).to(DEV)
    R = torch.from_numpy(np.stack([r, r[:, ::-1].copy(), 1 - r, r])).to(DEV)
    w = torch.tensor([1.0, 2.0, 0.5, 0.0], device=DEV)
    _, g1 = _grad(m, T, R)
    _, gw = _grad(m, T, R, weights=w)
    assert torch.equal(gw, g1 * w[:, None, None, None])


def test_layouts():
    m = _metric("standard_4k")
    t, r = _synth(3, 64, 96, seed=13)
    T, R = torch.from_numpy(np.stack([t, 1 - t])), torch.from_numpy(np.stack([r, 1 - r]))
    _, g = _grad(m, T.to(DEV), R.to(DEV))
    # host BHWC tensor: the gradient lands on the host, in BHWC
    xh = T.permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    jod = m.jod_images(xh, R.permute(0, 2, 3, 1).contiguous(), dim_order="BHWC")
    jod.sum().backward()
    assert xh.grad.device.type == "cpu" and xh.grad.shape == xh.shape
    assert torch.equal(xh.grad.permute(0, 3, 1, 2).to(DEV), g)
    # non-contiguous device view of a larger leaf
    base = torch.zeros((2, 3, 64, 104), device=DEV)
    base[..., 4:100] = T.to(DEV)
    base.requires_grad_(True)
    view = base[..., 4:100]
    assert not view.is_contiguous()
    m.jod_images(view, R.to(DEV)).sum().backward()
    assert torch.equal(base.grad[..., 4:100], g)
    assert (base.grad[..., :4] == 0).all() and (base.grad[..., 100:] == 0).all()


def test_interleaved_calls():
    m = _metric("standard_4k")
    t, r = _synth(3, 72, 120, seed=14)
    A, RA = torch.from_numpy(t[None]).to(DEV), torch.from_numpy(r[None]).to(DEV)
    _, g_plain = _grad(m, A, RA)
    x = A.clone().requires_grad_(True)
    jod = m.jod_images(x, RA)
    t2, r2 = _synth(3, 130, 90, seed=15)
    m.predict_images(torch.from_numpy(np.stack([t2] * 3)).to(DEV), torch.from_numpy(np.stack([r2] * 3)).to(DEV))
    jod.sum().backward()
    assert torch.equal(x.grad, g_plain)


def test_refusals():
    m = _metric("standard_4k")
    t, r = _synth(3, 64, 96, seed=16)
    x = torch.from_numpy(t[None]).to(DEV).requires_grad_(True)
    R = torch.from_numpy(r[None]).to(DEV)
    jod = m.jod_images(x, R)
    (g,) = torch.autograd.grad(jod.sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    with pytest.raises(RuntimeError, match="reference are not supported"):
        m.jod_images(x, R.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="Gradients through the metric are not supported"):
        m.predict_images(x, R)


def test_gradient_ascent_raises_jod():
    m = _metric("standard_fhd")
    t, r = _synth(3, 256, 256, seed=17)
    rng = np.random.default_rng(2)
    x = torch.from_numpy(np.clip(r + 0.06 * rng.standard_normal(r.shape), 0, 1).astype(np.float32)[None]).to(DEV)
    R = torch.from_numpy(r[None]).to(DEV)
    prev = None
    for step in range(20):
        xg = x.clone().requires_grad_(True)
        jod = m.jod_images(xg, R)
        jod.sum().backward()
        q = float(jod[0].detach())
        if prev is not None:
            assert q > prev, (step, q, prev)
        prev = q
        with torch.no_grad():
            x = (x + 0.004 * xg.grad / xg.grad.abs().max()).clamp(0, 1)
    print("JOD after 20 steps: %.4f" % prev)
