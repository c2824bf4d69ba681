"""fvvdp.jod_gazes on the GPU.  The yardstick is always existing code or the reference, never jod_gazes itself:

    values     predict_gazes (bit identity)
    gradients  g_loop = sum_g w_g * grad of jod_video(fixation_point=fp[g]), accumulated in float64 on the host,
               and the reference's autograd (tests/golden/g20_gaze_grad.npz)
    the layer kernel alone (G = 1)  fvvdp_video_grad_frames on the maps of the same gaze

Tolerances are 3x the worst error measured on MI355X, under the cap of 1.6e-3 the project grants a foveated gradient."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd import gaze_grad, video_grad
from fovvideovdp_amd.synth import synth_video_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gaze_grad_cases as gc          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NG = nat.GAZE_GROUP_MAX
COUNTS = (1, NG - 1, NG, NG + 1, 2 * NG + 1)
N = 5
FPS = 30
CAP = 1.6e-3

# (H, W, C) of the clips and the displays they are scored on: the sizes of tests/test_gpu_gazes.py (odd sizes, two strips at
# level 0 of 135x240, two chunks at 5x9; standard_hmd: a 110 degree field of view, whose bands have no grouped forward kernel)
CLIPS = {"gray68x121": (68, 121, 1), "rgb135x240": (135, 240, 3), "gray5x9": (5, 9, 1)}
CASES = [("gray68x121", "standard_4k"), ("rgb135x240", "standard_4k"), ("gray68x121", "standard_hdr_pq"),
         ("rgb135x240", "standard_hmd"), ("gray5x9", "standard_4k")]

# max|g - g_loop| / max|g_loop|, the worst over G in COUNTS, per case: 3x the value measured on MI355X (gray68x121 / standard_4k
# 1.42e-6, rgb135x240 / standard_4k 4.76e-7, gray68x121 / standard_hdr_pq 4.72e-6, rgb135x240 / standard_hmd 1.62e-6, gray5x9
# 3.47e-7): float32 rounding of S and of the order of the sum, three orders below the cap
LOOP_TOL = {("gray68x121", "standard_4k"): 4.3e-6, ("rgb135x240", "standard_4k"): 1.5e-6,
            ("gray68x121", "standard_hdr_pq"): 1.5e-5, ("rgb135x240", "standard_hmd"): 4.9e-6, ("gray5x9", "standard_4k"): 1.1e-6}
# max|g - g_ref| / max|g_ref| against the reference's autograd (g20): 3x the value measured on MI355X (4.32e-4; the foveated
# case d of tests/test_gpu_video_grad.py measures 3.9e-4 against the same reference: its fp32 finite-difference magnification)
GOLDEN_TOL = 1.3e-3
# max|g0 - g0_video| / max|g0_video| of the layer kernel alone (S recomputed against S read from the map): 3x the value measured
# on MI355X (gray68x121 / standard_4k 2.57e-7, gray68x121 / standard_hmd 5.07e-7, rgb135x240 / standard_4k 1.41e-7,
# rgb135x240 / standard_hmd 6.85e-7)
LAYER_TOL = {("gray68x121", "standard_4k"): 7.7e-7, ("rgb135x240", "standard_4k"): 4.3e-7, ("gray68x121", "standard_hmd"): 1.6e-6,
             ("rgb135x240", "standard_hmd"): 2.1e-6}


def _clip(name, pair=7):
    """float32 [1, C, N, H, W] in [0, 1] on the device."""
    H, W, C = CLIPS[name]
    t, r = synth_video_pair(N, H, W, pair=pair)
    t, r = t.to(torch.float32) / 255, r.to(torch.float32) / 255
    if C == 1:
        t, r = t.mean(dim=1, keepdim=True), r.mean(dim=1, keepdim=True)
    return t.contiguous().to(DEV), r.contiguous().to(DEV)


def _gazes(H, W, kind, n=N):
    """2 NG + 1 gazes: the frame corners, 500 pixels outside the frame on either side (the eccentricity clamp), the centre, then
    seeded points.  fixed: [G, 2]; moving: [G, n, 2], gaze g drifting from point g to point g + 5."""
    rng = np.random.RandomState(11)
    pts = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W + 499, H + 499), (-500, -500), (W // 2, H // 2)]
    while len(pts) < 2 * NG + 1:
        pts.append((float(rng.uniform(0, W - 1)), float(rng.uniform(0, H - 1))))
    fixed = np.asarray(pts, np.float32)
    if kind == "fixed":
        return fixed
    w = np.linspace(0.0, 1.0, n, dtype=np.float32)[None, :, None]
    return np.ascontiguousarray(fixed[:, None, :] * (1 - w) + np.roll(fixed, -5, axis=0)[:, None, :] * w)


def _weights(G):
    """Seeded, of mixed sign, one exact zero (from two gazes on)."""
    w = np.random.RandomState(100 + G).uniform(0.5, 2.0, G).astype(np.float32)
    w[1::2] *= -1
    if G >= 2:
        w[min(3, G - 1)] = 0.0
    return w


def _metric(display, **kw):
    return fv.fvvdp(display_name=display, foveated=True, quiet=True, device=DEV, **kw)


def _gaze_grad(m, t, r, fp, w, dim_order="BCFHW", fps=FPS):
    x = t.clone().requires_grad_(True)
    jod = m.jod_gazes(x, r, fp, dim_order=dim_order, frames_per_second=fps)
    (jod * torch.as_tensor(w, device=jod.device)).sum().backward()
    return jod.detach(), x.grad


_cache = {}


def _case(clip, display):
    """(metric, test, ref, moving gazes [2 NG + 1, N, 2], per-gaze gradients of jod_video [2 NG + 1, ...] in float64 on the
    host) -- the loop, made once, never changed."""
    key = (clip, display)
    if key not in _cache:
        t, r = _clip(clip)
        H, W, _ = CLIPS[clip]
        fp = _gazes(H, W, "moving")
        m = _metric(display)
        per = []
        for g in range(len(fp)):
            x = t.clone().requires_grad_(True)
            m.jod_video(x, r, frames_per_second=FPS, fixation_point=fp[g]).backward()
            per.append(x.grad.double().cpu().numpy())
        _cache[key] = (m, t, r, fp, np.stack(per))
    return _cache[key]


def _rel(g, ref):
    return float(np.abs(g - ref).max()) / float(np.abs(ref).max())


# ---- 1. forward bits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fixed", "moving"])
@pytest.mark.parametrize("clip,display", CASES)
def test_forward_is_bit_identical_to_predict_gazes(clip, display, kind):
    t, r = _clip(clip)
    H, W, _ = CLIPS[clip]
    fp = _gazes(H, W, kind)
    m = _metric(display)
    for G in COUNTS:
        want, _ = m.predict_gazes(t, r, fp[:G], frames_per_second=FPS)
        x = t.clone().requires_grad_(True)
        jod = m.jod_gazes(x, r, fp[:G], frames_per_second=FPS)
        assert jod.requires_grad and jod.dtype is torch.float32 and jod.device == DEV and tuple(jod.shape) == (G,)
        assert torch.equal(jod.detach(), want), (G, jod, want)
        assert torch.equal(m.jod_gazes(t, r, torch.from_numpy(fp[:G]), frames_per_second=FPS), want)
    one = m.predict(t, r, frames_per_second=FPS, fixation_point=fp[2])[0]
    assert torch.equal(jod.detach()[2], one)


# ---- 2. gradient against the loop of jod_video calls -----------------------------------------------------------------------
@pytest.mark.parametrize("clip,display", CASES)
def test_gradient_against_the_loop_of_jod_video(clip, display):
    m, t, r, fp, per = _case(clip, display)
    # the gazes matter: the loop's gradients of the first two gazes differ by more than 5 % of the larger of the two (the
    # per-gaze gradients g_loop(fp[g]); a weighted sum's size would depend on G and on the weights)
    sep = float(np.abs(per[0] - per[1]).max()) / float(max(np.abs(per[0]).max(), np.abs(per[1]).max()))
    print("%s %s: max|g_loop(fp[0]) - g_loop(fp[1])| / max|g_loop| = %.3f" % (clip, display, sep))
    assert sep > 0.05
    worst = 0.0
    for G in COUNTS:
        w = _weights(G)
        g_loop = np.tensordot(w.astype(np.float64), per[:G], axes=1)
        _, g = _gaze_grad(m, t, r, fp[:G], w)
        assert g.shape == t.shape and g.device == DEV and torch.isfinite(g).all()
        rel = _rel(g.double().cpu().numpy(), g_loop)
        worst = max(worst, rel)
        print("%s %s G=%d: max|g - g_loop| / max|g_loop| = %.3e  (max|g_loop| %.3e)" % (clip, display, G, rel, np.abs(g_loop).max()))
    print("%s %s: worst %.3e" % (clip, display, worst))
    tol = LOOP_TOL[(clip, display)]
    assert tol <= CAP
    assert worst <= tol


# ---- 3. golden from the reference's autograd --------------------------------------------------------------------------------
def test_golden_gradient_of_a_weighted_sum():
    t, r = gc.case_inputs()
    jod_ref, g_ref = gc.load_golden()
    m = _metric(gc.DISPLAY, temp_padding=gc.PADDING)
    T, R = torch.from_numpy(t).to(DEV), torch.from_numpy(r).to(DEV)
    jod, g = _gaze_grad(m, T, R, gc.case_gazes(), gc.WEIGHTS, dim_order="CFHW", fps=gc.FPS)
    print("JOD %s, reference %s" % (jod.cpu().numpy(), jod_ref))
    assert np.abs(jod.cpu().numpy() - jod_ref).max() < 2e-3
    rel = _rel(g.cpu().numpy(), g_ref)
    print("g20: max|g - g_ref| / max|g_ref| = %.3e  (max|g_ref| %.3e)" % (rel, np.abs(g_ref).max()))
    assert GOLDEN_TOL <= CAP
    assert rel <= GOLDEN_TOL


# ---- 4. the layer kernel alone, through the C ABI ---------------------------------------------------------------------------
@pytest.mark.parametrize("clip,display", sorted(LAYER_TOL))
def test_layer_kernel_against_the_single_gaze_backward(clip, display):
    """G = 1: fvvdp_gaze_grad_frames against fvvdp_video_grad_frames fed by the same map-writing foveated forward of that gaze.
    The only difference is S recomputed from the full tables against S read from the map."""
    t, r = _clip(clip)
    H, W, _ = CLIPS[clip]
    fix = _gazes(H, W, "moving")[7]
    m = _metric(display)
    lib = nat.lib()
    with torch.cuda.device(DEV):
        _, Q = video_grad._forward(m, t, r, float(FPS), fix)
        s = video_grad._Setup(m, t, float(FPS))
        assert s.batch >= N
        maps_arr, _maps = m._band_maps(N, W, H, s.n_bands, contrast_planes=4)
        q_scratch = torch.empty((s.n_bands, 2, N), dtype=torch.float32, device=DEV)
        oob = torch.zeros(1, dtype=torch.int32, device=DEV)
        s.ingest(lib, t, r, 0, N, oob)
        fx, g, _keep = m._fov_args(s.ctx, fix, 0, N, s.n_bands, W, H)
        nat.check(lib.fvvdp_bands_forward(s.ctx.handle, N, ctypes.c_void_p(q_scratch.data_ptr()), N, 0, fx, g, maps_arr, s.stream))
        prm, geom = m.native_params(), m._geom_struct()
        gamma = torch.full((1,), 1.25, device=DEV)
        nb1, nb2 = ctypes.c_size_t(), ctypes.c_size_t()
        nat.check(lib.fvvdp_video_grad_workspace(W, H, s.n_bands, N, ctypes.byref(nb1)))
        nat.check(lib.fvvdp_gaze_grad_workspace(W, H, s.n_bands, N, 1, ctypes.byref(nb2)))
        w1 = torch.empty(nb1.value // 4, dtype=torch.float32, device=DEV)
        w2 = torch.empty(nb2.value // 4, dtype=torch.float32, device=DEV)
        a = torch.full((N, 2, H, W), float("nan"), device=DEV)
        b = torch.full((N, 2, H, W), float("nan"), device=DEV)
        nat.check(lib.fvvdp_video_grad_frames(W, H, s.n_bands, N, ctypes.byref(prm), ctypes.byref(s.pp), ctypes.c_void_p(Q.data_ptr()),
                                              N, 0, ctypes.c_void_p(gamma.data_ptr()), maps_arr, ctypes.c_void_p(a.data_ptr()),
                                              ctypes.c_void_p(w1.data_ptr()), nb1.value, s.stream))
        lut0, lut1, d_axes, h_axes = gaze_grad._csf_tables(m)
        rho = np.ascontiguousarray(s.rho_band, dtype=np.float64)
        gaze = torch.from_numpy(np.ascontiguousarray(fix[None])).to(DEV)
        nat.check(lib.fvvdp_gaze_grad_frames(W, H, s.n_bands, N, 1, 0, ctypes.byref(prm), ctypes.byref(s.pp), ctypes.byref(geom),
                                             rho.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_void_p(lut0.data_ptr()),
                                             ctypes.c_void_p(lut1.data_ptr()), ctypes.c_void_p(d_axes.data_ptr()), nat.fptr(h_axes),
                                             ctypes.c_void_p(gaze.data_ptr()), 2 * N, ctypes.c_void_p(Q.data_ptr()), N, 0,
                                             ctypes.c_void_p(gamma.data_ptr()), maps_arr, ctypes.c_void_p(b.data_ptr()),
                                             ctypes.c_void_p(w2.data_ptr()), nb2.value, s.stream))
        torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.isfinite(b).all() and (a != 0).any()
    rel = _rel(b.double().cpu().numpy(), a.double().cpu().numpy())
    print("%s %s: max|g0 - g0_video| / max|g0_video| = %.3e" % (clip, display, rel))
    tol = LAYER_TOL[(clip, display)]
    assert tol <= CAP
    assert rel <= tol


# ---- 5. determinism and independence -----------------------------------------------------------------------------------------
def test_determinism_batches_and_zero_weight_gazes():
    m, t, r, fp, per = _case("rgb135x240", "standard_4k")
    G = NG + 1
    w = _weights(G)
    j0, g0 = _gaze_grad(m, t, r, fp[:G], w)
    j1, g1 = _gaze_grad(m, t, r, fp[:G], w)
    assert torch.equal(j0, j1) and torch.equal(g0, g1) and (g0 != 0).any()
    m2 = _metric("standard_4k")
    m2.grad_batch = 2                                      # three backward batches: the bits of one
    j2, g2 = _gaze_grad(m2, t, r, fp[:G], w)
    assert torch.equal(j2, j0) and torch.equal(g2, g0)
    # a gaze with weight 0 appended: the same bits, across a group boundary (8 -> 8 + 1) and inside one (9 -> 9 + 1)
    for n in (NG, G):
        _, ga = _gaze_grad(m, t, r, fp[:n], w[:n])
        _, gb = _gaze_grad(m, t, r, fp[:n + 1], np.append(w[:n], np.float32(0.0)))
        assert torch.equal(ga, gb), n
    # a permuted gaze order: another order of the same sum, within the tolerance of the loop test
    perm = np.random.RandomState(5).permutation(G)
    jp, gp = _gaze_grad(m, t, r, fp[:G][perm], w[perm])
    assert torch.equal(jp, j0[torch.as_tensor(perm, device=DEV)])
    g_loop = np.tensordot(w.astype(np.float64), per[:G], axes=1)
    assert _rel(gp.double().cpu().numpy(), g_loop) <= LOOP_TOL[("rgb135x240", "standard_4k")]
    assert float((gp - g0).abs().max()) <= LOOP_TOL[("rgb135x240", "standard_4k")] * float(np.abs(g_loop).max())


@pytest.mark.parametrize("cap", [1, 2, 4])
def test_the_group_size_does_not_matter(cap, monkeypatch):
    """gaze_grad.GROUP_MAX is the group_max argument of fvvdp_gaze_grad_frames: it caps the gazes per launch of gaze_layer_kernel
    (more launches, the later ones adding to what the earlier ones stored) -- same bits.  That the value reaches the entry
    point shows in the refusal of one it does not take."""
    m, t, r, fp, _ = _case("rgb135x240", "standard_4k")
    G = NG + 1
    w = _weights(G)
    j0, g0 = _gaze_grad(m, t, r, fp[:G], w)
    monkeypatch.setattr(gaze_grad, "GROUP_MAX", cap)
    j1, g1 = _gaze_grad(m, t, r, fp[:G], w)
    assert torch.equal(j1, j0) and torch.equal(g1, g0)
    monkeypatch.setattr(gaze_grad, "GROUP_MAX", 3)
    with pytest.raises(RuntimeError, match="group_max"):
        _gaze_grad(m, t, r, fp[:G], w)


# ---- 6. edge behaviour -------------------------------------------------------------------------------------------------------
def test_identical_clip():
    m, t, r, fp, _ = _case("gray68x121", "standard_4k")
    jod, g = _gaze_grad(m, r, r, fp[:NG + 1], _weights(NG + 1))
    assert torch.all(jod == 10.0) and torch.all(g == 0) and not torch.isnan(g).any()


def test_circular_padding_leaves_frame_0_without_gradient():
    H, W, n = 68, 121, 10                                  # 30 frames per second: 8 taps, N > fl + 1
    t, r = synth_video_pair(n, H, W, C=1, pair=5)
    t, r = (t.to(torch.float32) / 255).to(DEV), (r.to(torch.float32) / 255).to(DEV)
    fp = _gazes(H, W, "moving", n)[:3]
    m = _metric("standard_4k", temp_padding="circular")
    _, g = _gaze_grad(m, t, r, fp, np.float32([1.0, -0.5, 2.0]))
    assert (g[:, :, 0] == 0).all() and all((g[:, :, f] != 0).any() for f in range(1, n))


def test_layouts_and_second_backward():
    m, t, r, fp, _ = _case("rgb135x240", "standard_4k")
    G = 3
    w = _weights(G)
    _, g = _gaze_grad(m, t, r, fp[:G], w)
    # host FHWC tensor: the gradient lands on the host, in FHWC
    xh = t[0].permute(1, 2, 3, 0).contiguous().cpu().requires_grad_(True)
    jod = m.jod_gazes(xh, r[0].permute(1, 2, 3, 0).contiguous().cpu(), fp[:G], dim_order="FHWC", frames_per_second=FPS)
    (jod * torch.as_tensor(w, device=DEV)).sum().backward()
    assert xh.grad.device.type == "cpu" and xh.grad.shape == xh.shape
    assert torch.equal(xh.grad.permute(3, 0, 1, 2).to(DEV), g[0])
    x = t.clone().requires_grad_(True)
    jod = m.jod_gazes(x, r, fp[:G], frames_per_second=FPS)
    (g1,) = torch.autograd.grad(jod.sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):                      # once_differentiable: no double backward
        g1.sum().backward()
    x = t.clone().requires_grad_(True)
    jod = m.jod_gazes(x, r, fp[:G], frames_per_second=FPS)
    jod.sum().backward()
    with pytest.raises(RuntimeError):                      # the graph is freed: a second backward raises
        jod.sum().backward()


def test_no_residue():
    m, t, r, fp, _ = _case("gray68x121", "standard_hdr_pq")
    a = fp[4]

    def others():
        p = m.predict(t, r, frames_per_second=FPS, fixation_point=a)
        q, st = m.predict_gazes(t, r, fp[:NG + 1], frames_per_second=FPS)
        x = t.clone().requires_grad_(True)
        j = m.jod_video(x, r, frames_per_second=FPS, fixation_point=a)
        j.backward()
        return p[0].clone(), p[1]["Q_per_ch"].copy(), q.clone(), st["Q_per_ch"].copy(), j.detach().clone(), x.grad.clone()

    before = others()
    x = t.clone().requires_grad_(True)
    jod = m.jod_gazes(x, r, fp[:NG + 1], frames_per_second=FPS)
    mid = others()                                         # between the forward and the backward
    jod.sum().backward()
    after = others()
    j2, g2 = _gaze_grad(m, t, r, fp[:NG + 1], np.ones(NG + 1, np.float32))
    assert torch.equal(j2, jod.detach()) and torch.equal(g2, x.grad)
    for other in (mid, after):
        for u, v in zip(before, other):
            assert (np.array_equal(u, v) if isinstance(u, np.ndarray) else torch.equal(u, v))


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals():
    t, r = _clip("gray68x121")
    H, W, _ = CLIPS["gray68x121"]
    fp = _gazes(H, W, "fixed")[:3]
    m = _metric("standard_4k")
    with pytest.raises(RuntimeError, match="needs a foveated metric"):
        fv.fvvdp(display_name="standard_4k", quiet=True, device=DEV).jod_gazes(t, r, fp, frames_per_second=FPS)
    with pytest.raises(RuntimeError, match="makes no heat maps"):
        _metric("standard_4k", heatmap="threshold").jod_gazes(t, r, fp, frames_per_second=FPS)

    class Geometry(fv.fvvdp_display_geometry):
        pass

    user = _metric("standard_4k", display_geometry=Geometry((3840, 2160), diagonal_size_inches=30, distance_m=0.6))
    with pytest.raises(RuntimeError, match="display_geometry"):
        user.jod_gazes(t, r, fp, frames_per_second=FPS)
    with pytest.raises(RuntimeError, match="at least 2 frames"):
        m.jod_gazes(t[:, :, :1], r[:, :, :1], fp, frames_per_second=FPS)
    with pytest.raises(RuntimeError, match="B must be 1"):
        m.jod_gazes(torch.cat([t, t]), torch.cat([r, r]), fp, frames_per_second=FPS)
    with pytest.raises(RuntimeError, match="float32"):
        m.jod_gazes((t * 255).to(torch.uint8), (r * 255).to(torch.uint8), fp, frames_per_second=FPS)
    with pytest.raises(RuntimeError, match="reference are not supported"):
        m.jod_gazes(t, r.clone().requires_grad_(True), fp, frames_per_second=FPS)
    with pytest.raises(RuntimeError, match="frame rate too high"):
        m.jod_gazes(t, r, fp, frames_per_second=300)       # 75 taps
    for bad in (np.zeros((3, 3), np.float32), np.zeros((3, N + 1, 2), np.float32), np.zeros((0, 2), np.float32)):
        with pytest.raises(RuntimeError, match="fixation_points must be"):
            m.jod_gazes(t, r, bad, frames_per_second=FPS)
    with pytest.raises(RuntimeError, match="Gradients through the metric are not supported"):
        m.predict_gazes(t.clone().requires_grad_(True), r, fp, frames_per_second=FPS)
