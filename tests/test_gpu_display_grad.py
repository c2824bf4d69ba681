"""Gradients with respect to the display's photometry on the GPU (display_jod_images / display_jod_video): the two sums entry
points alone against float64 numpy, psi.grad end to end against central differences of the float64 oracle, the forward bit for
bit against predict_images / predict on a second metric, psi's dtype and device, the backward batching, degenerate inputs and a
step along the gradient."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

import display_grad_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# The kernels' bound per output: C u sum |terms|, the terms being tap x g0 x w_c x sensitivity (video) or g0 x w_c x sensitivity
# (stills), each fp32 rounding counted once (first order; the last unit covers the second-order terms and the fp64 adds, whose
# count x 2^-53 is below 2^-24 x 1e-4 for any frame that fits the device).
#   K_SENS = 8   the sensitivity value against float64 arithmetic on the same fp32 constants.  sRGB: the add and the multiply in
#                ((V + 0.055) / 1.055), one rounding each, raised to 2.4 (2 x 2.4 = 4.8), powf within 2 ulp: 6.8.  gamma a1: powf,
#                2; a2 = scale V^gamma ln V: powf 2, logf 2, two multiplies 2: 6.  The toe is one multiply.  PQ / linear: the value
#                is 0 or 1, exact (the tests keep every sample's luminance 1e-4 away from the clip, relative).
#   1            the product w_c x sensitivity.
#   12           the fp32 chain: a sum takes the PX x C <= 12 fused multiply-adds of one frame (one rounding each) before it moves
#                to fp64 (DS_CHAIN = 16 is the kernel's stated ceiling; stills: C <= 3).
#   video only:  2 fl  the ring: a window position collects 2 fl fused multiply-adds (taps x g0, both channels), one rounding each;
#                fl + 1  the folds: a frame adds at most fl head positions and one streaming term.
K_SENS = 8


def c_video(fl):
    return 2 * fl + (fl + 1) + K_SENS + 1 + 12 + 1


C_STILL = K_SENS + 1 + 3 + 1
MARGIN = 1e-4

DEV = torch.device("cuda:0")
PSI = {"sRGB": [200.0, 1000.0, 250.0, 0.005, 2.2], "gamma": [200.0, 50.0, 500.0, 0.005, 2.2],
       "PQ": [1500.0, 1e6, 10.0, 0.005, 2.2], "linear": [1500.0, 1e6, 10.0, 0.005, 2.2]}
RGB2Y = np.array([0.2126, 0.7152, 0.0722], dtype=np.float32)


@pytest.fixture(scope="module")
def fv():
    import fovvideovdp_amd
    from fovvideovdp_amd import _native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _native.lib()
    return fovvideovdp_amd


def native_eotf(eotf, psi=None):
    from fovvideovdp_amd import _native as nat
    b = ref.eotf_block(eotf, PSI[eotf] if psi is None else psi)
    e = nat.Eotf()
    e.kind, e.Y_peak, e.Y_black, e.gamma = b["kind"], float(b["Y_peak"]), float(b["Y_black"]), float(b["gamma"])
    return e, b


def samples(rng, shape, eotf):
    """Samples below 0, above 1, at 0, on both sides of the sRGB toe's end, and (PQ, linear) above Y_peak."""
    if eotf == "linear":
        V = rng.uniform(-5.0, 2200.0, shape)
        special = [0.0, 0.004, 0.006, 1499.0, 1501.0, -1.0]
    else:
        V = rng.uniform(-0.1, 1.1, shape)
        special = [0.0, -0.05, 1.0, 1.05, 0.04, 0.041, 0.04045, 0.9, 0.99]
    flat = V.reshape(-1)
    flat[rng.choice(flat.size, 40 * len(special), replace=False)] = np.repeat(special, 40)
    return away_from_clip(V.astype(np.float32), eotf)


def away_from_clip(V, eotf):
    """PQ, linear: a sample whose luminance lies within 2 MARGIN of Y_peak (relative) is replaced by one far below: at the
    threshold the indicator would depend on the last bits of an fp32 power."""
    if eotf in ("PQ", "linear"):
        L = ref.pq_luminance(np.clip(V.astype(np.float64), 0.0, 1.0)) if eotf == "PQ" else V.astype(np.float64)
        V = np.where(np.abs(L / PSI[eotf][0] - 1.0) < 2 * MARGIN, np.float32(0.5 if eotf == "PQ" else 100.0), V)
    return V.astype(np.float32)


def shifted(a, off):
    """A device copy of `a` whose first element sits `off` floats past a 256-byte boundary."""
    buf = torch.empty(a.size + 64, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 256 == 0
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v, buf


# ---- 1. the video sums kernel alone -----------------------------------------------------------------------------------------
def run_video(g0, V, taps, widx, fl, N, C_ch, e, off):
    from fovvideovdp_amd import _native as nat
    from fovvideovdp_amd.video_grad import _fold_arrays, fold_list
    lib = nat.lib()
    H, W = g0.shape[2:]
    HW = H * W
    dg, keep_g = shifted(g0, off)
    dv, keep_v = shifted(V, off)
    head, keep_h = shifted(np.zeros((fl, H, W), dtype=np.float32), off)
    ff, fp = _fold_arrays(fold_list(widx, fl, N))
    nbytes = C.c_size_t(0)
    nat.check(lib.fvvdp_video_display_sums_workspace(W, H, C.byref(nbytes)))
    work = torch.empty(nbytes.value // 8 + 32, dtype=torch.float64, device=DEV)
    out = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
    w = np.ascontiguousarray(RGB2Y)
    nat.check(lib.fvvdp_video_display_sums(W, H, N, C.c_void_p(dg.data_ptr()), ff.ctypes.data_as(C.POINTER(C.c_int32)),
                                           fp.ctypes.data_as(C.POINTER(C.c_int32)), nat.fptr(taps), fl, C.c_void_p(dv.data_ptr()),
                                           C_ch, N * HW, HW, C.byref(e), nat.fptr(w), C.c_void_p(head.data_ptr()), fl * HW * 4,
                                           C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()), nbytes.value, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def video_case(H, W, fl, N, pad, combos, seed, offsets=(0,)):
    """One g0 and window list, every (C, EOTF) of `combos` on it.  Returns the worst error in units of u sum |terms|."""
    from fovvideovdp_amd.fvvdp import window_frame_indices
    rng = np.random.default_rng(seed)
    g0 = (rng.standard_normal((N, 2, H, W)) * 1e-3).astype(np.float32)
    taps = (rng.standard_normal((2, fl)) * 0.3).astype(np.float32)
    widx = np.asarray(window_frame_indices(N, fl, pad))
    assert np.array_equal(widx, ref.window_indices(N, fl, pad))
    if pad == "circular" and N > fl + 1:
        assert 0 not in widx                                   # frame 0 is unseen: exact zeros from it
    s, sa = ref.video_s(g0.reshape(N, 2, H * W), taps, widx, fl, N)
    worst = 0.0
    for C_ch, eotf in combos:
        e, blk = native_eotf(eotf)
        V = samples(rng, (C_ch, N, H, W), eotf)
        assert ref.clip_margin(V, blk) > MARGIN
        wgt = RGB2Y if C_ch == 3 else np.ones(1, dtype=np.float32)
        want, mag = ref.sums_of(s, sa, V.reshape(C_ch, N, H * W), wgt, blk)
        if eotf == "gamma":
            assert want[2] != 0 and np.isfinite(want[2])
        else:
            assert want[2] == 0
        for off in offsets:
            got = run_video(g0, V, taps, widx, fl, N, C_ch, e, off)
            again = run_video(g0, V, taps, widx, fl, N, C_ch, e, off)
            assert got.tobytes() == again.tobytes()             # no atomics: bit-identical from run to run
            err = np.abs(got - want) / (U * np.where(mag > 0, mag, 1.0))
            assert np.all(got[mag == 0] == 0)
            worst = max(worst, err.max())
            assert np.isfinite(got).all() and err.max() <= c_video(fl), (H, W, fl, N, pad, C_ch, eotf, off, err, c_video(fl))
    return worst


ALL = list(itertools.product((1, 3), ("sRGB", "gamma", "PQ", "linear")))


@pytest.mark.parametrize("fl", [8, 15, 30, 60])
def test_video_sums_kernel(fv, fl):
    """40 x 52 = 2080 pixels: four pixels per lane (fl <= 16: three workgroups, the last one partly empty) or two; 37 x 41 = 1517,
    odd: one pixel per lane; pointers 1 and 2 floats off a 256-byte boundary (one pixel per lane; two for the long rings)."""
    worst = 0.0
    for i, (N, pad) in enumerate(itertools.product((3, 12), ("replicate", "circular", "pingpong"))):
        worst = max(worst, video_case(40, 52, fl, N, pad, ALL, 1000 + 10 * fl + i))
    worst = max(worst, video_case(37, 41, fl, 12, "circular", ALL[1::2] + ALL[0::2][:2], 2000 + fl))
    worst = max(worst, video_case(37, 41, fl, 3, "pingpong", ALL[2:4], 2100 + fl))
    worst = max(worst, video_case(40, 52, fl, 12, "replicate", [(3, "gamma"), (1, "PQ")], 2200 + fl, offsets=(1, 2)))
    print("fl %d: worst error %.2f u sum|terms| (bound %d)" % (fl, worst, c_video(fl)))


# ---- 2. the still sums entry alone -------------------------------------------------------------------------------------------
def still_case(fv, C_ch, eotf, seed):
    """Three pairs of 67 x 121 through a real map-writing pass under the display block of `eotf`; g0 of either side read back
    through the gradient entry points with a display model whose derivative is 1 (linear, C = 1, samples inside the clip)."""
    from fovvideovdp_amd import _native as nat
    from fovvideovdp_amd.image_grad import _Setup, slope_planes
    lib = nat.lib()
    n, H, W = 3, 67, 121
    HW = H * W
    rng = np.random.default_rng(seed)
    rv = samples(rng, (n, C_ch, H, W), eotf)
    tv = away_from_clip((rv + (0.03 if eotf != "linear" else 20.0) * rng.standard_normal(rv.shape)).astype(np.float32), eotf)
    e, blk = native_eotf(eotf)
    assert min(ref.clip_margin(tv, blk), ref.clip_margin(rv, blk)) > MARGIN
    m = fv.fvvdp(display_name="standard_4k", device=DEV, quiet=True)
    t, r = torch.from_numpy(tv).to(DEV), torch.from_numpy(rv).to(DEV)
    s = _Setup(m, t)
    s.e = e
    maps_arr, _maps = m._band_maps(n, W, H, s.n_bands, contrast_planes=2)
    slopes, _slopes = slope_planes(m, n, W, H, s.n_bands)
    Q = torch.zeros((s.n_bands, 2, n), dtype=torch.float32, device=DEV)
    jod = torch.empty(n, dtype=torch.float32, device=DEV)
    tp = s.ingest(lib, t, r, 0, n)
    rp = (C.c_void_p * n)(*[r[k].data_ptr() for k in range(n)])
    nat.check(lib.fvvdp_ctx_set_slope_maps(s.ctx.handle, slopes))
    try:
        nat.check(lib.fvvdp_images_forward_pool(s.ctx.handle, n, C.c_void_p(Q.data_ptr()), n, 0, None, None, maps_arr,
                                                C.byref(s.pp), C.c_void_p(jod.data_ptr()), s.stream))
    finally:
        nat.check(lib.fvvdp_ctx_set_slope_maps(s.ctx.handle, None))
    prm = m.native_params()
    ones = torch.ones(n, dtype=torch.float32, device=DEV)
    # g0 of both sides: dL/dV = 1 and w = 1 make the gradient entry points return it as they form it
    lin = nat.Eotf()
    lin.kind, lin.Y_peak, lin.Y_black = nat.EOTF_LINEAR, 1e30, 0.0
    unit = torch.ones((n, 1, H, W), dtype=torch.float32, device=DEV)
    up = (C.c_void_p * n)(*[unit[k].data_ptr() for k in range(n)])
    g0 = torch.empty((2, n, 1, H, W), dtype=torch.float32, device=DEV)
    gb, rb = C.c_size_t(0), C.c_size_t(0)
    nat.check(lib.fvvdp_images_grad_workspace(W, H, s.n_bands, n, C.byref(gb)))
    nat.check(lib.fvvdp_ref_grad_workspace(W, H, s.n_bands, n, 1, C.byref(rb)))
    gwork = torch.empty(max(gb.value, rb.value) // 4 + 64, dtype=torch.float32, device=DEV)
    gp = (C.c_void_p * n)(*[g0[0, k].data_ptr() for k in range(n)])
    nat.check(lib.fvvdp_images_grad(W, H, s.n_bands, n, C.byref(prm), C.byref(s.pp), C.c_void_p(Q.data_ptr()), n, 0,
                                    C.c_void_p(ones.data_ptr()), maps_arr, up, 1, HW, C.byref(lin), None, gp,
                                    C.c_void_p(gwork.data_ptr()), gb.value, s.stream))
    gp = (C.c_void_p * n)(*[g0[1, k].data_ptr() for k in range(n)])
    nat.check(lib.fvvdp_images_ref_grad(W, H, s.n_bands, n, C.byref(prm), C.byref(s.pp), C.c_void_p(Q.data_ptr()), n, 0,
                                        C.c_void_p(ones.data_ptr()), maps_arr, slopes, up, 1, HW, C.byref(lin), None, gp,
                                        C.c_void_p(gwork.data_ptr()), rb.value, s.stream))
    w = np.ascontiguousarray(RGB2Y)
    wgt = RGB2Y if C_ch == 3 else np.ones(1, dtype=np.float32)
    worst = 0.0
    for side, (sl, ptrs, V) in enumerate(((None, tp, tv), (slopes, rp, rv))):
        nbytes = C.c_size_t(0)
        nat.check(lib.fvvdp_images_display_sums_workspace(W, H, s.n_bands, n, side, C.byref(nbytes)))
        work = torch.empty(nbytes.value // 8 + 32, dtype=torch.float64, device=DEV)
        outs = []
        for _ in range(2):
            out = torch.full((n, 3), float("nan"), dtype=torch.float64, device=DEV)
            nat.check(lib.fvvdp_images_display_sums(W, H, s.n_bands, n, C.byref(prm), C.byref(s.pp), C.c_void_p(Q.data_ptr()), n, 0,
                                                    C.c_void_p(ones.data_ptr()), maps_arr, sl, ptrs, C_ch, HW, C.byref(e),
                                                    nat.fptr(w), C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()),
                                                    nbytes.value, s.stream))
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy())
        assert outs[0].tobytes() == outs[1].tobytes()
        g = g0[side].cpu().numpy().reshape(n, HW).astype(np.float64)
        assert np.abs(g).max() > 0
        for k in range(n):
            want, mag = ref.sums_of(g[k], np.abs(g[k]), V[k].reshape(C_ch, HW), wgt, blk)
            err = np.abs(outs[0][k] - want) / (U * np.where(mag > 0, mag, 1.0))
            assert np.all(outs[0][k][mag == 0] == 0)
            worst = max(worst, err.max())
            assert np.isfinite(outs[0][k]).all() and err.max() <= C_STILL, (C_ch, eotf, side, k, err)
    return worst


@pytest.mark.parametrize("eotf", ["sRGB", "gamma", "PQ", "linear"])
def test_still_sums_entry(fv, eotf):
    worst = max(still_case(fv, C_ch, eotf, 3000 + 7 * C_ch + len(eotf)) for C_ch in (1, 3))
    print("%s: worst error %.2f u sum|terms| (bound %d)" % (eotf, worst, C_STILL))


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------
def metric_for(fv, name, psi=None, **kw):
    """The metric of a case.  psi given: built AT psi (the second metric of a comparison).  Otherwise the metric the case calls
    display_jod_* on: a case that fixes a display is built with nothing of it but the EOTF kind -- a 100 cd/m^2 panel with the
    constructor's defaults -- so that the fixed values reach the kernels through psi alone; the others run at the metric's own
    display parameters (psi0 is the display's)."""
    from fovvideovdp_amd.display_model import fvvdp_display_photo_eotf
    display, eotf, fixed, fov, C_ch, N, fps, pad = ref.CASES[name]
    if psi is None and fixed:
        ph = fvvdp_display_photo_eotf(100.0, EOTF=eotf)
        assert not np.array_equal([ph.Y_peak, ph.contrast, ph.E_ambient, ph.k_refl, ph.gamma], ref.psi0(name))
    else:
        v = dict(zip(ref.NAMES, (float(x) for x in (ref.psi0(name) if psi is None else psi))))
        ph = fvvdp_display_photo_eotf(v["Y_peak"], contrast=v["contrast"], EOTF=eotf, gamma=v["gamma"], E_ambient=v["E_ambient"],
                                      k_refl=v["k_refl"])
    return fv.fvvdp(display_name=display, display_photometry=ph, foveated=fov, temp_padding=pad, device=DEV, quiet=True, **kw)


def call(m, name, psi, test=None, rf=None):
    t, r, gaze = ref.inputs(name)
    t, r = (t if test is None else test), (r if rf is None else rf)
    if ref.CASES[name][5] == 0:
        return m.display_jod_images(t[:, :, 0], r[:, :, 0], psi, dim_order="BCHW", fixation_point=gaze)
    return m.display_jod_video(t, r, psi, dim_order="BCFHW", frames_per_second=ref.CASES[name][6], fixation_point=gaze)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_psi_grad_against_central_differences(fv, name):
    """|psi.grad - central differences of the float64 oracle| / scale_i <= 3 x DISAGREE.  The GPU path and the reference are both
    fp32 evaluations of one formula against float64; DISAGREE is the reference's distance from the same central differences and
    the factor 3 is this project's convention.  Observed on an MI355X: see DESIGN.md section 4; never used to set the bound."""
    worst, _ = ref.disagree()
    for k in range(len(ref.weights(name))):
        assert ref.clamp_counts(name, k) == (0, 0)
    m = metric_for(fv, name)
    psi = torch.tensor(ref.psi0(name), dtype=torch.float64, requires_grad=True)
    jod = call(m, name, psi)
    w = torch.tensor(ref.weights(name), dtype=torch.float32, device=DEV)
    (jod.reshape(-1) * w).sum().backward()
    for k, j in enumerate(jod.reshape(-1).tolist()):
        assert abs(j - ref.jod(name, ref.psi0(name), k)) < 1e-3
    cd, sc = ref.weighted(name, ref.central_differences)
    got = psi.grad.numpy()
    err = ref.normalised(got - cd, sc)
    print("%s: psi.grad %s\n  central differences %s\n  normalised error %s  worst %.3e  (bound %.3e)"
          % (name, got, cd, err, err.max(), 3 * worst))
    assert np.isfinite(got).all() and err.max() <= 3 * worst


@pytest.mark.parametrize("name", ["still_gamma_stack", "rgb_srgb_30", "gray_fov_gamma_60", "hdr_pq_30"])
def test_psi_grad_under_a_foreign_psi_is_that_of_a_metric_built_there(fv, name):
    """psi.grad at a psi that differs from the metric's own photometry in every entry, with more than one backward batch, is
    byte-identical to the gradient a second metric BUILT at that psi gives at its own parameters (and differs from the
    gradient at the first metric's own): the ingest of the backward batches and both sums entries read psi's block, not the
    metric's.  The first metric's photometry and context stay the same objects."""
    m = metric_for(fv, name)
    ph, state = m.display_photometry, dict(vars(m.display_photometry))
    own = m.display_parameter_tensor()
    w = torch.tensor(ref.weights(name), dtype=torch.float32, device=DEV)

    def grad(metric, values, gb):
        metric.grad_batch = gb
        psi = torch.tensor(values, dtype=torch.float64, requires_grad=True)
        jod = call(metric, name, psi)
        (jod.reshape(-1) * w).sum().backward()
        metric.grad_batch = None
        return jod.detach().cpu().numpy(), psi.grad.numpy()

    j_own, g_own = grad(m, own.tolist(), 2)
    ctx = m._ctx
    for factors in ([0.6, 1.7, 0.5, 2.0, 1.1], [1.37, 0.31, 2.2, 0.7, 0.93]):
        values = [float(a * b) for a, b in zip(ref.psi0(name), factors)]
        assert all(a != b for a, b in zip(values, own.tolist()))
        j, g = grad(m, values, 2)
        j2, g2 = grad(metric_for(fv, name, values), values, None)
        assert j.tobytes() == j2.tobytes() and g.tobytes() == g2.tobytes(), (g, g2)
        assert np.isfinite(g).all() and np.any(g != 0) and not np.array_equal(g, g_own) and not np.array_equal(j, j_own)
        assert m.display_photometry is ph and dict(vars(ph)) == state and m._ctx is ctx


# ---- 4. forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["still_gamma_stack", "rgb_srgb_30", "hdr_pq_30", "circular_30"])
def test_forward_is_predict_on_a_second_metric(fv, name):
    from fovvideovdp_amd import display_grad as dg
    m = metric_for(fv, name)
    ph, state = m.display_photometry, dict(vars(m.display_photometry))
    t, r, gaze = ref.inputs(name)
    still = ref.CASES[name][5] == 0
    p0 = ref.psi0(name)
    psis = [torch.tensor(p0, dtype=torch.float64),
            torch.tensor(p0 * [0.6, 1.7, 0.5, 2.0, 1.1], dtype=torch.float64),
            torch.tensor(p0 * [1.37, 0.31, 2.2, 0.7, 0.93], dtype=torch.float32)]
    call(m, name, psis[0])
    ctx = m._ctx
    assert ctx is not None
    for psi in psis:
        jod = call(m, name, psi)
        assert jod.grad_fn is None and jod.dtype == torch.float32 and jod.device == DEV
        vals = dg.psi_values(psi)
        e = dg.eotf_of(dg.photometry_of(m, vals))
        other = metric_for(fv, name, [float(v) for v in psi.tolist()])
        with torch.cuda.device(DEV):
            if still:
                td, rd = torch.from_numpy(t[:, :, 0]).to(DEV).contiguous(), torch.from_numpy(r[:, :, 0]).to(DEV).contiguous()
                j2, Q, _ = dg._images_forward(m, td, rd, None, e, False)
                q, stats = other.predict_images(t[:, :, 0], r[:, :, 0], dim_order="BCHW")
                want_Q = np.ascontiguousarray(np.asarray(stats["Q_per_ch"])[..., 0].transpose(1, 2, 0))
            else:
                td, rd = torch.from_numpy(t).to(DEV).contiguous(), torch.from_numpy(r).to(DEV).contiguous()
                fix = m._fixation(gaze, td.shape[4], td.shape[3], td.shape[2]) if m.foveated else None
                j2, Q, _ = dg._video_forward(m, td, rd, float(ref.CASES[name][6]), fix, e, False)
                q, stats = other.predict(t, r, dim_order="BCFHW", frames_per_second=ref.CASES[name][6], fixation_point=gaze)
                want_Q = np.asarray(stats["Q_per_ch"])
        assert jod.cpu().numpy().tobytes() == q.cpu().numpy().astype(np.float32).tobytes() == j2.cpu().numpy().tobytes()
        assert Q.cpu().numpy().tobytes() == np.ascontiguousarray(want_Q, dtype=np.float32).tobytes()
        assert m.display_photometry is ph and dict(vars(ph)) == state and m._ctx is ctx
    # a call that raises leaves them alone as well
    bad = psis[0].clone()
    bad[0] = -1.0
    with pytest.raises(RuntimeError, match="Y_peak must be positive"):
        call(m, name, bad)
    with pytest.raises(RuntimeError, match="same shape"):
        call(m, name, psis[0], rf=r[..., :-1])
    assert m.display_photometry is ph and dict(vars(ph)) == state and m._ctx is ctx


# ---- 5. dtype, device, batching, degenerate inputs, a step -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["still_gamma_stack", "pingpong_rgb"])
def test_psi_dtype_device_and_batching(fv, name):
    m = metric_for(fv, name)
    p0 = ref.psi0(name)
    grads = {}
    for dtype in (torch.float32, torch.float64):
        for dev in ("cpu", DEV):
            psi = torch.tensor(p0, dtype=dtype, device=dev, requires_grad=True)
            jod = call(m, name, psi)
            assert jod.grad_fn is not None
            jod.sum().backward()
            assert psi.grad.dtype == dtype and psi.grad.device == psi.device and psi.grad.shape == (5,)
            grads[(dtype, str(dev))] = psi.grad.cpu().double().numpy()
            with pytest.raises(RuntimeError):
                jod2 = call(m, name, psi)
                g, = torch.autograd.grad(jod2.sum(), psi, create_graph=True)
                g.sum().backward()                               # double backward
    assert np.array_equal(grads[(torch.float64, "cpu")], grads[(torch.float64, str(DEV))])
    assert np.array_equal(grads[(torch.float32, "cpu")], grads[(torch.float32, str(DEV))])
    ref_bytes = None
    for gb in (1, 2, None):
        m.grad_batch = gb
        psi = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
        call(m, name, psi).sum().backward()
        b = psi.grad.numpy().tobytes()
        ref_bytes = b if ref_bytes is None else ref_bytes
        assert b == ref_bytes, gb
    m.grad_batch = None
    # no grad mode, and a psi that does not require grad: the plain forward
    with torch.no_grad():
        assert call(m, name, torch.tensor(p0, requires_grad=True)).grad_fn is None


@pytest.mark.parametrize("name", ["still_gamma_stack", "gray_fov_gamma_60"])
def test_identical_inputs_give_jod_10_and_a_zero_gradient(fv, name):
    m = metric_for(fv, name)
    t, r, gaze = ref.inputs(name)
    psi = torch.tensor(ref.psi0(name), dtype=torch.float64, requires_grad=True)
    jod = call(m, name, psi, test=r, rf=r)
    assert torch.all(jod == 10.0)
    jod.sum().backward()
    assert torch.all(psi.grad == 0) and torch.isfinite(psi.grad).all()


def test_a_step_along_the_gradient_of_log_y_peak(fv):
    name = "rgb_srgb_30"
    m = metric_for(fv, name)
    p0 = torch.tensor(ref.psi0(name), dtype=torch.float64)
    lp = torch.tensor(math.log(float(p0[0])), dtype=torch.float64, requires_grad=True)

    def jod_at(l):
        return call(m, name, torch.cat([torch.exp(l).reshape(1), p0[1:]]))

    j0 = jod_at(lp)
    j0.backward()
    g = float(lp.grad)
    assert g != 0 and np.isfinite(g)
    eta = 0.05
    with torch.no_grad():
        up, down = float(jod_at(lp + eta * np.sign(g))), float(jod_at(lp - eta * np.sign(g)))
    print("dJOD/dlog Y_peak %.5f: JOD %.6f, +eta %.6f, -eta %.6f (predicted change %.6f)" % (g, float(j0.detach()), up, down, eta * abs(g)))
    assert up > float(j0.detach()) > down
    # the first-order prediction holds to within half of itself
    assert abs((up - float(j0.detach())) - eta * abs(g)) < 0.5 * eta * abs(g)
