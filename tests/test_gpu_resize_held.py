"""GPU: clips whose test and reference have frame sizes AND frame counts of their own (include/fvvdp_hip_resize_held.h,
fvvdp.predict_resized / fvvdp.jod_video_resized with test_frames= / reference_frames=).

  1. the ingest, bit for bit: level 0 after fvvdp_temporal_channels_resized_held against fvvdp_temporal_channels_resized on the
     clips expanded with index_select;
  2. the value: predict_resized with maps against predict_resized on the expanded clips, JOD and Q_per_ch bit for bit;
  3. the adjoint alone: fvvdp_resize_grad_held against resize_held_ref.adjoint in float64, test_gpu_resize.py's construction of the
     bound (4 x the float32 restatement's own error relative to the sum of a sample's absolute terms), exact zeros, a NaN-filled
     strided output, equal bits on a second run, fvvdp_resize_grad's bits with the identity map;
  4. the gradient end to end: against index_select under autograd into the existing jod_video_resized, with the bound of 3.
     evaluated by the restatement on the luminance gradient of the same call;
  5. equal bits across backward batches, placements, layouts and runs;
  6. the hand-over to today's calls.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd import resize_grad as rg
from fovvideovdp_amd.fvvdp import window_frame_indices
from fovvideovdp_amd.grad_passes import forward_clip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import held_cases as hc                      # noqa: E402
import resize_cases as rc                    # noqa: E402
import resize_held_cases as rhc              # noqa: E402
import resize_held_ref as rhr                # noqa: E402
import resize_ref as rref                    # noqa: E402
import yuv_channels_ref as yref              # noqa: E402
from lowlevel import Pipeline                # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
I32P = C.POINTER(C.c_int32)
ROTATION = [pytest.param(c, id=rhc.case_id(c)) for c in rhc.rotation()]


def product_photometry(model):
    if model == "gamma2.4":
        return dict(display_photometry=fv.fvvdp_display_photo_eotf(200, contrast=1000, EOTF="gamma", gamma=2.4, E_ambient=250,
                                                                   k_refl=0.005))
    return dict(display_name=model)


def stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def rgb2y():
    return np.asarray(yref.orc.load_defaults()["color_spaces.json"]["sRGB"]["RGB2Y"], np.float32)


def device_stream(x, pad=0):
    """test_gpu_resize.device_stream: (fvvdp_resize_stream, tensor to keep alive) of a clip [C, F, h, w]; pad: NaN-filled samples
    between consecutive planes."""
    Cn, F, h, w = x.shape
    t = torch.from_numpy(np.array(x))
    if pad:
        buf = torch.full((Cn, F, h * w + pad), float("nan") if t.dtype is torch.float32 else 255, dtype=t.dtype)
        buf[:, :, :h * w] = t.reshape(Cn, F, h * w)
        t = buf
    t = t.to(DEV)
    fs = h * w + pad
    return nat.ResizeStream(t.data_ptr(), nat.FVVDP_U8 if t.dtype is torch.uint8 else nat.FVVDP_F32, Cn, w, h, fs, F * fs), t


def u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---- 1. the ingest, bit for bit ------------------------------------------------------------------------------------------------------
def ingest_pair(m, mode, target, test, ref, m_t, m_r, fl, taps, widx, N, pad=0):
    """(level 0 of the held ingest on the streams, level 0 of the existing ingest on the expanded clips), [N, 4, Ho, Wo] each."""
    Wo, Ho = target
    _, e = m._image_eotf(torch.float32)
    widx = np.ascontiguousarray(widx, dtype=np.int32)
    it, ir = np.ascontiguousarray(np.asarray(m_t)[widx], np.int32), np.ascontiguousarray(np.asarray(m_r)[widx], np.int32)
    lib = nat.lib()
    out = []
    for held in (True, False):
        pipe = Pipeline(m, Wo, Ho, 4, N)
        try:
            if held:
                ts, keep_t = device_stream(test, pad)
                rs, keep_r = device_stream(ref)
                nat.check(lib.fvvdp_temporal_channels_resized_held(pipe.handle, C.byref(ts), C.byref(rs), test.shape[1], ref.shape[1],
                                                                   nat.RESIZE_MODES[mode], C.byref(e), nat.fptr(rgb2y()),
                                                                   it.ctypes.data_as(I32P), ir.ctypes.data_as(I32P), nat.fptr(taps), fl, N, 0,
                                                                   stream()))
            else:
                ts, keep_t = device_stream(rhr.expand(test, m_t), pad)
                rs, keep_r = device_stream(rhr.expand(ref, m_r))
                nat.check(lib.fvvdp_temporal_channels_resized(pipe.handle, C.byref(ts), C.byref(rs), nat.RESIZE_MODES[mode], C.byref(e),
                                                              nat.fptr(rgb2y()), widx.ctypes.data_as(I32P), nat.fptr(taps), fl, N, 0,
                                                              stream()))
            out.append(pipe.export_level(0, N).cpu().numpy())
        finally:
            pipe.close()
    return out


@pytest.mark.parametrize("c", ROTATION)
def test_ingest_bit_for_bit(c):
    m = fv.fvvdp(temp_padding=c["padding"], quiet=True, device=DEV, **product_photometry(c["display"]))
    fl, taps = m._temporal_taps(c["fps"])
    N = rc.RING[c["fps"]] + 3
    assert (8 if fl <= 8 else 16 if fl <= 16 else 32) == rc.RING[c["fps"]]
    test, ref, m_t, m_r = rhc.inputs(c)
    widx = window_frame_indices(N, fl, c["padding"])
    got, want = ingest_pair(m, c["mode"], c["target"], test, ref, m_t, m_r, fl, taps, widx, N, pad=4 if c["fps"] == 60 else 0)
    assert np.isfinite(want).all() and want.any()
    assert np.array_equal(u32(got), u32(want)), rhc.case_id(c)
    # a map that holds frames gives a list that repeats entries: a reuse happens (`skipping` alone holds nothing)
    if c["maps"] != "skipping":
        lists = [np.asarray(mm)[np.asarray(widx)] for mm in (m_t, m_r)]
        assert any((np.diff(lst) == 0).any() for lst in lists)


def test_ingest_two_launch_windows():
    """fl - 1 + n_out beyond the list of one launch (fl = 8, 320 outputs): two launch windows, and the first step of the second
    converts its frames whatever the list held before it."""
    N, target, source = 320, (120, 68), (60, 34)
    m = fv.fvvdp(quiet=True, device=DEV, display_name="standard_fhd")
    fl, taps = m._temporal_taps(30)
    assert fl == 8 and fl - 1 + N > 320
    rng = np.random.default_rng(320)
    m_t, F_t = hc.c_abi_map("hold2", N)
    m_r = np.arange(N, dtype=np.int32)
    test = rng.uniform(-0.1, 1.1, (1, F_t, source[1], source[0])).astype(np.float32)
    ref = rng.integers(0, 256, (1, N, target[1], target[0])).astype(np.uint8)
    widx = window_frame_indices(N, fl, "replicate")
    got, want = ingest_pair(m, "bilinear", target, test, ref, m_t, m_r, fl, taps, widx, N)
    assert np.array_equal(u32(got), u32(want))
    assert want[-1].any() and want[313:].any()                    # the second window's outputs are there


# ---- 2. the value --------------------------------------------------------------------------------------------------------------------
# name: (N display frames, C, source, target, mode, display, fps, padding, maps, foveated)
E2E = {
    "k2_bilinear_srgb": (12, 3, (60, 34), (120, 68), "bilinear", "standard_fhd", 30, "replicate", "k2", False),
    "k4_bicubic_pq": (20, 3, (80, 46), (122, 68), "bicubic", "standard_hdr_pq", 60, "circular", "k4", False),
    "both_area_gamma": (12, 3, (240, 136), (120, 68), "area", "gamma2.4", 30, "pingpong", "both", False),
    "skip_nearest_fov": (11, 1, (40, 23), (120, 68), "nearest", "standard_4k", 30, "replicate", "skipping", True),
}
_E2E = {}


def e2e_inputs(name):
    """(test float32 [C, F_t, h, w], reference float32 [C, F_r, Ho, Wo], m_t, m_r, gaze or None): the reference is what its frame
    first shows of the resized, clipped test, plus noise -- the JOD is neither 10 nor at the floor."""
    if name not in _E2E:
        N, Cn, source, target, mode, display, fps, padding, maps, fov = E2E[name]
        m_t, F_t, m_r, F_r = rhc.case_maps(maps, N)
        seed = 2700 + sorted(E2E).index(name)
        test, _ = rc.draw_clip([seed], Cn, F_t, source, target, mode)
        base = np.clip(rref.resize(test.astype(np.float64), target, mode), 0, 1)
        first = [int(m_t[int(np.argmax(m_r == j))]) if (m_r == j).any() else 0 for j in range(F_r)]
        rng = np.random.default_rng([seed, 1])
        ref = np.clip(base[:, first] + rng.normal(0, 0.05, (Cn, F_r, target[1], target[0])), 0, 1).astype(np.float32)
        gaze = None
        if fov:
            s = np.linspace(0.2, 0.8, N)
            gaze = np.stack([s * target[0], (1 - s) * target[1]], axis=1).astype(np.float32)
        test.setflags(write=False)
        ref.setflags(write=False)
        _E2E[name] = (test, ref, m_t, m_r, gaze)
    return _E2E[name]


def e2e_metric(name):
    N, Cn, source, target, mode, display, fps, padding, maps, fov = E2E[name]
    return fv.fvvdp(foveated=fov, temp_padding=padding, quiet=True, device=DEV, heatmap=None, **product_photometry(display))


def e2e_kw(name, held=True):
    N, Cn, source, target, mode, display, fps, padding, maps, fov = E2E[name]
    test, ref, m_t, m_r, gaze = e2e_inputs(name)
    kw = dict(full_screen_resize=mode, resize_resolution=target, frames_per_second=fps, dim_order="CFHW")
    if gaze is not None:
        kw["fixation_point"] = torch.from_numpy(gaze)
    if held:
        # an int where the map is one, a sequence otherwise
        kt = rhc.MAPS[maps][0]
        kw["test_frames"] = int(kt[4:]) if kt.startswith("hold") and N % int(kt[4:]) == 0 else m_t
        kw["reference_frames"] = 1 if rhc.MAPS[maps][1] == "identity" else m_r
    return kw


def sel(x, m):
    return x.index_select(1, torch.as_tensor(np.asarray(m), dtype=torch.int64, device=x.device))


@pytest.mark.parametrize("name", sorted(E2E))
def test_value_is_predict_resized_on_the_expanded_clips(name):
    m = e2e_metric(name)
    test, ref, m_t, m_r, gaze = e2e_inputs(name)
    t, r = torch.from_numpy(test.copy()).to(DEV), torch.from_numpy(ref.copy()).to(DEV)
    got, stats = m.predict_resized(t, r, **e2e_kw(name))
    want, wstats = m.predict_resized(sel(t, m_t).contiguous(), sel(r, m_r).contiguous(), **e2e_kw(name, held=False))
    print("\n%s: JOD %.6f" % (name, float(got)))
    assert 0 < float(want) < 10
    assert torch.equal(got, want) and np.array_equal(u32(stats["Q_per_ch"]), u32(wstats["Q_per_ch"]))
    assert stats["N_frames"] == E2E[name][0] == wstats["N_frames"] and (stats["width"], stats["height"]) == E2E[name][3]
    with torch.no_grad():
        jn = m.jod_video_resized(t, r, **e2e_kw(name))
    assert jn.grad_fn is None and torch.equal(jn, want)
    # a uint8 reference goes the same way
    r8 = (r * 255).round().to(torch.uint8)
    got8, _ = m.predict_resized(t, r8, **e2e_kw(name))
    want8, _ = m.predict_resized(sel(t, m_t).contiguous(), sel(r8, m_r).contiguous(), **e2e_kw(name, held=False))
    assert torch.equal(got8, want8)


# ---- 3. the adjoint alone --------------------------------------------------------------------------------------------------------------
def run_adjoint(m, c, test, m_map, gL, pad, identity_call=False):
    """fvvdp_resize_grad_held (or fvvdp_resize_grad: identity_call) into a NaN-filled buffer with `pad` samples between the planes;
    the workspace holds two frames of the first stage.  Returns [C, F, h, w]."""
    Cn, F, h, w = test.shape
    Wo, Ho = c["target"]
    N = gL.shape[0]
    ts, keep = device_stream(test, pad)
    _, e = m._image_eotf(torch.float32)
    gLd = torch.from_numpy(gL).to(DEV)
    tables = nat.resize_grad_table_bytes(w, h) if identity_call else nat.resize_grad_held_table_bytes(w, h, F)
    work_bytes = tables + 4 * 2 * Cn * Ho * Wo
    work = torch.empty(work_bytes, dtype=torch.uint8, device=DEV)
    out = torch.full((Cn, F, h * w + pad), float("nan"), device=DEV)
    mm = None if identity_call else np.ascontiguousarray(m_map, dtype=np.int32)
    if identity_call:
        nat.check(nat.lib().fvvdp_resize_grad(Wo, Ho, N, C.c_void_p(gLd.data_ptr()), C.byref(ts), C.c_void_p(out.data_ptr()),
                                              nat.RESIZE_MODES[c["mode"]], C.byref(e), nat.fptr(rgb2y()), C.c_void_p(work.data_ptr()),
                                              work_bytes, stream()))
    else:
        nat.check(nat.lib().fvvdp_resize_grad_held(Wo, Ho, N, F, C.c_void_p(gLd.data_ptr()), mm.ctypes.data_as(I32P), C.byref(ts),
                                                   C.c_void_p(out.data_ptr()), nat.RESIZE_MODES[c["mode"]], C.byref(e), nat.fptr(rgb2y()),
                                                   C.c_void_p(work.data_ptr()), work_bytes, stream()))
    res = out.cpu().numpy()
    assert np.isnan(res[:, :, h * w:]).all()                                      # what lies between the planes is not written
    return res[:, :, :h * w].reshape(Cn, F, h, w)


def adjoint_bound(gL, test, m_map, c, display):
    """(g64, S, e_ref): the float64 adjoint, the sum of every sample's absolute terms, and the float32 restatement's own error
    relative to it."""
    kind, kw = rref.eotf_args(yref.photometry_for(display))
    a = (gL, test, m_map, c["target"], c["mode"], rgb2y(), kind)
    g64 = rhr.adjoint(*a, dtype=np.float64, **kw)
    g32 = rhr.adjoint(*a, dtype=np.float32, **kw)
    S = rhr.adjoint(*a, dtype=np.float64, absolute=True, **kw)
    nz = S != 0
    e_ref = float((np.abs(g32.astype(np.float64) - g64)[nz] / S[nz]).max())
    return g64, S, e_ref


@pytest.mark.parametrize("c", ROTATION)
def test_adjoint_per_sample(c):
    N = 6
    m = fv.fvvdp(quiet=True, device=DEV, **product_photometry(c["display"]))
    test, _, m_t, _ = rhc.inputs(c, N)
    Cn, F, h, w = test.shape
    gL = rhc.gl_for(c, N)
    g64, S, e_ref = adjoint_bound(gL, test, m_t, c, c["display"])
    pad = 8 if Cn == 3 else 0
    got = run_adjoint(m, c, test, m_t, gL, pad)
    again = run_adjoint(m, c, test, m_t, gL, pad)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))             # equal bits on a second run
    assert np.isfinite(got).all()                                                 # every sample was written (the buffer held NaN)
    zero = S == 0                                 # a frame never shown, every reaching target clipped, or skipped by a downscale
    assert (got[zero] == 0).all() and (g64[zero] == 0).all()
    shown = np.zeros(F, bool)
    shown[m_t] = True
    assert zero[:, ~shown].all()                  # every sample of a frame no display frame shows
    if c["maps"] == "skipping":
        assert (~shown).sum() >= 2
    if c["mode"] == "nearest" and c["source"] != (7, 5):
        assert zero[:, shown].any()               # samples whose targets are all clipped (a third of them and more at these sizes)
    if c["source"] == (240, 136) and c["mode"] == "nearest":
        assert zero[:, shown].mean() > 0.5        # x0.5: three of four samples are skipped
    err = float((np.abs(got.astype(np.float64) - g64)[~zero] / S[~zero]).max())
    bound = yref.error_bound(e_ref)
    print("\nheld resize adjoint %s: err %.3g e_ref %.3g bound %.3g, %d exact zeros of %d" % (rhc.case_id(c), err, e_ref, bound,
                                                                                             int(zero.sum()), zero.size))
    assert err <= bound


@pytest.mark.parametrize("c", ROTATION[::3])
def test_adjoint_identity_map_is_resize_grad(c):
    N = 5
    m = fv.fvvdp(quiet=True, device=DEV, **product_photometry(c["display"]))
    test = rc.rotation_inputs(c, N)[0]
    gL = rhc.gl_for(c, N)
    pad = 8 if test.shape[0] == 3 else 0
    got = run_adjoint(m, c, test, np.arange(N), gL, pad)
    want = run_adjoint(m, c, test, None, gL, pad, identity_call=True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- 4. the gradient end to end ----------------------------------------------------------------------------------------------------------
def e2e_grad(m, name, device=DEV):
    test, ref, m_t, m_r, gaze = e2e_inputs(name)
    t = torch.from_numpy(test.copy()).to(device).requires_grad_(True)
    r = torch.from_numpy(ref.copy()).to(device)
    jod = m.jod_video_resized(t, r, **e2e_kw(name))
    jod.backward()
    return jod.detach(), t.grad


@pytest.mark.parametrize("name", sorted(E2E))
def test_gradient_against_autograd_through_index_select(name):
    """The existing jod_video_resized on index_select(test) under autograd sums the per-display-frame adjoints of a source frame in
    torch's index_add; the held path sums the luminance gradient over the run first.  The two differ by float32 rounding of the
    same terms: per sample, relative to the sum of its absolute terms, within 4 x the float32 restatement's own error, the
    restatement evaluated on the luminance gradient of this very call."""
    N, Cn, source, target, mode, display, fps, padding, maps, fov = E2E[name]
    m = e2e_metric(name)
    test, ref, m_t, m_r, gaze = e2e_inputs(name)
    jod, g = e2e_grad(m, name)
    t2 = torch.from_numpy(test.copy()).to(DEV).requires_grad_(True)
    r = torch.from_numpy(ref.copy()).to(DEV)
    j2 = m.jod_video_resized(sel(t2, m_t), sel(r, m_r).contiguous(), **e2e_kw(name, held=False))
    j2.backward()
    assert torch.equal(jod, j2.detach()) and 0 < float(jod) < 10
    got, want = g.cpu().numpy(), t2.grad.cpu().numpy()
    # the luminance gradient of the call, through the launch layer's own seam
    cfg = (float(fps), nat.RESIZE_MODES[mode], target, (m_t, m_r))
    with torch.cuda.device(DEV):
        tp, rp = torch.from_numpy(test.copy()).to(DEV), r
        fix = m._fixation(None if gaze is None else torch.from_numpy(gaze), target[0], target[1], N) if fov else None
        jf, Q = forward_clip(rg._setup(m, tp, rp, cfg), fix)
        _, gL, _ = rg._luminance_grad(m, tp, rp, cfg, fix, Q, torch.ones(1))
    assert torch.equal(jf, jod)
    g64, S, e_ref = adjoint_bound(gL.cpu().numpy(), test, m_t, dict(target=target, mode=mode), display)
    zero = S == 0
    assert (got[zero] == 0).all() and (want[zero] == 0).all()
    shown = np.zeros(test.shape[1], bool)
    shown[m_t] = True
    assert (got[:, ~shown] == 0).all()
    bound = yref.error_bound(e_ref)
    ratio = float((np.abs(got.astype(np.float64) - want)[~zero] / S[~zero]).max())
    r64 = float((np.abs(got.astype(np.float64) - g64)[~zero] / S[~zero]).max())
    print("\n%s: JOD %.6f, held against index_select %.3g, held against float64 %.3g, e_ref %.3g, bound %.3g"
          % (name, float(jod), ratio, r64, e_ref, bound))
    assert g.any() and ratio <= bound and r64 <= bound


def test_identical_streams_give_ten_and_zeros():
    """The same tensor as test and reference under the same map, both resized: JOD == 10 and exact zeros."""
    test, _ = rc.draw_clip([56], 3, 5, (60, 34), (122, 68), "bilinear")
    m = fv.fvvdp(display_name="standard_4k", quiet=True, device=DEV)
    t = torch.from_numpy(test).to(DEV).requires_grad_(True)
    jod = m.jod_video_resized(t, t.detach().clone(), full_screen_resize="bilinear", resize_resolution=(122, 68), dim_order="CFHW",
                              frames_per_second=30, test_frames=2, reference_frames=2)
    jod.backward()
    assert float(jod.detach()) == 10.0
    assert bool(torch.isfinite(t.grad).all()) and bool((t.grad == 0).all())


# ---- 5. equal bits ------------------------------------------------------------------------------------------------------------------------
def test_grad_batch_placement_and_layout_give_equal_bits():
    name = "k2_bilinear_srgb"
    grads, jods = {}, {}
    for gb in (None, 1, 2):
        m = e2e_metric(name)
        m.grad_batch = gb
        jods[gb], grads[gb] = e2e_grad(m, name)
    assert torch.equal(grads[None], grads[1]) and torch.equal(grads[None], grads[2]) and torch.equal(jods[None], jods[1])
    m = e2e_metric(name)
    j2, g2 = e2e_grad(m, name)                                                     # a second run
    assert torch.equal(g2, grads[None]) and torch.equal(j2, jods[None])
    jh, gh = e2e_grad(m, name, device="cpu")                                       # host-resident inputs: the gradient on the host
    assert torch.equal(jh, jods[None]) and gh.device.type == "cpu" and torch.equal(gh, grads[None].cpu())
    test, ref, m_t, m_r, _ = e2e_inputs(name)
    kw = e2e_kw(name)
    t, r = torch.from_numpy(test.copy()).to(DEV), torch.from_numpy(ref.copy()).to(DEV)
    tp = t.permute(1, 2, 3, 0).contiguous().requires_grad_(True)                   # [F, h, w, C]
    jp = m.jod_video_resized(tp, r.permute(1, 2, 3, 0).contiguous(), **dict(kw, dim_order="FHWC"))
    jp.backward()
    assert torch.equal(jp.detach(), jods[None]) and tp.grad.shape == tp.shape and torch.equal(tp.grad.permute(3, 0, 1, 2), grads[None])
    tf = t.permute(1, 0, 2, 3).contiguous()[None].requires_grad_(True)             # [1, F, C, h, w]: read where it lies
    jf = m.jod_video_resized(tf, r.permute(1, 0, 2, 3).contiguous()[None], **dict(kw, dim_order="BFCHW"))
    jf.backward()
    assert torch.equal(jf.detach(), jods[None]) and torch.equal(tf.grad[0].permute(1, 0, 2, 3), grads[None])


# ---- 6. the hand-over ------------------------------------------------------------------------------------------------------------------------
def test_identity_maps_are_todays_calls():
    name = "a_bilinear_x2_srgb_30"
    N, Cn, source, target, mode, display, fps, padding, opt = rc.CASES[name]
    m = fv.fvvdp(display_name=display, temp_padding=padding, quiet=True, device=DEV)
    test, ref = rc.case_inputs(name)
    kw = dict(full_screen_resize=mode, resize_resolution=target, frames_per_second=fps, dim_order="CFHW")
    ident = dict(test_frames=np.arange(N), reference_frames=list(range(N)))
    t, r = torch.from_numpy(test.copy()).to(DEV), torch.from_numpy(ref.copy()).to(DEV)
    q, stats = m.predict_resized(t, r, **kw)
    q2, stats2 = m.predict_resized(t, r, **kw, **ident)
    assert torch.equal(q, q2) and np.array_equal(u32(stats["Q_per_ch"]), u32(stats2["Q_per_ch"]))
    a, b = t.clone().requires_grad_(True), t.clone().requires_grad_(True)
    ja, jb = m.jod_video_resized(a, r, **kw), m.jod_video_resized(b, r, **kw, **ident)
    ja.backward()
    jb.backward()
    assert torch.equal(ja, jb) and torch.equal(a.grad, b.grad)
    # both streams at the target size: predict's and jod_video's
    rng = np.random.default_rng(6)
    tt = torch.from_numpy(np.clip(ref + rng.normal(0, 0.03, ref.shape), 0, 1).astype(np.float32)).to(DEV)
    q, stats = m.predict(tt, r, dim_order="CFHW", frames_per_second=fps)
    q2, stats2 = m.predict_resized(tt, r, **kw, **ident)
    assert torch.equal(q, q2) and np.array_equal(u32(stats["Q_per_ch"]), u32(stats2["Q_per_ch"]))
    a, b = tt.clone().requires_grad_(True), tt.clone().requires_grad_(True)
    ja, jb = m.jod_video(a, r, dim_order="CFHW", frames_per_second=fps), m.jod_video_resized(b, r, **kw, **ident)
    ja.backward()
    jb.backward()
    assert torch.equal(ja, jb) and torch.equal(a.grad, b.grad)
    # ... and with a map that is not the identity: predict_held's and jod_video_held's
    half = tt[:, ::2].contiguous()
    q, stats = m.predict_held(half, r, dim_order="CFHW", frames_per_second=fps, test_frames=2)
    q2, stats2 = m.predict_resized(half, r, **kw, test_frames=2)
    assert torch.equal(q, q2) and np.array_equal(u32(stats["Q_per_ch"]), u32(stats2["Q_per_ch"]))
    a, b = half.clone().requires_grad_(True), half.clone().requires_grad_(True)
    ja = m.jod_video_held(a, r, dim_order="CFHW", frames_per_second=fps, test_frames=2)
    jb = m.jod_video_resized(b, r, **kw, test_frames=2)
    ja.backward()
    jb.backward()
    assert torch.equal(ja, jb) and torch.equal(a.grad, b.grad)
