"""Gradients of the JOD with respect to the display's photometry: fvvdp.display_jod_images / display_jod_video, the parameter
vector behind them and their autograd function (include/fvvdp_hip_display.h).

The five parameters of DISPLAY_PARAMETER_NAMES are the numeric constructor arguments of fvvdp_display_photo_eotf.  They enter
the metric only through the fvvdp_eotf block, which is an argument of every ingest: a call evaluates the sources under a vector
`psi` on the metric's ordinary native context with a block made from psi exactly as fvvdp._image_eotf makes it from the
metric's own photometry object, so the JOD is bit-identical to that of a metric built with
fvvdp_display_photo_eotf(Y_peak, contrast, EOTF, gamma, E_ambient, k_refl) from the same Python floats.  Nothing of the metric
is written and nothing is cached per psi.

When psi needs a gradient the forward also makes, per backward batch, one ingest under psi, one map-writing pyramid pass with
the slope planes on and the two level-0 backward passes of jod_images / jod_video(wrt="both") with gamma = 1; what their last
kernel would multiply by dL/dV and store is multiplied by dL/dpsi and summed instead (fvvdp_images_display_sums per batch,
fvvdp_video_display_sums once per stream after the last batch).  Only three sums per stream are kept -- [2, 3] doubles for a
clip, [B, 2, 3] for a stack -- and backward() is `chain`: float64 arithmetic on them, times the upstream gradient."""
import ctypes as C
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .display_model import fvvdp_display_photo_eotf, native_eotf
from .fvvdp import fvvdp as _fvvdp

DISPLAY_PARAMETER_NAMES = _fvvdp.DISPLAY_PARAMETER_NAMES
_IDX = {name: i for i, name in enumerate(DISPLAY_PARAMETER_NAMES)}
_POSITIVE = ("Y_peak", "contrast", "gamma")
_NON_NEGATIVE = ("E_ambient", "k_refl")
_SCALED = ("sRGB", "gamma")              # luminance = scale f(V) + Y_black; PQ and linear: clip(g(V), 0.005, Y_peak) + Y_black


def _stock_photometry(metric, name):
    ph = metric.display_photometry
    if type(ph) is not fvvdp_display_photo_eotf:
        raise RuntimeError("%s differentiates the five parameters of fvvdp_display_photo_eotf (sRGB, gamma, PQ or linear) and this "
                           "metric's photometry is a %s, which has no such parameters; build the metric with a "
                           "fvvdp_display_photo_eotf (gradients for the images or frames under any closed-form display: "
                           "jod_images / jod_video)" % (name, type(ph).__name__))
    if ph.EOTF not in ("sRGB", "gamma", "PQ", "linear"):
        raise RuntimeError("Unknown EOTF '%s'" % ph.EOTF)
    return ph


def display_parameter_tensor(metric):
    """The metric's current values of DISPLAY_PARAMETER_NAMES as a 1-D float64 host tensor."""
    ph = _stock_photometry(metric, "display_parameter_tensor")
    return torch.tensor([float(getattr(ph, name)) for name in DISPLAY_PARAMETER_NAMES], dtype=torch.float64)


def psi_values(psi):
    """psi (a 1-D tensor or sequence of the 5 values of DISPLAY_PARAMETER_NAMES) -> list of Python floats; refuses what no
    display can have.  A host tensor is read without touching the GPU."""
    t = psi.detach() if isinstance(psi, torch.Tensor) else torch.as_tensor(np.asarray(psi, dtype=np.float64))
    if t.dim() != 1 or t.shape[0] != len(DISPLAY_PARAMETER_NAMES):
        raise RuntimeError("psi must be a 1-D vector of the %d parameters of DISPLAY_PARAMETER_NAMES, got shape %s"
                           % (len(DISPLAY_PARAMETER_NAMES), tuple(t.shape)))
    if not t.is_floating_point():
        raise RuntimeError("psi must be a float32 or float64 tensor, got %s" % t.dtype)
    vals = [float(v) for v in t.to(device="cpu", dtype=torch.float64).tolist()]
    bad = [DISPLAY_PARAMETER_NAMES[i] for i, v in enumerate(vals) if not math.isfinite(v)]
    if bad:
        raise RuntimeError("psi has non-finite entries: %s" % ", ".join(bad))
    for name in _POSITIVE:
        if not vals[_IDX[name]] > 0:
            raise RuntimeError("psi: %s must be positive, got %g" % (name, vals[_IDX[name]]))
    for name in _NON_NEGATIVE:
        if vals[_IDX[name]] < 0:
            raise RuntimeError("psi: %s must not be negative, got %g" % (name, vals[_IDX[name]]))
    return vals


def photometry_of(metric, vals, name="display_jod_images"):
    """A fvvdp_display_photo_eotf with the values `vals` and the metric's own EOTF kind."""
    ph = _stock_photometry(metric, name)
    v = dict(zip(DISPLAY_PARAMETER_NAMES, vals))
    return fvvdp_display_photo_eotf(v["Y_peak"], contrast=v["contrast"], EOTF=ph.EOTF, gamma=v["gamma"],
                                    E_ambient=v["E_ambient"], k_refl=v["k_refl"], name=ph.name)


def set_display_parameters(metric, psi):
    """Gives the metric a new fvvdp_display_photo_eotf with the values of psi and the metric's own EOTF kind, through
    set_display_model (the geometry stays)."""
    vals = psi_values(psi)
    metric.set_display_model(display_photometry=photometry_of(metric, vals, "set_display_parameters"),
                             display_geometry=metric.display_geometry)


def eotf_of(photometry):
    """The fvvdp_eotf block of float samples under a stock photometry object: the conversions of fvvdp._image_eotf."""
    kind, d = native_eotf(photometry)
    e = nat.Eotf()
    e.kind = kind
    e.Y_peak = d.get("Y_peak", 0.0)
    e.Y_black = d.get("Y_black", 0.0)
    e.gamma = d.get("gamma", 1.0)
    e.L_min = d.get("L_min", 0.0)
    e.L_max = d.get("L_max", 0.0)
    return e


# ---- the chain: the three sums -> dJOD/dpsi ------------------------------------------------------------------------------
def chain(U, vals, eotf):
    """dJOD/dpsi [..., 5] float64 (a host tensor) from U [..., 3] = (U0, U1, U2), the sums of include/fvvdp_hip_display.h with the
    test's and the reference's added (any device and float dtype); vals: the values of psi; eotf: "sRGB", "gamma", "PQ" or
    "linear".  With Y_black = E k / pi + Y_peak / c and scale = Y_peak - Y_black, U0 = dJOD/dY_black, U2 = dJOD/dgamma, and U1 =
    dJOD/dscale (sRGB, gamma) or dJOD/dY_peak at fixed Y_black (PQ, linear: the upper luminance clip).  In numpy: backward()
    runs after the device has drained, so every microsecond here is one of the call's."""
    Yp, c, E, k, _ = vals
    U = U.detach().to(device="cpu", dtype=torch.float64).numpy()
    U0, U1, U2 = U[..., 0], U[..., 1], U[..., 2]
    zero = np.zeros_like(U2)
    if eotf in _SCALED:
        J = (U1 * (1.0 - 1.0 / c) + U0 / c, (U1 - U0) * (Yp / (c * c)), (U0 - U1) * (k / math.pi), (U0 - U1) * (E / math.pi),
             U2 if eotf == "gamma" else zero)
    else:
        J = (U1 + U0 / c, -U0 * (Yp / (c * c)), U0 * (k / math.pi), U0 * (E / math.pi), zero)
    return torch.from_numpy(np.stack(J, axis=-1))


# ---- the forward under psi -----------------------------------------------------------------------------------------------
def _images_forward(metric, t, r, fix, e, want_sums):
    """The launches of predict_images under the display block e -> (JOD [B], Q_per_ch [bands, 2, B], sums [B, 2, 3] float64 or
    None).  t, r: contiguous
    fp32 [B, C, H, W] on the metric's device."""
    from .image_grad import _Setup, grad_batch_size, grad_planes, slope_planes
    s = _Setup(metric, t)
    s.e = e
    B, dev, HW = s.B, metric.device, s.H * s.W
    Q = torch.zeros((s.n_bands, 2, B), dtype=torch.float32, device=dev)
    jod = torch.empty(B, dtype=torch.float32, device=dev)
    lib = nat.lib()
    for b0 in range(0, B, s.batch):
        nb = min(s.batch, B - b0)
        s.ingest(lib, t, r, b0, nb)
        fx, g, _keep = metric._fov_args(s.ctx, fix, b0, nb, s.n_bands, s.W, s.H)
        nat.check(lib.fvvdp_images_forward_pool(s.ctx.handle, nb, C.c_void_p(Q.data_ptr()), B, b0, fx, g, None, C.byref(s.pp),
                                                C.c_void_p(jod.data_ptr() + 4 * b0), s.stream))
    if not want_sums:
        return jod, Q, None
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, grad_planes("both"))
    maps_arr, _maps = metric._band_maps(gb, s.W, s.H, s.n_bands, contrast_planes=2)
    slopes, _slopes = slope_planes(metric, gb, s.W, s.H, s.n_bands)
    tb, rb = C.c_size_t(), C.c_size_t()
    nat.check(lib.fvvdp_images_display_sums_workspace(s.W, s.H, s.n_bands, gb, 0, C.byref(tb)))
    nat.check(lib.fvvdp_images_display_sums_workspace(s.W, s.H, s.n_bands, gb, 1, C.byref(rb)))
    work = torch.empty((max(tb.value, rb.value) + 7) // 8, dtype=torch.float64, device=dev)
    q_scratch = torch.empty((s.n_bands, 2, gb), dtype=torch.float32, device=dev)
    jod_scratch = torch.empty(gb, dtype=torch.float32, device=dev)
    ones = torch.ones(gb, dtype=torch.float32, device=dev)
    part = torch.empty((2, gb, nat.DISPLAY_SUMS), dtype=torch.float64, device=dev)
    sums = torch.empty((B, 2, nat.DISPLAY_SUMS), dtype=torch.float64, device=dev)
    prm = metric.native_params()
    for b0 in range(0, B, gb):
        nb = min(gb, B - b0)
        tp = s.ingest(lib, t, r, b0, nb)
        rp = (C.c_void_p * nb)(*[r[k].data_ptr() for k in range(b0, b0 + nb)])
        fx, g, _keep = metric._fov_args(s.ctx, fix, b0, nb, s.n_bands, s.W, s.H)
        nat.check(lib.fvvdp_ctx_set_slope_maps(s.ctx.handle, slopes))
        try:
            nat.check(lib.fvvdp_images_forward_pool(s.ctx.handle, nb, C.c_void_p(q_scratch.data_ptr()), nb, 0, fx, g, maps_arr,
                                                    C.byref(s.pp), C.c_void_p(jod_scratch.data_ptr()), s.stream))
        finally:
            nat.check(lib.fvvdp_ctx_set_slope_maps(s.ctx.handle, None))
        for side, (sl, ptrs, nbytes) in enumerate(((None, tp, tb.value), (slopes, rp, rb.value))):
            nat.check(lib.fvvdp_images_display_sums(s.W, s.H, s.n_bands, nb, C.byref(prm), C.byref(s.pp), C.c_void_p(Q.data_ptr()),
                                                    B, b0, C.c_void_p(ones.data_ptr()), maps_arr, sl, ptrs, s.C, HW, C.byref(s.e),
                                                    nat.fptr(s.w), C.c_void_p(part[side].data_ptr()),
                                                    C.c_void_p(work.data_ptr()), nbytes, s.stream))
        sums[b0:b0 + nb] = part[:, :nb].transpose(0, 1)
    return jod, Q, sums


def _video_forward(metric, t, r, fps, fix, e, want_sums):
    """The launches of predict (sync=False) under the display block e -> (JOD 0-d, Q_per_ch [bands, 2, N], sums [2, 3]
    float64 or None).  t, r: contiguous
    fp32 [1, C, N, H, W] on the metric's device."""
    from .image_grad import grad_batch_size
    from .video_grad import _Buffers, _Setup, _fold_arrays, fold_list, video_grad_planes
    s = _Setup(metric, t, fps)
    s.e = e
    N, dev, HW = s.N, metric.device, s.H * s.W
    nq = s.n_bands * 2 * N
    res = torch.zeros(nq + 2, dtype=torch.float32, device=dev)          # Q_per_ch | range flag | JOD, as predict lays it out
    Q = res[:nq].view(s.n_bands, 2, N)
    oob = res[nq:nq + 1].view(torch.int32)
    lib = nat.lib()
    for b0 in range(0, N, s.batch):
        nb = min(s.batch, N - b0)
        s.ingest(lib, t, r, b0, nb, oob)
        fx, g, _keep = metric._fov_args(s.ctx, fix, b0, nb, s.n_bands, s.W, s.H)
        if b0 + nb == N:
            nat.check(lib.fvvdp_bands_forward_pool(s.ctx.handle, nb, C.c_void_p(Q.data_ptr()), N, b0, fx, g, None,
                                                   C.byref(s.pp), C.c_void_p(res[nq + 1:].data_ptr()), s.stream))
        else:
            nat.check(lib.fvvdp_bands_forward(s.ctx.handle, nb, C.c_void_p(Q.data_ptr()), N, b0, fx, g, None, s.stream))
    if not want_sums:
        return res[nq + 1], Q, None
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, video_grad_planes("both"))
    vb, rb, sb = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    nat.check(lib.fvvdp_video_grad_workspace(s.W, s.H, s.n_bands, gb, C.byref(vb)))
    nat.check(lib.fvvdp_ref_grad_workspace(s.W, s.H, s.n_bands, gb, 2, C.byref(rb)))
    nat.check(lib.fvvdp_video_display_sums_workspace(s.W, s.H, C.byref(sb)))
    buf = _Buffers("display_jod_video", metric, s, t, gb, vb.value, True, rb.value, results=False)
    prm = metric.native_params()
    gamma = torch.ones(1, dtype=torch.float32, device=dev)
    for b0 in range(0, N, gb):
        nb = min(gb, N - b0)
        buf.maps_pass(lib, metric, s, t, r, fix, b0, nb)
        nat.check(lib.fvvdp_video_grad_frames(s.W, s.H, s.n_bands, nb, C.byref(prm), C.byref(s.pp), C.c_void_p(Q.data_ptr()), N, b0,
                                              C.c_void_p(gamma.data_ptr()), buf.maps_arr, C.c_void_p(buf.g0.data_ptr()),
                                              C.c_void_p(buf.work.data_ptr()), buf.work_bytes, s.stream))
        nat.check(lib.fvvdp_video_ref_grad_frames(s.W, s.H, s.n_bands, nb, C.byref(prm), C.byref(s.pp), C.c_void_p(Q.data_ptr()), N,
                                                  b0, C.c_void_p(gamma.data_ptr()), buf.maps_arr, buf.slopes,
                                                  C.c_void_p(buf.g0_r.data_ptr()), C.c_void_p(buf.work_r.data_ptr()),
                                                  buf.ref_bytes, s.stream))
    ff, fp = _fold_arrays(fold_list(s.widx, s.fl, N))
    work = torch.empty((sb.value + 7) // 8, dtype=torch.float64, device=dev)
    sums = torch.empty((2, nat.DISPLAY_SUMS), dtype=torch.float64, device=dev)
    for side, (g0, clip) in enumerate(((buf.g0, t), (buf.g0_r, r))):
        nat.check(lib.fvvdp_video_display_sums(s.W, s.H, N, C.c_void_p(g0.data_ptr()), ff.ctypes.data_as(C.POINTER(C.c_int32)),
                                               fp.ctypes.data_as(C.POINTER(C.c_int32)), nat.fptr(s.taps), s.fl,
                                               C.c_void_p(clip.data_ptr()), s.C, N * HW, HW, C.byref(s.e), nat.fptr(s.w),
                                               C.c_void_p(buf.head.data_ptr()), buf.head.numel() * 4,
                                               C.c_void_p(sums[side].data_ptr()), C.c_void_p(work.data_ptr()), sb.value, s.stream))
    return res[nq + 1], Q, sums


class _DisplayFunction(torch.autograd.Function):
    """psi -> JOD ([B] for images, 0-d for a clip).  `run(want_sums)` makes the forward under psi's values; the sums do not
    depend on the upstream gradient, so the forward forms them and keeps [..., 2, 3] doubles."""

    @staticmethod
    def forward(ctx, psi, metric, vals, eotf, run):
        want = bool(ctx.needs_input_grad[0])
        with torch.cuda.device(metric.device):
            jod, _, sums = run(want)
        if want:
            ctx.vals, ctx.eotf = vals, eotf
            ctx.psi_device, ctx.psi_dtype = psi.device, psi.dtype
            ctx.save_for_backward(sums)
        return jod.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_jod):
        sums, = ctx.saved_tensors
        # The chain is linear in the sums, so the upstream gradient is applied to them on the device (three small launches that
        # queue behind the forward's) and ONE read-back of three doubles follows: backward() waits for the device to drain, and
        # whatever it does after that is not hidden behind device work
        g = grad_jod.to(device=sums.device, dtype=torch.float64).reshape(-1, 1, 1)
        U = (g * sums.reshape(-1, 2, nat.DISPLAY_SUMS)).sum(dim=(0, 1))
        return chain(U, ctx.vals, ctx.eotf).to(device=ctx.psi_device, dtype=ctx.psi_dtype), None, None, None, None


def _refuse(name, metric, test, reference, other):
    for a in (test, reference):
        if isinstance(a, torch.Tensor) and a.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("%s differentiates the JOD with respect to the display's parameters only and this test or "
                               "reference requires grad; detach it (gradients for the images or frames: %s)" % (name, other))
    if metric.do_heatmap:
        raise RuntimeError("%s makes no heat maps: build the metric with heatmap=None (heat maps: predict)" % name)


def _need_float(name, test, reference):
    from .video_source import fvvdp_video_source_array
    t, r = fvvdp_video_source_array._as_tensor(test), fvvdp_video_source_array._as_tensor(reference)
    if t.dtype != torch.float32 or r.dtype != torch.float32:
        raise RuntimeError("%s needs float32 test and reference (got %s and %s): convert integer sources to float32 in [0, 1] -- "
                           "the integer path is a table of code values, not a closed form in the display's parameters -- and "
                           "float16 / bfloat16 sources with .float(): the reductions over the samples read float32"
                           % (name, t.dtype, r.dtype))
    return t, r


def _apply(metric, psi, vals, eotf, run):
    if isinstance(psi, torch.Tensor) and psi.requires_grad and torch.is_grad_enabled():
        return _DisplayFunction.apply(psi, metric, vals, eotf, run)
    with torch.cuda.device(metric.device):
        return run(False)[0]


def display_jod_images(metric, test, reference, psi, dim_order="BCHW", fixation_point=None):
    """fvvdp.display_jod_images (see there)."""
    from .fvvdp import _image_stack
    name = "display_jod_images"
    vals = psi_values(psi)
    ph = photometry_of(metric, vals, name)
    _refuse(name, metric, test, reference, "jod_images")
    t, r = _need_float(name, test, reference)
    t, r = _image_stack(t, r, dim_order)
    if t.shape[1] != 1 and t.shape[1] != 3:
        raise RuntimeError('The content must have either 1 or 3 colour channels.')
    metric._check_device()
    t, r = t.detach().to(metric.device).contiguous(), r.detach().to(metric.device).contiguous()
    fix = metric._fixation(fixation_point, t.shape[3], t.shape[2], t.shape[0]) if metric.foveated else None
    e = eotf_of(ph)
    return _apply(metric, psi, vals, ph.EOTF, lambda want: _images_forward(metric, t, r, fix, e, want))


def display_jod_video(metric, test, reference, psi, dim_order="BCFHW", frames_per_second=0, fixation_point=None):
    """fvvdp.display_jod_video (see there)."""
    from .video_grad import clip_arguments
    name = "display_jod_video"
    vals = psi_values(psi)
    ph = photometry_of(metric, vals, name)
    _refuse(name, metric, test, reference, "jod_video")
    t, r = _need_float(name, test, reference)
    t, r = clip_arguments(name, metric, t, r, dim_order, frames_per_second)
    metric._check_device()
    t, r = t.detach().to(metric.device).contiguous(), r.detach().to(metric.device).contiguous()
    fix = metric._fixation(fixation_point, t.shape[4], t.shape[3], t.shape[2]) if metric.foveated else None
    e = eotf_of(ph)
    fps = float(frames_per_second)
    return _apply(metric, psi, vals, ph.EOTF, lambda want: _video_forward(metric, t, r, fps, fix, e, want))
