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
clip, [B, 2, 3] for a stack -- and backward() is `chain`: float64 arithmetic on them, times the upstream gradient.
The setups (with psi's display block), both forward loops, the map-writing passes, the buffers and the level-0 backward are
grad_passes.py's, shared with the other differentiable entry points."""
import ctypes as C
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .display_model import fvvdp_display_photo_eotf, native_eotf
from .fvvdp import _image_stack, fvvdp as _fvvdp
from .grad_passes import (ClipSetup, ImageSetup, Maps, _apply, _fold_arrays, _ptr, _refuse, batches, fold_list, forward_clip,
                          forward_images, grad_batch_size, level0_backward, level0_buffers, vector_values, work_tensor,
                          workspace_bytes)
from .image_grad import grad_planes
from .video_grad import clip_arguments, video_grad_planes
from .video_source import fvvdp_video_source_array

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
    vals = vector_values("psi", "DISPLAY_PARAMETER_NAMES", psi)
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
    s = ImageSetup(metric, t, r, eotf=e)
    B, dev, HW = s.B, metric.device, s.H * s.W
    jod, Q = forward_images(s, fix)
    if not want_sums:
        return jod, Q, None
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, grad_planes("both"))
    maps = Maps(metric, s.W, s.H, s.n_bands, 2, gb).add_slopes()
    lib = nat.lib()
    tb = workspace_bytes(lib.fvvdp_images_display_sums_workspace, s.W, s.H, s.n_bands, gb, 0)
    rb = workspace_bytes(lib.fvvdp_images_display_sums_workspace, s.W, s.H, s.n_bands, gb, 1)
    work = work_tensor(max(tb, rb), torch.float64)
    ones = torch.ones(gb, dtype=torch.float32, device=dev)
    part = torch.empty((2, gb, nat.DISPLAY_SUMS), dtype=torch.float64, device=dev)
    sums = torch.empty((B, 2, nat.DISPLAY_SUMS), dtype=torch.float64, device=dev)
    prm = s.params()
    for b0, nb in batches(B, gb):
        tp = s.write_maps(maps, fix, b0, nb)
        rp = (C.c_void_p * nb)(*[r[k].data_ptr() for k in range(b0, b0 + nb)])
        for side, (sl, ptrs, nbytes) in enumerate(((None, tp, tb), (maps.slopes, rp, rb))):
            nat.check(lib.fvvdp_images_display_sums(s.W, s.H, s.n_bands, nb, C.byref(prm), C.byref(s.pp), _ptr(Q), B, b0,
                                                    _ptr(ones), maps.maps_arr, sl, ptrs, s.C, HW, C.byref(s.e), nat.fptr(s.w),
                                                    _ptr(part[side]), _ptr(work), nbytes, s.stream))
        sums[b0:b0 + nb] = part[:, :nb].transpose(0, 1)
    return jod, Q, sums


def _video_forward(metric, t, r, fps, fix, e, want_sums):
    """The launches of predict (sync=False) under the display block e -> (JOD 0-d, Q_per_ch [bands, 2, N], sums [2, 3]
    float64 or None).  t, r: contiguous
    fp32 [1, C, N, H, W] on the metric's device."""
    s = ClipSetup(metric, t, fps, r, eotf=e)
    N, dev, HW = s.N, metric.device, s.H * s.W
    jod, Q = forward_clip(s, fix)
    if not want_sums:
        return jod, Q, None
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, video_grad_planes("both"))
    lib = nat.lib()
    buf = level0_buffers("display_jod_video", metric, s, t, gb, True, True, results=False)
    sb = workspace_bytes(lib.fvvdp_video_display_sums_workspace, s.W, s.H)
    prm = s.params()
    gamma = torch.ones(1, dtype=torch.float32, device=dev)
    for b0, nb in batches(N, gb):
        buf.maps_pass(lib, metric, s, t, r, fix, b0, nb)
        level0_backward(buf, s, prm, Q, N, b0, nb, gamma)
    ff, fp = _fold_arrays(fold_list(s.widx, s.fl, N))
    work = work_tensor(sb, torch.float64)
    sums = torch.empty((2, nat.DISPLAY_SUMS), dtype=torch.float64, device=dev)
    for side, (g0, clip) in enumerate(((buf.g0, t), (buf.g0_r, r))):
        nat.check(lib.fvvdp_video_display_sums(s.W, s.H, N, _ptr(g0), ff.ctypes.data_as(C.POINTER(C.c_int32)),
                                               fp.ctypes.data_as(C.POINTER(C.c_int32)), nat.fptr(s.taps), s.fl, _ptr(clip), s.C,
                                               N * HW, HW, C.byref(s.e), nat.fptr(s.w), _ptr(buf.head), buf.head.numel() * 4,
                                               _ptr(sums[side]), _ptr(work), sb, s.stream))
    return jod, Q, sums


class _DisplayFunction(torch.autograd.Function):
    """psi -> JOD ([B] for images, 0-d for a clip).  `run(want_sums)` makes the forward under psi's values; the sums do not
    depend on the upstream gradient, so the forward forms them and keeps [..., 2, 3] doubles."""

    @staticmethod
    def forward(ctx, psi, metric, run, vals, eotf):
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


def _need_float(name, test, reference):
    t, r = fvvdp_video_source_array._as_tensor(test), fvvdp_video_source_array._as_tensor(reference)
    if t.dtype != torch.float32 or r.dtype != torch.float32:
        raise RuntimeError("%s needs float32 test and reference (got %s and %s): convert integer sources to float32 in [0, 1] -- "
                           "the integer path is a table of code values, not a closed form in the display's parameters -- and "
                           "float16 / bfloat16 sources with .float(): the reductions over the samples read float32"
                           % (name, t.dtype, r.dtype))
    return t, r


def display_jod_images(metric, test, reference, psi, dim_order="BCHW", fixation_point=None):
    """fvvdp.display_jod_images (see there)."""
    name = "display_jod_images"
    vals = psi_values(psi)
    ph = photometry_of(metric, vals, name)
    _refuse(name, "the display's parameters", metric, test, reference, "jod_images", " (heat maps: predict)")
    t, r = _need_float(name, test, reference)
    t, r = _image_stack(t, r, dim_order)
    if t.shape[1] != 1 and t.shape[1] != 3:
        raise RuntimeError('The content must have either 1 or 3 colour channels.')
    metric._check_device()
    t, r = t.detach().to(metric.device).contiguous(), r.detach().to(metric.device).contiguous()
    fix = metric._fixation(fixation_point, t.shape[3], t.shape[2], t.shape[0]) if metric.foveated else None
    e = eotf_of(ph)
    run = lambda want: _images_forward(metric, t, r, fix, e, want)          # noqa: E731
    return _apply(_DisplayFunction, metric, psi, run, vals, ph.EOTF)


def display_jod_video(metric, test, reference, psi, dim_order="BCFHW", frames_per_second=0, fixation_point=None):
    """fvvdp.display_jod_video (see there)."""
    name = "display_jod_video"
    vals = psi_values(psi)
    ph = photometry_of(metric, vals, name)
    _refuse(name, "the display's parameters", metric, test, reference, "jod_video", " (heat maps: predict)")
    t, r = _need_float(name, test, reference)
    t, r = clip_arguments(name, metric, t, r, dim_order, frames_per_second)
    metric._check_device()
    t, r = t.detach().to(metric.device).contiguous(), r.detach().to(metric.device).contiguous()
    fix = metric._fixation(fixation_point, t.shape[4], t.shape[3], t.shape[2]) if metric.foveated else None
    e = eotf_of(ph)
    fps = float(frames_per_second)
    run = lambda want: _video_forward(metric, t, r, fps, fix, e, want)          # noqa: E731
    return _apply(_DisplayFunction, metric, psi, run, vals, ph.EOTF)
