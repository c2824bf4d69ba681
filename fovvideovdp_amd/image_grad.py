"""Differentiable still-image JOD: fvvdp.jod_images and its autograd function (include/fvvdp_hip_grad.h).

The forward makes the launches of fvvdp.predict_images (fvvdp_images_channels + fvvdp_images_forward_pool) with arguments from
the same methods of the metric, so the JODs are bit-identical to it.  The backward re-runs them per backward batch with every
band's maps written (band contrast, L_bkg, S, D), then fvvdp_images_grad turns the maps and the forward's Q_per_ch into
dJOD/dtest on the device.  Neither pass reads context scratch left by the other, and neither synchronises with the host."""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .display_model import native_eotf
from .fvvdp import _image_stack

# Device memory one backward batch (of image pairs, or of video frames: video_grad.py) may hold in maps and workspace; the
# pyramid scratch of the context comes on top.  For video that is 52 B per pyramid pixel and frame, 0.58 GB per 3840x2160
# frame.  Chosen on the arithmetic alone (seven 4K frames per batch keep every launch of the batch above 10^7 band pixels,
# the clip-long buffers of a 60-frame 4K clip -- 10 GB -- fit beside it many times in 288 GB); not tuned on a measurement.
GRAD_BYTES_BUDGET = 4e9
# fp32 planes per pyramid pixel and pair: maps (D 2 + contrast 2 + L_bkg 1 + S 2) and workspace (layer + sweep gradients)
GRAD_PLANES = 7 + 2


class _Setup:
    """What forward and backward share for one [B, C, H, W] stack: pyramid size, display model, context, launch constants."""

    def __init__(self, metric, t):
        self.B, self.C, self.H, self.W = t.shape
        self.n_bands, self.rho_band = metric._band_count(self.W, self.H)
        self.dtype, self.e = metric._image_eotf(torch.float32)
        self.w = metric._rgb2y()
        self.batch = metric._batch_size(self.W, self.H, 2, self.B)
        self.ctx = metric._context(self.W, self.H, self.n_bands, 2, self.batch, self.rho_band)
        self.stream = C.c_void_p(torch.cuda.current_stream(metric.device).cuda_stream)
        self.pp = metric._pool_params()

    def ingest(self, lib, t, r, b0, nb):
        tp = (C.c_void_p * nb)(*[t[k].data_ptr() for k in range(b0, b0 + nb)])
        rp = (C.c_void_p * nb)(*[r[k].data_ptr() for k in range(b0, b0 + nb)])
        nat.check(lib.fvvdp_images_channels(self.ctx.handle, tp, rp, nb, self.dtype, self.C, self.H * self.W, C.byref(self.e),
                                            nat.fptr(self.w), 0, None, self.stream))
        return tp


def _forward(metric, t, r, fix):
    """JOD [B] and Q_per_ch [n_bands, 2, B] on the device: the launches of predict_images, no flags read back, no heat maps."""
    s = _Setup(metric, t)
    B, dev = s.B, metric.device
    Q = torch.zeros((s.n_bands, 2, B), dtype=torch.float32, device=dev)
    jod = torch.empty(B, dtype=torch.float32, device=dev)
    lib = nat.lib()
    for b0 in range(0, B, s.batch):
        nb = min(s.batch, B - b0)
        s.ingest(lib, t, r, b0, nb)
        fx, g, _keep = metric._fov_args(s.ctx, fix, b0, nb, s.n_bands, s.W, s.H)
        nat.check(lib.fvvdp_images_forward_pool(s.ctx.handle, nb, C.c_void_p(Q.data_ptr()), B, b0, fx, g, None, C.byref(s.pp),
                                                C.c_void_p(jod.data_ptr() + 4 * b0), s.stream))
    return jod, Q


def grad_batch_size(metric, W, H, n_bands, batch, planes):
    """Pairs or frames per backward batch: the context's batch, capped by GRAD_BYTES_BUDGET of maps + workspace at `planes`
    fp32 values per pyramid pixel (metric.grad_batch overrides the cap, e.g. to run several backward batches on a small
    stack)."""
    gb = getattr(metric, "grad_batch", None)
    if gb is not None:
        return max(1, min(int(gb), batch))
    px = sum(w * h for w, h in metric._level_sizes(W, H, n_bands))
    return max(1, min(batch, int(GRAD_BYTES_BUDGET // (px * 4 * planes))))


def _backward(metric, t, r, fix, Q, gamma):
    """gamma[k] * dJOD_k/dt_k for the contiguous device stack t [B, C, H, W]."""
    s = _Setup(metric, t)
    B, dev = s.B, metric.device
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, GRAD_PLANES)
    grad = torch.empty_like(t)
    maps_arr, _maps = metric._band_maps(gb, s.W, s.H, s.n_bands, contrast_planes=2)
    lib = nat.lib()
    nbytes = C.c_size_t()
    nat.check(lib.fvvdp_images_grad_workspace(s.W, s.H, s.n_bands, gb, C.byref(nbytes)))
    work = torch.empty((nbytes.value + 3) // 4, dtype=torch.float32, device=dev)
    q_scratch = torch.empty((s.n_bands, 2, gb), dtype=torch.float32, device=dev)
    jod_scratch = torch.empty(gb, dtype=torch.float32, device=dev)
    prm = metric.native_params()
    gamma = gamma.to(device=dev, dtype=torch.float32).contiguous()
    for b0 in range(0, B, gb):
        nb = min(gb, B - b0)
        tp = s.ingest(lib, t, r, b0, nb)
        fx, g, _keep = metric._fov_args(s.ctx, fix, b0, nb, s.n_bands, s.W, s.H)
        nat.check(lib.fvvdp_images_forward_pool(s.ctx.handle, nb, C.c_void_p(q_scratch.data_ptr()), nb, 0, fx, g, maps_arr,
                                                C.byref(s.pp), C.c_void_p(jod_scratch.data_ptr()), s.stream))
        gp = (C.c_void_p * nb)(*[grad[k].data_ptr() for k in range(b0, b0 + nb)])
        nat.check(lib.fvvdp_images_grad(s.W, s.H, s.n_bands, nb, C.byref(prm), C.byref(s.pp), C.c_void_p(Q.data_ptr()), B, b0,
                                        C.c_void_p(gamma.data_ptr() + 4 * b0), maps_arr, tp, s.C, s.H * s.W, C.byref(s.e),
                                        nat.fptr(s.w), gp, C.c_void_p(work.data_ptr()), nbytes.value, s.stream))
    return grad


class JodImagesFunction(torch.autograd.Function):
    """test [B, C, H, W] (contiguous fp32 on the metric's device), reference (the same, constant) -> JOD [B]."""

    @staticmethod
    def forward(ctx, test, reference, metric, fix):
        with torch.cuda.device(metric.device):
            jod, Q = _forward(metric, test, reference, fix)
        ctx.metric, ctx.fix = metric, fix
        ctx.save_for_backward(test, reference, Q)
        return jod

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_jod):
        test, reference, Q = ctx.saved_tensors
        grad = None
        if ctx.needs_input_grad[0]:
            with torch.cuda.device(ctx.metric.device):
                grad = _backward(ctx.metric, test, reference, ctx.fix, Q, grad_jod)
        return grad, None, None, None


def refuse_unsupported(name, metric, reference):
    """What jod_images and jod_video (`name`) refuse before they look at the shapes."""
    if isinstance(reference, torch.Tensor) and reference.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("%s: gradients with respect to the reference are not supported; detach the reference" % name)
    if native_eotf(metric.display_photometry) is None:
        raise RuntimeError("%s needs a display model with a closed form for float input (sRGB, gamma, PQ, linear or "
                           "absolute); a user photometry class has none" % name)


def need_float32(name, what, t, r):
    if t.dtype != torch.float32 or r.dtype != torch.float32:
        raise RuntimeError("%s needs float32 test and reference %s (got %s and %s)" % (name, what, t.dtype, r.dtype))


def place(metric, t, r):
    """Test and reference contiguous on the metric's device, the reference detached.  The layout change and the move to the
    device stay visible to autograd: the gradient reaches the caller's own tensor."""
    metric._check_device()
    return t.to(metric.device).contiguous(), r.detach().to(metric.device).contiguous()


def jod_images(metric, test, reference, dim_order="BCHW", fixation_point=None):
    """fvvdp.jod_images (see there)."""
    refuse_unsupported("jod_images", metric, reference)
    t, r = _image_stack(test, reference, dim_order)
    need_float32("jod_images", "images", t, r)
    t, r = place(metric, t, r)
    fix = None
    if metric.foveated:
        fix = metric._fixation(fixation_point, t.shape[3], t.shape[2], t.shape[0])
    return JodImagesFunction.apply(t, r, metric, fix)
