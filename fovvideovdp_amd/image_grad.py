"""Differentiable still-image JOD: fvvdp.jod_images and its autograd function (include/fvvdp_hip_grad.h).

The forward runs the launches of fvvdp.predict_images (fvvdp_images_channels + fvvdp_images_forward_pool), so the JODs are
bit-identical to it.  The backward re-runs them per backward batch with every band's maps written (band contrast, L_bkg, S,
D), then fvvdp_images_grad turns the maps and the forward's Q_per_ch into dJOD/dtest on the device.  Neither pass reads
context scratch left by the other, and neither synchronises with the host."""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .display_model import native_eotf, native_geometry

# device memory one backward batch may hold in maps and workspace (the pyramid scratch of the context comes on top)
GRAD_BYTES_BUDGET = 4e9


def _sizes(width, height, n_bands):
    out = [(width, height)]
    for _ in range(n_bands):
        w, h = out[-1]
        out.append(((w + 1) // 2, (h + 1) // 2))
    return out


def _fov_args(metric, ctx, fix, b0, nb, n_bands, width, height):
    """(fixation pointer, geometry pointer) of a foveated batch, as fvvdp._predict_image_group passes them."""
    if not metric.foveated:
        return None, None, None
    fxa = np.ascontiguousarray(fix[b0:b0 + nb], dtype=np.float32)
    g = None
    if native_geometry(metric.display_geometry) is not None:
        g = C.byref(metric._geom_struct())
    else:
        metric._set_view_maps(ctx, n_bands, width, height)
        fxa = metric._gaze_view_dirs(fxa, width, height)
    return nat.fptr(fxa), g, fxa


class _Setup:
    """What forward and backward share for one [B, C, H, W] stack: pyramid size, display model, context, launch constants."""

    def __init__(self, metric, t):
        from .fvvdp import band_frequencies
        self.B, self.C, self.H, self.W = t.shape
        self.n_bands, self.rho_band = band_frequencies(self.W, self.H, metric.pix_per_deg)
        if self.n_bands < 1:
            raise RuntimeError("Frame %dx%d is too small for this display (no band-pass level)" % (self.W, self.H))
        self.dtype, self.e = metric._image_eotf(torch.float32)
        self.w = metric._rgb2y()
        self.batch = metric._batch_size(self.W, self.H, 2, self.B)
        self.ctx = metric._context(self.W, self.H, self.n_bands, 2, self.batch, self.rho_band)
        self.stream = C.c_void_p(torch.cuda.current_stream(metric.device).cuda_stream)
        self.pp = nat.PoolParams(metric.beta_sch, metric.beta_tch, metric.beta_t, metric.w_transient, metric.jod_a,
                                 float(10.0 ** metric.log_jod_exp))

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
        fx, g, _keep = _fov_args(metric, s.ctx, fix, b0, nb, s.n_bands, s.W, s.H)
        nat.check(lib.fvvdp_images_forward_pool(s.ctx.handle, nb, C.c_void_p(Q.data_ptr()), B, b0, fx, g, None, C.byref(s.pp),
                                                C.c_void_p(jod.data_ptr() + 4 * b0), s.stream))
    return jod, Q


def grad_batch_size(metric, W, H, n_bands, batch):
    """Pairs per backward batch: the context's batch, capped by GRAD_BYTES_BUDGET of maps + workspace (metric.grad_batch
    overrides the cap, e.g. to run several backward batches on a small stack)."""
    gb = getattr(metric, "grad_batch", None)
    if gb is not None:
        return max(1, min(int(gb), batch))
    px = sum(w * h for w, h in _sizes(W, H, n_bands))
    per_pair = px * 4 * (7 + 2)           # maps: D 2 + contrast 2 + L_bkg 1 + S 2 planes; workspace: layer + sweep gradients
    return max(1, min(batch, int(GRAD_BYTES_BUDGET // per_pair)))


def _backward(metric, t, r, fix, Q, gamma):
    """gamma[k] * dJOD_k/dt_k for the contiguous device stack t [B, C, H, W]."""
    s = _Setup(metric, t)
    B, dev = s.B, metric.device
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch)
    grad = torch.empty_like(t)
    sizes = _sizes(s.W, s.H, s.n_bands)
    maps_arr = (nat.BandMaps * s.n_bands)()
    keep = []
    for b in range(s.n_bands):
        w, h = sizes[b]
        D = torch.empty((gb, 2, h, w), dtype=torch.float32, device=dev)
        Cn = torch.empty((gb, 2, h, w), dtype=torch.float32, device=dev)
        L = torch.empty((gb, h, w), dtype=torch.float32, device=dev)
        S = torch.empty((gb, 2, h, w), dtype=torch.float32, device=dev)
        keep += [D, Cn, L, S]
        maps_arr[b].d_D, maps_arr[b].d_contrast, maps_arr[b].d_lbkg, maps_arr[b].d_S = (
            D.data_ptr(), Cn.data_ptr(), L.data_ptr(), S.data_ptr())
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
        fx, g, _keep = _fov_args(metric, s.ctx, fix, b0, nb, s.n_bands, s.W, s.H)
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


def jod_images(metric, test, reference, dim_order="BCHW", fixation_point=None):
    """fvvdp.jod_images (see there)."""
    from .fvvdp import _image_stack
    if isinstance(reference, torch.Tensor) and reference.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("jod_images: gradients with respect to the reference are not supported; detach the reference")
    if native_eotf(metric.display_photometry) is None:
        raise RuntimeError("jod_images needs a display model with a closed form for float input (sRGB, gamma, PQ, linear or "
                           "absolute); a user photometry class has none")
    t, r = _image_stack(test, reference, dim_order)
    if t.dtype != torch.float32 or r.dtype != torch.float32:
        raise RuntimeError("jod_images needs float32 test and reference images (got %s and %s)" % (t.dtype, r.dtype))
    metric._check_device()
    # the layout change and the move to the device stay visible to autograd: the gradient reaches the caller's own tensor
    t = t.to(metric.device).contiguous()
    r = r.detach().to(metric.device).contiguous()
    fix = None
    if metric.foveated:
        fix = metric._fixation(fixation_point, t.shape[3], t.shape[2], t.shape[0])
    return JodImagesFunction.apply(t, r, metric, fix)
