"""Differentiable still-image JOD: fvvdp.jod_images and its autograd function (include/fvvdp_hip_grad.h, and
include/fvvdp_hip_ref_grad.h for the gradient with respect to the reference, `wrt=`).

The forward makes the launches of fvvdp.predict_images (fvvdp_images_channels + fvvdp_images_forward_pool) with arguments from
the same methods of the metric, so the JODs are bit-identical to it.  The backward re-runs them per backward batch with every
band's maps written (band contrast, L_bkg, S, D), then fvvdp_images_grad turns the maps and the forward's Q_per_ch into
dJOD/dtest on the device; with wrt="reference" / "both" the same maps plus the slope planes of the CSF look-up go to
fvvdp_images_ref_grad for dJOD/dreference -- one ingest and one pyramid pass whatever `wrt`.  Neither pass reads context scratch left by the other, and neither synchronises with the host."""
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
WRT = ("test", "reference", "both")


def check_wrt(wrt):
    if wrt not in WRT:
        raise ValueError('wrt must be "test", "reference" or "both", got %r' % (wrt,))
    return wrt


def grad_planes(wrt, planes_test=GRAD_PLANES, maps=7, per_plane=1):
    """fp32 values per pyramid pixel and batch entry that the backward with respect to `wrt` holds in maps and workspace: the
    reference's backward adds the slope planes (2, as S) and a workspace of GLR + GX + GG to the maps.
    planes_test: what the test side's backward holds (maps included); maps: the maps' share of it; per_plane: planes per entry
    of the reference's workspace (1: an image pair, 2: a video frame)."""
    if wrt == "test":
        return planes_test
    ref = maps + 2 + 3 * per_plane
    return ref if wrt == "reference" else ref + (planes_test - maps)


def slope_planes(metric, n, width, height, n_bands):
    """The slope planes kappa [n][2][h_b][w_b] of every band (fvvdp_ctx_set_slope_maps) and the pointer array both entry points
    take; the caller keeps the tensors alive."""
    keep = [torch.empty((n, 2, h, w), dtype=torch.float32, device=metric.device)
            for w, h in metric._level_sizes(width, height, n_bands)[:n_bands]]
    return (C.c_void_p * n_bands)(*[k.data_ptr() for k in keep]), keep


class _Setup:
    """What forward and backward share for one [B, C, H, W] stack: pyramid size, display model, context, launch constants."""

    def __init__(self, metric, t):
        self.B, self.C, self.H, self.W = t.shape
        self.n_bands, self.rho_band = metric._band_count(self.W, self.H)
        self.dtype, self.e = metric._image_eotf(t.dtype)          # float32, float16 or bfloat16 (float_pair)
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


def _backward(metric, t, r, fix, Q, gamma, need_t=True, need_r=False):
    """(gamma[k] * dJOD_k/dt_k, gamma[k] * dJOD_k/dr_k) for the contiguous device stacks t, r [B, C, H, W]; None for the one
    not asked for.  The ingest and the map-writing pyramid pass run once per backward batch, whichever gradients follow."""
    s = _Setup(metric, t)
    B, dev = s.B, metric.device
    wrt = "both" if need_t and need_r else ("reference" if need_r else "test")
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, grad_planes(wrt))
    grad_t = torch.empty_like(t) if need_t else None
    grad_r = torch.empty_like(r) if need_r else None
    maps_arr, _maps = metric._band_maps(gb, s.W, s.H, s.n_bands, contrast_planes=2)
    lib = nat.lib()
    nbytes, rbytes = C.c_size_t(), C.c_size_t()
    if need_t:
        nat.check(lib.fvvdp_images_grad_workspace(s.W, s.H, s.n_bands, gb, C.byref(nbytes)))
        work = torch.empty((nbytes.value + 3) // 4, dtype=torch.float32, device=dev)
    if need_r:
        nat.check(lib.fvvdp_ref_grad_workspace(s.W, s.H, s.n_bands, gb, 1, C.byref(rbytes)))
        rwork = torch.empty((rbytes.value + 3) // 4, dtype=torch.float32, device=dev)
        slopes, _slopes = slope_planes(metric, gb, s.W, s.H, s.n_bands)
    q_scratch = torch.empty((s.n_bands, 2, gb), dtype=torch.float32, device=dev)
    jod_scratch = torch.empty(gb, dtype=torch.float32, device=dev)
    prm = metric.native_params()
    gamma = gamma.to(device=dev, dtype=torch.float32).contiguous()
    for b0 in range(0, B, gb):
        nb = min(gb, B - b0)
        tp = s.ingest(lib, t, r, b0, nb)
        fx, g, _keep = metric._fov_args(s.ctx, fix, b0, nb, s.n_bands, s.W, s.H)
        if need_r:
            nat.check(lib.fvvdp_ctx_set_slope_maps(s.ctx.handle, slopes))
        try:
            nat.check(lib.fvvdp_images_forward_pool(s.ctx.handle, nb, C.c_void_p(q_scratch.data_ptr()), nb, 0, fx, g, maps_arr,
                                                    C.byref(s.pp), C.c_void_p(jod_scratch.data_ptr()), s.stream))
        finally:
            if need_r:
                nat.check(lib.fvvdp_ctx_set_slope_maps(s.ctx.handle, None))
        if need_t:
            gp = (C.c_void_p * nb)(*[grad_t[k].data_ptr() for k in range(b0, b0 + nb)])
            nat.check(lib.fvvdp_images_grad_st(s.W, s.H, s.n_bands, nb, C.byref(prm), C.byref(s.pp), C.c_void_p(Q.data_ptr()), B, b0,
                                               C.c_void_p(gamma.data_ptr() + 4 * b0), maps_arr, tp, s.dtype, s.C, s.H * s.W,
                                               C.byref(s.e), nat.fptr(s.w), gp, C.c_void_p(work.data_ptr()), nbytes.value,
                                               s.stream))
        if need_r:
            rp = (C.c_void_p * nb)(*[r[k].data_ptr() for k in range(b0, b0 + nb)])
            gp = (C.c_void_p * nb)(*[grad_r[k].data_ptr() for k in range(b0, b0 + nb)])
            nat.check(lib.fvvdp_images_ref_grad_st(s.W, s.H, s.n_bands, nb, C.byref(prm), C.byref(s.pp), C.c_void_p(Q.data_ptr()),
                                                   B, b0, C.c_void_p(gamma.data_ptr() + 4 * b0), maps_arr, slopes, rp, s.dtype,
                                                   s.C, s.H * s.W, C.byref(s.e), nat.fptr(s.w), gp,
                                                   C.c_void_p(rwork.data_ptr()), rbytes.value, s.stream))
    return grad_t, grad_r


class JodImagesFunction(torch.autograd.Function):
    """test, reference [B, C, H, W] (contiguous, of one dtype -- float32, float16 or bfloat16 -- on the metric's device) -> JOD [B]
    (fp32).  The tensors saved for backward are the inputs as they came, and each gradient has its input's dtype.  place() detaches the input that
    `wrt` treats as a constant, so needs_input_grad names the gradients to make."""

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
        grad_t = grad_r = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            with torch.cuda.device(ctx.metric.device):
                grad_t, grad_r = _backward(ctx.metric, test, reference, ctx.fix, Q, grad_jod, ctx.needs_input_grad[0],
                                           ctx.needs_input_grad[1])
        return grad_t, grad_r, None, None


def refuse_unsupported(name, metric, test, reference, wrt="test"):
    """What jod_images, jod_video and jod_gazes (`name`) refuse before they look at the shapes.  wrt None: `name` has no wrt=."""
    grad_on = torch.is_grad_enabled()
    if wrt in ("test", None) and isinstance(reference, torch.Tensor) and reference.requires_grad and grad_on:
        hint = (' (wrt= exists on jod_images and jod_video only)' if wrt is None else
                ', or ask for its gradient with wrt="reference" or wrt="both"')
        raise RuntimeError("%s: gradients with respect to the reference are not supported; detach the reference%s" % (name, hint))
    if wrt == "reference" and isinstance(test, torch.Tensor) and test.requires_grad and grad_on:
        raise RuntimeError('%s: wrt="reference" treats the test as a constant and this one requires grad; detach it, or ask '
                           'for both gradients with wrt="both"' % name)
    if native_eotf(metric.display_photometry) is None:
        raise RuntimeError("%s needs a display model with a closed form for float input (sRGB, gamma, PQ, linear or "
                           "absolute); a user photometry class has none" % name)


FLOAT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def float_pair(name, what, t, r):
    """Test and reference of jod_images / jod_video / jod_gazes (`name`) with one dtype the kernels read: float32, float16 or
    bfloat16.  A pair of two equal dtypes passes as it is: the half-precision kernels ingest it, and the gradient is written in
    that dtype.  A mixed pair (say a float16 test from a network under autocast with a float32 reference from a dataset): the
    narrower side is upcast with torch's .float(), inside autograd's view -- the float32 kernels run and the gradient reaches the
    caller's tensor in its own dtype through torch's cast node."""
    if t.dtype not in FLOAT_DTYPES or r.dtype not in FLOAT_DTYPES:
        raise RuntimeError("%s needs float32, float16 or bfloat16 test and reference %s (got %s and %s)"
                           % (name, what, t.dtype, r.dtype))
    if t.dtype != r.dtype:
        t, r = t.float(), r.float()
    return t, r


def place(metric, t, r, wrt="test"):
    """Test and reference contiguous on the metric's device, the one `wrt` treats as a constant detached.  The layout change
    and the move to the device stay visible to autograd: the gradient reaches the caller's own tensor."""
    metric._check_device()
    if wrt == "test":
        r = r.detach()
    elif wrt == "reference":
        t = t.detach()
    return t.to(metric.device).contiguous(), r.to(metric.device).contiguous()


def jod_images(metric, test, reference, dim_order="BCHW", fixation_point=None, wrt="test"):
    """fvvdp.jod_images (see there)."""
    check_wrt(wrt)
    refuse_unsupported("jod_images", metric, test, reference, wrt)
    t, r = _image_stack(test, reference, dim_order)
    t, r = float_pair("jod_images", "images", t, r)
    t, r = place(metric, t, r, wrt)
    fix = None
    if metric.foveated:
        fix = metric._fixation(fixation_point, t.shape[3], t.shape[2], t.shape[0])
    return JodImagesFunction.apply(t, r, metric, fix)
