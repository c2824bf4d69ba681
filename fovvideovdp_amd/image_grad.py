"""Differentiable still-image JOD: fvvdp.jod_images and its autograd function (include/fvvdp_hip_grad.h, and
include/fvvdp_hip_ref_grad.h for the gradient with respect to the reference, `wrt=`).

The forward makes the launches of fvvdp.predict_images (fvvdp_images_channels + fvvdp_images_forward_pool) with arguments from
the same methods of the metric, so the JODs are bit-identical to it.  The backward re-runs them per backward batch with every
band's maps written (band contrast, L_bkg, S, D), then fvvdp_images_grad turns the maps and the forward's Q_per_ch into
dJOD/dtest on the device; with wrt="reference" / "both" the same maps plus the slope planes of the CSF look-up go to
fvvdp_images_ref_grad for dJOD/dreference -- one ingest and one pyramid pass whatever `wrt`.  Neither pass reads context scratch left by the other, and neither synchronises with the host.
The setup, the forward loop and the map-writing pass are grad_passes.py's, shared with the other differentiable entry points;
what is here is the argument handling (also video_grad's and gaze_grad's), the two gradient launches and the autograd function."""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .display_model import native_eotf
from .fvvdp import _image_stack
from .grad_passes import (GRAD_BYTES_BUDGET, ImageSetup as _Setup, Maps, _ptr, batches, forward_images,      # noqa: F401
                          grad_batch_size, slope_planes, workspace)           # (some only for the tests and tools that import them here)

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


def _forward(metric, t, r, fix):
    """JOD [B] and Q_per_ch [n_bands, 2, B] on the device (grad_passes.forward_images)."""
    return forward_images(_Setup(metric, t, r), fix)


def _backward(metric, t, r, fix, Q, gamma, need_t=True, need_r=False):
    """(gamma[k] * dJOD_k/dt_k, gamma[k] * dJOD_k/dr_k) for the contiguous device stacks t, r [B, C, H, W]; None for the one
    not asked for.  The ingest and the map-writing pyramid pass run once per backward batch, whichever gradients follow."""
    s = _Setup(metric, t, r)
    B, dev = s.B, metric.device
    wrt = "both" if need_t and need_r else ("reference" if need_r else "test")
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, grad_planes(wrt))
    grad_t = torch.empty_like(t) if need_t else None
    grad_r = torch.empty_like(r) if need_r else None
    lib = nat.lib()
    maps = Maps(metric, s.W, s.H, s.n_bands, 2, gb)
    if need_t:
        nbytes, work = workspace(lib.fvvdp_images_grad_workspace, s.W, s.H, s.n_bands, gb)
    if need_r:
        rbytes, rwork = workspace(lib.fvvdp_ref_grad_workspace, s.W, s.H, s.n_bands, gb, 1)
        maps.add_slopes()
    prm = s.params()
    gamma = gamma.to(device=dev, dtype=torch.float32).contiguous()
    common = (C.byref(prm), C.byref(s.pp), _ptr(Q), B)
    for b0, nb in batches(B, gb):
        tp = s.write_maps(maps, fix, b0, nb)
        if need_t:
            gp = (C.c_void_p * nb)(*[grad_t[k].data_ptr() for k in range(b0, b0 + nb)])
            nat.check(lib.fvvdp_images_grad_st(s.W, s.H, s.n_bands, nb, *common, b0, _ptr(gamma, 4 * b0), maps.maps_arr, tp,
                                               s.dtype, s.C, s.H * s.W, C.byref(s.e), nat.fptr(s.w), gp, _ptr(work), nbytes,
                                               s.stream))
        if need_r:
            rp = (C.c_void_p * nb)(*[r[k].data_ptr() for k in range(b0, b0 + nb)])
            gp = (C.c_void_p * nb)(*[grad_r[k].data_ptr() for k in range(b0, b0 + nb)])
            nat.check(lib.fvvdp_images_ref_grad_st(s.W, s.H, s.n_bands, nb, *common, b0, _ptr(gamma, 4 * b0), maps.maps_arr,
                                                   maps.slopes, rp, s.dtype, s.C, s.H * s.W, C.byref(s.e), nat.fptr(s.w), gp,
                                                   _ptr(rwork), rbytes, s.stream))
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
