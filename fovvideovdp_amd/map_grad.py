"""Differentiable difference maps: fvvdp.diff_map_images / diff_map_video and their autograd functions
(include/fvvdp_hip_diffmap.h).

The forward makes the launches of predict_images / predict on a metric built with heatmap="raw" -- the ingest, the pyramid pass
with the difference maps D written, fvvdp_heatmap_reconstruct -- with arguments from the same methods of the metric, so the map
rounded to float16 is that heat map bit for bit; it stays on the device in fp32 and nothing is copied to the host.  The backward
re-runs the ingest and the map-writing pass per backward batch (every band's maps: D, contrast, L_bkg, S), reconstructs v_0
without the final power (units "jod"), and fvvdp_diffmap_images_grad / fvvdp_diffmap_video_grad_frames turn the cotangent of the
map into the gradient of the test images / of level 0's two test planes; for a clip one fvvdp_video_grad_input_st then applies
the transpose of the temporal filter and the display model's derivative.  The setup, the map-writing pass and the clip's buffers
are grad_passes.py's, the argument handling image_grad's and video_grad's."""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .fvvdp import _image_stack
from .grad_passes import ClipBuffers, ClipSetup, ImageSetup, Maps, _ptr, batches, grad_batch_size, work_tensor, workspace_bytes
from .image_grad import GRAD_PLANES as IMAGE_PLANES, float_pair, place, refuse_unsupported
from .video_grad import GRAD_PLANES as VIDEO_PLANES, clip_arguments

UNITS = {"jod": nat.DIFFMAP_JOD, "linear": nat.DIFFMAP_LINEAR}
# fp32 planes per pyramid pixel and batch entry: what the JOD's backward holds (maps and workspace) plus the A chain (one value
# per pyramid pixel) and v_0 (one per level-0 pixel, 3/4 of a pyramid pixel: counted as one)
MAP_IMAGE_PLANES = IMAGE_PLANES + 2
MAP_VIDEO_PLANES = VIDEO_PLANES + 2
# device memory the D maps of one forward batch may hold: the cap predict_images / predict put on a heat-map batch
FORWARD_BYTES_BUDGET = 2e9


def check_units(units):
    if units not in UNITS:
        raise ValueError('units must be "jod" or "linear", got %r' % (units,))
    return units


def _refuse(name, metric, test, reference):
    """What diff_map_images / diff_map_video (`name`) refuse before they look at the shapes: a reference that requires grad, a
    user photometry class."""
    if isinstance(reference, torch.Tensor) and reference.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("%s differentiates the map with respect to the test only and this reference requires grad; detach "
                           "the reference (there is no wrt= here)" % name)
    refuse_unsupported(name, metric, test, reference, None)


class _DMaps:
    """The difference maps D of every band for forward batches of up to n pairs or frames, and the scratch the pass pools into
    (what ImageSetup.launch / ClipSetup.launch take as `maps`)."""

    def __init__(self, metric, W, H, n_bands, n):
        self.maps_arr, self._keep = metric._band_maps(n, W, H, n_bands)
        self.slopes = None
        self.q_scratch = torch.empty((n_bands, 2, n), dtype=torch.float32, device=metric.device)
        self.jod_scratch = torch.empty(n, dtype=torch.float32, device=metric.device)
        self.d_ptrs = (C.c_void_p * n_bands)(*[d.data_ptr() for d in self._keep])


def _d_ptrs(maps, n_bands):
    """The D maps of a grad_passes.Maps (D, contrast, L_bkg, S per band) as fvvdp_heatmap_reconstruct takes them."""
    return (C.c_void_p * n_bands)(*[maps.maps_arr[b].d_D for b in range(n_bands)])


def _reconstruct(s, d_ptrs, nb, out, units):
    """D maps of nb entries -> out [nb, H, W]: the map in `units` (the arguments of fvvdp._heatmap_batch for "jod")."""
    m = s.metric
    if units == "jod":
        beta_jod = float(np.power(10.0, m.log_jod_exp))
        nat.check(nat.lib().fvvdp_heatmap_reconstruct(s.ctx.handle, nb, d_ptrs, float(m.w_transient), beta_jod, abs(float(m.jod_a)),
                                                      _ptr(out), s.stream))
    else:
        nat.check(nat.lib().fvvdp_heatmap_reconstruct_linear(s.ctx.handle, nb, d_ptrs, float(m.w_transient), _ptr(out), s.stream))


def _forward_batch(s, total):
    """Pairs or frames per forward batch: the context's batch under predict's cap for a batch with heat maps."""
    return max(1, min(s.batch, total, int(FORWARD_BYTES_BUDGET // (s.W * s.H * 4 * 12))))


# ---- still images ---------------------------------------------------------------------------------------------------------
def _forward_images(metric, t, r, fix, units):
    """The map [B, H, W] of the contiguous device stacks t, r [B, C, H, W]."""
    s = ImageSetup(metric, t, r)
    out = torch.empty((s.B, s.H, s.W), dtype=torch.float32, device=metric.device)
    fb = _forward_batch(s, s.B)
    dm = _DMaps(metric, s.W, s.H, s.n_bands, fb)
    for b0, nb in batches(s.B, fb):
        s.write_maps(dm, fix, b0, nb)
        _reconstruct(s, dm.d_ptrs, nb, out[b0:b0 + nb], units)
    return out


def _backward_images(metric, t, r, fix, G, units):
    """sum_px G[k] dmap_k/dt_k for the contiguous device stacks t, r [B, C, H, W] and the cotangent G [B, H, W]."""
    s = ImageSetup(metric, t, r)
    lib = nat.lib()
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, MAP_IMAGE_PLANES)
    grad = torch.empty_like(t)
    maps = Maps(metric, s.W, s.H, s.n_bands, 2, gb)
    d_ptrs = _d_ptrs(maps, s.n_bands)
    nbytes = workspace_bytes(lib.fvvdp_diffmap_grad_workspace, s.W, s.H, s.n_bands, gb, 1, None, None)
    work = work_tensor(nbytes)
    v0 = torch.empty((gb, s.H, s.W), dtype=torch.float32, device=metric.device) if units == "jod" else None
    prm = s.params()
    for b0, nb in batches(s.B, gb):
        tp = s.write_maps(maps, fix, b0, nb)
        if v0 is not None:
            _reconstruct(s, d_ptrs, nb, v0, "linear")
        gp = (C.c_void_p * nb)(*[grad[k].data_ptr() for k in range(b0, b0 + nb)])
        nat.check(lib.fvvdp_diffmap_images_grad(s.W, s.H, s.n_bands, nb, C.byref(prm), C.byref(s.pp), UNITS[units],
                                                _ptr(G, 4 * b0 * s.H * s.W), None if v0 is None else _ptr(v0), maps.maps_arr, tp,
                                                s.dtype, s.C, s.H * s.W, C.byref(s.e), nat.fptr(s.w), gp, _ptr(work), nbytes,
                                                s.stream))
    return grad


class DiffMapImagesFunction(torch.autograd.Function):
    """test, reference [B, C, H, W] (contiguous, of one dtype -- float32, float16 or bfloat16 -- on the metric's device) -> the
    map [B, H, W] (fp32).  The tensors saved for backward are the inputs as they came; the gradient has the test's dtype."""

    @staticmethod
    def forward(ctx, test, reference, metric, fix, units):
        with torch.cuda.device(metric.device):
            out = _forward_images(metric, test, reference, fix, units)
        ctx.metric, ctx.fix, ctx.units = metric, fix, units
        ctx.save_for_backward(test, reference)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_map):
        test, reference = ctx.saved_tensors
        grad = None
        if ctx.needs_input_grad[0]:
            m = ctx.metric
            G = grad_map.to(device=m.device, dtype=torch.float32).contiguous()
            with torch.cuda.device(m.device):
                grad = _backward_images(m, test, reference, ctx.fix, G, ctx.units)
        return grad, None, None, None, None


def diff_map_images(metric, test, reference, dim_order="BCHW", fixation_point=None, units="jod"):
    """fvvdp.diff_map_images (see there)."""
    check_units(units)
    _refuse("diff_map_images", metric, test, reference)
    t, r = _image_stack(test, reference, dim_order)
    t, r = float_pair("diff_map_images", "images", t, r)
    t, r = place(metric, t, r)
    fix = None
    if metric.foveated:
        fix = metric._fixation(fixation_point, t.shape[3], t.shape[2], t.shape[0])
    return DiffMapImagesFunction.apply(t, r, metric, fix, units)


# ---- clips ------------------------------------------------------------------------------------------------------------------
def _forward_video(metric, t, r, fps, fix, units):
    """The map [N, H, W] of the contiguous device clips t, r [1, C, N, H, W]."""
    s = ClipSetup(metric, t, fps, r)
    out = torch.empty((s.N, s.H, s.W), dtype=torch.float32, device=metric.device)
    oob = torch.zeros(1, dtype=torch.int32, device=metric.device)
    fb = _forward_batch(s, s.N)
    dm = _DMaps(metric, s.W, s.H, s.n_bands, fb)
    for b0, nb in batches(s.N, fb):
        s.write_maps(dm, fix, b0, nb, oob)
        _reconstruct(s, dm.d_ptrs, nb, out[b0:b0 + nb], units)
    return out


def _backward_video(metric, t, r, fps, fix, G, units):
    """sum_px G dmap/dt for the contiguous device clips t, r [1, C, N, H, W] and the cotangent G [N, H, W]; batched and checked
    against the free device memory as jod_video's backward (grad_passes.ClipBuffers)."""
    s = ClipSetup(metric, t, fps, r)
    lib = nat.lib()
    HW = s.H * s.W
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, MAP_VIDEO_PLANES)
    nbytes = workspace_bytes(lib.fvvdp_diffmap_grad_workspace, s.W, s.H, s.n_bands, gb, 2, None, None)
    v0_bytes = gb * HW * 4 if units == "jod" else 0
    buf = ClipBuffers("diff_map_video", metric, s, t, gb, nbytes, extra_bytes=v0_bytes)
    d_ptrs = _d_ptrs(buf.maps, s.n_bands)
    v0 = torch.empty((gb, s.H, s.W), dtype=torch.float32, device=metric.device) if units == "jod" else None
    prm = s.params()
    for b0, nb in batches(s.N, gb):
        buf.maps_pass(lib, metric, s, t, r, fix, b0, nb)
        if v0 is not None:
            _reconstruct(s, d_ptrs, nb, v0, "linear")
        nat.check(lib.fvvdp_diffmap_video_grad_frames(s.W, s.H, s.n_bands, nb, C.byref(prm), C.byref(s.pp), UNITS[units],
                                                      _ptr(G, 4 * b0 * HW), None if v0 is None else _ptr(v0), s.N, b0,
                                                      buf.maps.maps_arr, _ptr(buf.g0), _ptr(buf.work), nbytes, s.stream))
    return buf.input_grad(lib, s, t)


class DiffMapVideoFunction(torch.autograd.Function):
    """test, reference [1, C, N, H, W] (contiguous, of one dtype -- float32, float16 or bfloat16 -- on the metric's device) -> the
    map [N, H, W] (fp32).  The tensors saved for backward are the clips as they came; the gradient has the test's dtype."""

    @staticmethod
    def forward(ctx, test, reference, metric, fps, fix, units):
        with torch.cuda.device(metric.device):
            out = _forward_video(metric, test, reference, fps, fix, units)
        ctx.metric, ctx.fps, ctx.fix, ctx.units = metric, fps, fix, units
        ctx.save_for_backward(test, reference)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_map):
        test, reference = ctx.saved_tensors
        grad = None
        if ctx.needs_input_grad[0]:
            m = ctx.metric
            G = grad_map.to(device=m.device, dtype=torch.float32).contiguous()
            with torch.cuda.device(m.device):
                grad = _backward_video(m, test, reference, ctx.fps, ctx.fix, G, ctx.units)
        return grad, None, None, None, None, None


def diff_map_video(metric, test, reference, dim_order="BCFHW", frames_per_second=0, fixation_point=None, units="jod"):
    """fvvdp.diff_map_video (see there)."""
    check_units(units)
    _refuse("diff_map_video", metric, test, reference)
    t, r = clip_arguments("diff_map_video", metric, test, reference, dim_order, frames_per_second)
    t, r = place(metric, t, r)
    fix = None
    if metric.foveated:
        fix = metric._fixation(fixation_point, t.shape[4], t.shape[3], t.shape[2])
    return DiffMapVideoFunction.apply(t, r, metric, float(frames_per_second), fix, units)
