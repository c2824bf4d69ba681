"""Differentiable video JOD: fvvdp.jod_video and its autograd function (include/fvvdp_hip_video_grad.h).

The forward makes the launches of fvvdp.predict for a device-resident float clip (fvvdp_temporal_channels per frame batch,
fvvdp_bands_forward, the pooling of fvvdp_bands_forward_pool on the last batch) with arguments from the same methods of the
metric, so the JOD is bit-identical to it.  The backward re-runs them per backward batch with every band's maps written,
fvvdp_video_grad_frames turns the maps and the forward's Q_per_ch into the gradient of level 0's two test planes (a clip-long
buffer), and one fvvdp_video_grad_input applies the transpose of the sliding-window temporal filter and the display model's
derivative.  With wrt="reference" / "both" the same maps plus the slope planes of the CSF look-up go to
fvvdp_video_ref_grad_frames (include/fvvdp_hip_ref_grad.h) and a second fvvdp_video_grad_input runs on the reference clip: one
ingest and one pyramid pass per backward batch whatever `wrt`.  Neither pass reads context scratch left by the other, and neither synchronises with the host.
The setup, the forward loop, the buffers with their map-writing pass and the level-0 backward are grad_passes.py's, shared with
the other differentiable entry points; what is here is the argument handling (also gaze_grad's and display_grad's), the
backward's loop and the autograd function."""
import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .fvvdp import filter_length                            # (imported from here by tools)
from .grad_passes import (ClipBuffers as _Buffers, ClipSetup as _Setup, _fold_arrays, backward_bytes, batches,   # noqa: F401
                          fold_list, forward_clip, grad_batch_size, level0_backward, level0_buffers)
from .image_grad import check_wrt, float_pair, grad_planes, place, refuse_unsupported
from .video_source import fvvdp_video_source_array, reshuffle_dims

# fp32 planes per pyramid pixel and frame: maps (D 2 + contrast 4 + L_bkg 1 + S 2) and workspace (layer + sweep gradients of
# both channels)
GRAD_PLANES = 9 + 4


def video_grad_planes(wrt):
    """fp32 values per pyramid pixel and frame of a backward batch, per `wrt` (image_grad.grad_planes): 13, 17, 21."""
    return grad_planes(wrt, GRAD_PLANES, 9, 2)


def _forward(metric, t, r, fps, fix):
    """JOD (0-d) and Q_per_ch [n_bands, 2, N] on the device (grad_passes.forward_clip)."""
    return forward_clip(_Setup(metric, t, fps, r), fix)


def _backward(metric, t, r, fps, fix, Q, gamma, need_t=True, need_r=False):
    """(gamma * dJOD/dt, gamma * dJOD/dr) for the contiguous device clips t, r [1, C, N, H, W]; None for the one not asked for.
    The ingest and the map-writing pyramid pass run once per backward batch, whichever gradients follow."""
    s = _Setup(metric, t, fps, r)
    wrt = "both" if need_t and need_r else ("reference" if need_r else "test")
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, video_grad_planes(wrt))
    buf = level0_buffers("jod_video", metric, s, t, gb, need_t, need_r)
    prm = s.params()
    gamma = gamma.to(device=metric.device, dtype=torch.float32).reshape(1).contiguous()
    lib = nat.lib()
    for b0, nb in batches(s.N, gb):
        buf.maps_pass(lib, metric, s, t, r, fix, b0, nb)
        level0_backward(buf, s, prm, Q, s.N, b0, nb, gamma, need_t, need_r)
    grad_t = buf.input_grad(lib, s, t) if need_t else None
    grad_r = buf.input_grad(lib, s, r, buf.g0_r, buf.grad_r) if need_r else None
    return grad_t, grad_r


class JodVideoFunction(torch.autograd.Function):
    """test, reference [1, C, N, H, W] (contiguous, of one dtype -- float32, float16 or bfloat16 -- on the metric's device) -> JOD
    (0-d, fp32).  The tensors saved for backward are the clips as they came, and each gradient has its clip's dtype.  place() detaches the input that
    `wrt` treats as a constant, so needs_input_grad names the gradients to make."""

    @staticmethod
    def forward(ctx, test, reference, metric, fps, fix):
        with torch.cuda.device(metric.device):
            jod, Q = _forward(metric, test, reference, fps, fix)
        ctx.metric, ctx.fps, ctx.fix = metric, fps, fix
        ctx.save_for_backward(test, reference, Q)
        return jod.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_jod):
        test, reference, Q = ctx.saved_tensors
        grad_t = grad_r = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            with torch.cuda.device(ctx.metric.device):
                grad_t, grad_r = _backward(ctx.metric, test, reference, ctx.fps, ctx.fix, Q, grad_jod, ctx.needs_input_grad[0],
                                           ctx.needs_input_grad[1])
        return grad_t, grad_r, None, None, None


def clip_arguments(name, metric, test, reference, dim_order, frames_per_second, wrt=None):
    """What jod_video and jod_gazes (`name`) accept: one float32 / float16 / bfloat16 clip pair (float_pair) of at least 2 frames, C = 1 or 3, a closed-form display
    model, a temporal filter of at most VIDEO_GRAD_MAX_TAPS taps.  Returns test and reference as [1, C, N, H, W] tensors, not yet
    placed on the device.  wrt: which input the gradient is taken for (None: `name` has no wrt=, the test)."""
    refuse_unsupported(name, metric, test, reference, wrt)
    if tuple(test.shape) != tuple(reference.shape):
        raise RuntimeError('Test and reference image/video tensors must be exactly the same shape')
    d = dim_order.upper()
    if len(d) != len(test.shape):
        raise RuntimeError('Input tensor much have exactly as many dimensions as there are characters in the "dims" parameter')
    if len(set(d)) != len(d) or set(d) - set("BCFHW") or "H" not in d or "W" not in d:
        raise RuntimeError('dim_order must be made of distinct letters of "BCFHW" and contain H and W, got "%s"' % dim_order)
    t = fvvdp_video_source_array._as_tensor(test)
    r = fvvdp_video_source_array._as_tensor(reference)
    if "F" not in d or t.shape[d.index("F")] < 2:
        raise RuntimeError("%s needs a clip: an F axis of at least 2 frames in dim_order (a single frame is a still "
                           "image: use jod_images)" % name)
    if "B" in d and t.shape[d.index("B")] != 1:
        raise RuntimeError("%s takes one clip per call (B must be 1)" % name)
    t, r = float_pair(name, "clips", t, r)
    if not frames_per_second > 0:
        raise RuntimeError("When passing video sequences, you must set frames_per_second parameter")
    fl = filter_length(frames_per_second)
    if fl > nat.VIDEO_GRAD_MAX_TAPS:
        raise RuntimeError("%s: frame rate too high for the backward: its temporal filter has %d taps, the transpose "
                           "kernel covers %d (256 frames per second)" % (name, fl, nat.VIDEO_GRAD_MAX_TAPS))
    t, r = reshuffle_dims(t, d, "BCFHW"), reshuffle_dims(r, d, "BCFHW")
    if t.shape[1] != 1 and t.shape[1] != 3:
        raise RuntimeError('The content must have either 1 or 3 colour channels.')
    return t, r


def jod_video(metric, test, reference, dim_order="BCFHW", frames_per_second=0, fixation_point=None, wrt="test"):
    """fvvdp.jod_video (see there)."""
    check_wrt(wrt)
    t, r = clip_arguments("jod_video", metric, test, reference, dim_order, frames_per_second, wrt)
    t, r = place(metric, t, r, wrt)
    fix = None
    if metric.foveated:
        fix = metric._fixation(fixation_point, t.shape[4], t.shape[3], t.shape[2])
    return JodVideoFunction.apply(t, r, metric, float(frames_per_second), fix)
