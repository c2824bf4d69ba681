"""Clips whose test and reference have frame counts of their own: fvvdp.predict_held, fvvdp.jod_video_held and the autograd
function of the latter (include/fvvdp_hip_held.h).

Each stream is shown by sample-and-hold through a frame map m_s: display frame v in [0, N) shows source frame m_s[v].  The pair is
judged at the display's rate, and

    predict_held(test, ref, ...)  ==  predict(test.index_select(frames, m_t), ref.index_select(frames, m_r), ...)

bit for bit (JOD and Q_per_ch): taps, the temporal padding and the gaze refer to display frames, and the window list each stream's
ingest reads is the display-rate list sent through its map (fvvdp_temporal_channels_held: the ring bodies of predict's ingest with
a stride pair per stream).  The backward is jod_video's per batch -- the map-writing pass and fvvdp_video_grad_frames /
fvvdp_video_ref_grad_frames into a clip-long level-0 gradient at the display's rate -- and ends, once per differentiated stream,
with fvvdp_video_grad_input_held: the temporal transpose, the transpose of the hold and the display model's derivative in one
kernel, dJOD at the stream's own frame count.  No expanded clip exists at any point.  The launch layer is grad_passes.py's
(HeldClipSetup, ClipBuffers, level0_backward)."""
import ctypes as C
import logging
import numbers

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .display_model import native_eotf
from .fvvdp import filter_length
from .grad_passes import (HeldClipSetup, _ptr, batches, grad_batch_size, held_fold_arrays, held_strides, level0_backward, level0_buffers)
from .image_grad import FLOAT_DTYPES, check_wrt, refuse_unsupported
from .video_grad import video_grad_planes
from .video_source import fvvdp_video_source, fvvdp_video_source_array, reshuffle_dims

SAMPLE_DTYPES = (torch.uint8, torch.int16, torch.float32, torch.float16, torch.bfloat16)


def frame_map(what, spec, F):
    """`spec` (test_frames= / reference_frames=) for a stream of F source frames -> the frame map, int32 [N].  An int k >= 1:
    display frame v shows frame v // k (N = F k).  A 1-D integer sequence, array or tensor m: display frame v shows frame m[v];
    non-decreasing, 0 <= m[v] < F; entries may repeat (the frame is held) and may skip (the frame is never shown)."""
    if isinstance(spec, bool) or isinstance(spec, (float, np.floating)):
        raise ValueError("%s_frames must be an int k >= 1 or a 1-D integer sequence, got %r" % (what, spec))
    if isinstance(spec, numbers.Integral):
        k = int(spec)
        if k < 1:
            raise ValueError("%s_frames=%d: a frame is held for k >= 1 display frames" % (what, k))
        return (np.arange(F * k, dtype=np.int64) // k).astype(np.int32)
    m = spec.detach().cpu().numpy() if isinstance(spec, torch.Tensor) else np.asarray(spec)
    if m.dtype.kind not in "iu":
        raise ValueError("%s_frames must hold integers (frame numbers), got %s" % (what, m.dtype))
    if m.ndim != 1:
        raise ValueError("%s_frames must be an int or a 1-D sequence, got shape %s" % (what, tuple(m.shape)))
    m = m.astype(np.int64)
    if m.size and (m.min() < 0 or m.max() >= F):
        raise ValueError("%s_frames names frame %d outside the %s's [0, %d)" % (what, int(m.min() if m.min() < 0 else m.max()), what, F))
    if (np.diff(m) < 0).any():
        v = int(np.nonzero(np.diff(m) < 0)[0][0]) + 1
        raise ValueError("%s_frames must be non-decreasing (entry %d: %d after %d)" % (what, v, int(m[v]), int(m[v - 1])))
    return m.astype(np.int32)


def frame_maps(test_frames, reference_frames, F_t, F_r):
    """(m_t, m_r): both maps, of one length N >= 2."""
    m_t, m_r = frame_map("test", test_frames, F_t), frame_map("reference", reference_frames, F_r)
    if len(m_t) != len(m_r):
        raise ValueError("the test is shown for %d display frames and the reference for %d: test_frames and reference_frames "
                         "must lead to one count" % (len(m_t), len(m_r)))
    if len(m_t) < 2:
        raise ValueError("a clip needs at least 2 display frames, got %d" % len(m_t))
    return m_t, m_r


def _is_identity(m, F):
    return len(m) == F and np.array_equal(m, np.arange(F))


def _clip(name, what, x, dim_order, dtypes):
    """One stream as a [1, C, F, H, W] tensor (a view where possible)."""
    if isinstance(x, fvvdp_video_source):
        raise RuntimeError("%s takes arrays or tensors; the %s is a video source object (%s)" % (name, what, type(x).__name__))
    if not isinstance(x, (np.ndarray, torch.Tensor)):
        raise RuntimeError("%s takes arrays or tensors; the %s is %s" % (name, what, type(x).__name__))
    t = fvvdp_video_source_array._as_tensor(x)
    if t.dtype not in dtypes:
        raise RuntimeError("%s takes %s samples; the %s is %s" % (name, ", ".join(str(d).replace("torch.", "").replace("int16", "uint16") for d in dtypes),
                                                                  what, str(x.dtype).replace("torch.", "")))
    d = dim_order.upper()
    if len(d) != t.dim():
        raise RuntimeError('Input tensor much have exactly as many dimensions as there are characters in the "dims" parameter')
    if len(set(d)) != len(d) or set(d) - set("BCFHW") or "H" not in d or "W" not in d:
        raise RuntimeError('dim_order must be made of distinct letters of "BCFHW" and contain H and W, got "%s"' % dim_order)
    if "F" not in d:
        raise RuntimeError("%s needs clips: an F axis in dim_order" % name)
    if "B" in d and t.shape[d.index("B")] != 1:
        raise RuntimeError("%s takes one clip per call (B must be 1)" % name)
    t = reshuffle_dims(t, d, "BCFHW")
    if t.shape[1] != 1 and t.shape[1] != 3:
        raise RuntimeError('The content must have either 1 or 3 colour channels.')
    return t


def _arguments(name, metric, test, reference, dim_order, frames_per_second, test_frames, reference_frames, dtypes):
    """Everything that is refused before device work.  Returns (test, reference) as [1, C, F_s, H, W] views and the two maps."""
    if metric.do_heatmap:
        raise RuntimeError("%s makes no heat maps: build the metric with heatmap=None" % name)
    t = _clip(name, "test", test, dim_order, dtypes)
    r = _clip(name, "reference", reference, dim_order, dtypes)
    if t.shape[1] != r.shape[1]:
        raise RuntimeError("%s: test and reference differ in their channel counts (%d and %d)" % (name, t.shape[1], r.shape[1]))
    if tuple(t.shape[3:]) != tuple(r.shape[3:]):
        raise RuntimeError("%s: test and reference differ in their frame sizes (%dx%d and %dx%d); clips of different resolutions: "
                           "predict_resized" % (name, t.shape[4], t.shape[3], r.shape[4], r.shape[3]))
    m_t, m_r = frame_maps(test_frames, reference_frames, t.shape[2], r.shape[2])
    if not frames_per_second > 0:
        raise RuntimeError("When passing video sequences, you must set frames_per_second parameter")
    fl = filter_length(frames_per_second)
    if fl > nat.HELD_MAX_TAPS:
        raise RuntimeError("%s: display rate too high: its temporal filter has %d taps, the held-frame kernels cover %d "
                           "(128 frames per second)" % (name, fl, nat.HELD_MAX_TAPS))
    return t, r, m_t, m_r


def dense_planar(x):
    """May the kernels read the [1, C, F, H, W] view in place?  Frames of H x W contiguous samples; channel and frame strides that
    each hold a frame at least (planes of frames, BCFHW / CFHW, or frames of planes, FCHW)."""
    _, Cn, F, H, W = x.shape
    hw = H * W
    return (x.stride(4) == 1 and x.stride(3) == W and (F == 1 or x.stride(2) >= hw) and (Cn == 1 or x.stride(1) >= hw))


def _place(metric, x):
    x = x.to(metric.device)
    return x if dense_planar(x) else x.contiguous()


def _forward(s, fix):
    """grad_passes.forward_clip with the whole result buffer: (res, Q) -- res = Q_per_ch | range flag | JOD, as predict lays it
    out."""
    nq = s.n_bands * 2 * s.N
    res = torch.zeros(nq + 2, dtype=torch.float32, device=s.metric.device)
    Q = res[:nq].view(s.n_bands, 2, s.N)
    oob = res[nq:nq + 1].view(torch.int32)
    b0 = 0
    for nb in s.schedule:
        s.launch(fix, b0, nb, oob, Q, s.N, b0, _ptr(res[nq + 1:]) if b0 + nb == s.N else None)
        b0 += nb
    return res, Q


def _input_grad(lib, s, buf, head, x, m, g0):
    """A clip-long level-0 gradient at the display's rate -> the gradient of the source clip x [1, C, F, H, W] shown through m,
    laid out as x."""
    grad = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
    ff, fp = held_fold_arrays(m, s.widx, s.fl)
    i32p = C.POINTER(C.c_int32)
    nat.check(lib.fvvdp_video_grad_input_held(s.W, s.H, s.N, x.shape[2], _ptr(g0), m.ctypes.data_as(i32p), ff.ctypes.data_as(i32p),
                                              fp.ctypes.data_as(i32p), nat.fptr(s.taps), s.fl, _ptr(x), _ptr(grad), s.dtype, s.C,
                                              *held_strides(x), C.byref(s.e), nat.fptr(s.w), _ptr(head),
                                              head.numel() * 4, s.stream))
    return grad


def _backward(metric, t, r, cfg, fix, Q, gamma, need_t, need_r):
    """(gamma * dJOD/dt, gamma * dJOD/dr) for the placed clips, each at its own frame count; None for the one not asked for."""
    fps, m_t, m_r = cfg
    s = HeldClipSetup(metric, t, fps, r, m_t, m_r)
    wrt = "both" if need_t and need_r else ("reference" if need_r else "test")
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, video_grad_planes(wrt))
    HW = s.H * s.W
    head_floats = nat.held_map_bytes(s.N) // 4 + s.fl * HW
    # beside ClipBuffers' own: the results at the streams' own frame counts, and the side buffer with the map at its head
    extra = 4 * head_floats + (t.numel() * t.element_size() if need_t else 0) + (r.numel() * r.element_size() if need_r else 0)
    buf = level0_buffers("jod_video_held", metric, s, None, gb, need_t, need_r, results=False, head=False, extra_bytes=extra)
    head = torch.empty(head_floats, dtype=torch.float32, device=metric.device)
    prm = s.params()
    gamma = gamma.to(device=metric.device, dtype=torch.float32).reshape(1).contiguous()
    lib = nat.lib()
    for b0, nb in batches(s.N, gb):
        buf.maps_pass(lib, metric, s, t, r, fix, b0, nb)
        level0_backward(buf, s, prm, Q, s.N, b0, nb, gamma, need_t, need_r)
    grad_t = _input_grad(lib, s, buf, head, t, s.m_t, buf.g0) if need_t else None
    grad_r = _input_grad(lib, s, buf, head, r, s.m_r, buf.g0_r) if need_r else None
    return grad_t, grad_r


class JodVideoHeldFunction(torch.autograd.Function):
    """test [1, C, F_t, H, W], reference [1, C, F_r, H, W] (placed: _place; one dtype -- float32, float16 or bfloat16) -> JOD (0-d,
    fp32).  The tensors saved for backward are the source clips, and each gradient has its clip's shape and dtype."""

    @staticmethod
    def forward(ctx, test, reference, metric, cfg, fix):
        fps, m_t, m_r = cfg
        with torch.cuda.device(metric.device):
            res, Q = _forward(HeldClipSetup(metric, test, fps, reference, m_t, m_r), fix)
        ctx.metric, ctx.cfg, ctx.fix = metric, cfg, fix
        ctx.save_for_backward(test, reference, Q)
        return res[-1].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_jod):
        test, reference, Q = ctx.saved_tensors
        grad_t = grad_r = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            with torch.cuda.device(ctx.metric.device):
                grad_t, grad_r = _backward(ctx.metric, test, reference, ctx.cfg, ctx.fix, Q, grad_jod, ctx.needs_input_grad[0],
                                           ctx.needs_input_grad[1])
        return grad_t, grad_r, None, None, None


def jod_video_held(metric, test, reference, dim_order="BCFHW", frames_per_second=0, fixation_point=None, test_frames=1,
                   reference_frames=1, wrt="test"):
    """fvvdp.jod_video_held (see there)."""
    name = "jod_video_held"
    check_wrt(wrt)
    refuse_unsupported(name, metric, test, reference, wrt)
    t, r, m_t, m_r = _arguments(name, metric, test, reference, dim_order, frames_per_second, test_frames, reference_frames,
                                FLOAT_DTYPES)
    if _is_identity(m_t, t.shape[2]) and _is_identity(m_r, r.shape[2]):
        return metric.jod_video(test, reference, dim_order=dim_order, frames_per_second=frames_per_second,
                                fixation_point=fixation_point, wrt=wrt)
    metric._check_device()
    if t.dtype != r.dtype:                  # a mixed pair: the narrower side upcast inside autograd's view (image_grad.float_pair)
        t, r = t.float(), r.float()
    if wrt == "test":
        r = r.detach()
    elif wrt == "reference":
        t = t.detach()
    t, r = _place(metric, t), _place(metric, r)
    fix = metric._fixation(fixation_point, t.shape[4], t.shape[3], len(m_t)) if metric.foveated else None
    return JodVideoHeldFunction.apply(t, r, metric, (float(frames_per_second), m_t, m_r), fix)


def predict_held(metric, test, reference, dim_order="BCFHW", frames_per_second=0, fixation_point=None, test_frames=1,
                 reference_frames=1):
    """fvvdp.predict_held (see there)."""
    name = "predict_held"
    for a in (test, reference):
        if isinstance(a, torch.Tensor) and a.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("predict_held is forward-only and this test or reference requires grad; detach it "
                               "(differentiable: fvvdp.jod_video_held)")
    t, r, m_t, m_r = _arguments(name, metric, test, reference, dim_order, frames_per_second, test_frames, reference_frames,
                                SAMPLE_DTYPES)
    if _is_identity(m_t, t.shape[2]) and _is_identity(m_r, r.shape[2]):
        return metric.predict(test, reference, dim_order=dim_order, frames_per_second=frames_per_second,
                              fixation_point=fixation_point)
    floats = t.dtype in FLOAT_DTYPES or r.dtype in FLOAT_DTYPES or t.dtype != r.dtype
    if floats and native_eotf(metric.display_photometry) is None:
        raise RuntimeError("%s needs a display model with a closed form for float input (sRGB, gamma, PQ, linear or absolute); "
                           "a user photometry class has none" % name)
    metric._check_device()
    if t.dtype != r.dtype:                  # each array unpacked by its own dtype, as predict does for a mixed pair
        t, r = metric._to_unit_float(t), metric._to_unit_float(r)
    t, r = _place(metric, t), _place(metric, r)
    fix = metric._fixation(fixation_point, t.shape[4], t.shape[3], len(m_t)) if metric.foveated else None
    with torch.cuda.device(metric.device):
        s = HeldClipSetup(metric, t, float(frames_per_second), r, m_t, m_r)
        res, Q = _forward(s, fix)
        res_h = metric._to_host(res)                       # the one host synchronisation of the call
    nq = Q.numel()
    stats = {"Q_per_ch": res_h[:nq].view(s.n_bands, 2, s.N).numpy(), "rho_band": s.rho_band,
             "frames_per_second": frames_per_second, "width": s.W, "height": s.H, "N_frames": s.N}
    if int(res_h[nq:nq + 1].view(torch.int32)[0]) != 0:
        logging.warning("Pixel outside the valid range 0-1")
    return res[nq + 1], stats
