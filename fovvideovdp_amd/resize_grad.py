"""Clips whose test and reference have frame sizes of their own: fvvdp.predict_resized, fvvdp.jod_video_resized and the autograd
function of the latter (include/fvvdp_hip_resize.h).

Each stream is a float32 or uint8 clip at its own resolution; the target -- the display's resolution unless resize_resolution says
otherwise -- is the size the metric judges at.  The forward resizes inside the ingest (fvvdp_temporal_channels_resized: torch's
interpolate arithmetic, the clip to [0, 1], the display model and the temporal filter in one kernel) and then makes the launches
of predict / jod_video.  The backward is jod_video's per batch -- the map-writing pass and fvvdp_video_grad_frames into a clip-long
level-0 gradient at the target size -- and ends, once per clip, with the temporal transpose down to the luminance frames
(fvvdp_video_grad_luminance) and the adjoint of the resize (fvvdp_resize_grad): dJOD/dtest at the test's own resolution.  No RGB
clip at the target size exists at any point.  The launch layer is grad_passes.py's (ResizedClipSetup, forward_clip, ClipBuffers).

With test_frames= / reference_frames= (held.py's frame maps) each stream also has a frame COUNT of its own
(include/fvvdp_hip_resize_held.h):

    predict_resized(test, ref, test_frames=a, reference_frames=b, ...)
        == predict_resized(test.index_select(frames, m_t), ref.index_select(frames, m_r), ...)

bit for bit (JOD and Q_per_ch).  The ingest reads each stream through its map and converts a held frame once
(fvvdp_temporal_channels_resized_held, ResizedHeldClipSetup); the backward keeps the luminance gradient at the display's rate and
ends with fvvdp_resize_grad_held, which sums it over the display frames that show a source frame before the resize's adjoint runs,
once per SOURCE frame.  No expanded clip exists at any point."""
import ctypes as C
import numbers

import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .display_model import native_eotf
from .fvvdp import filter_length
from .grad_passes import (ResizedClipSetup, ResizedHeldClipSetup, _fold_arrays, _ptr, batches, fold_list, forward_clip, grad_batch_size, level0_backward,
                          level0_buffers, resize_stream)
from .held import _is_identity, frame_maps
from .video_grad import video_grad_planes
from .video_source import fvvdp_video_source_array, reshuffle_dims

# frames the first stage of the adjoint holds at once (C x Ho x Wo floats each): enough to fill the device at any size the metric
# takes, small beside the clip-long buffers
ADJOINT_FRAMES = 4


def _default_frames(spec):
    """Is test_frames= / reference_frames= left at the int 1?"""
    return isinstance(spec, numbers.Integral) and not isinstance(spec, bool) and int(spec) == 1


def _clip(name, what, x, dim_order, constant, held=False):
    """One clip as a [C, N, H, W] tensor (a view where possible).  The test must be float32 when it is differentiated; otherwise
    float32 or uint8.  held: the stream is shown through a frame map, so one frame is a clip too."""
    dt = str(getattr(x, "dtype", type(x).__name__)).replace("torch.", "")
    if dt not in (("float32", "uint8") if constant else ("float32",)):
        raise RuntimeError("%s takes float32 %ssamples; the %s is %s.  Half-precision, float64 and uint16 samples are not supported"
                           % (name, "or uint8 " if constant else "", what, dt))
    t = fvvdp_video_source_array._as_tensor(x)
    d = dim_order.upper()
    if len(d) != t.dim():
        raise RuntimeError('Input tensor much have exactly as many dimensions as there are characters in the "dims" parameter')
    if len(set(d)) != len(d) or set(d) - set("BCFHW") or "H" not in d or "W" not in d:
        raise RuntimeError('dim_order must be made of distinct letters of "BCFHW" and contain H and W, got "%s"' % dim_order)
    if held and "F" in d and t.shape[d.index("F")] >= 1:
        pass                                                 # (the display count is checked with the maps)
    elif "F" not in d or t.shape[d.index("F")] < 2:
        raise RuntimeError("%s needs clips: an F axis of at least 2 frames in dim_order (single images are not resized here)" % name)
    if "B" in d and t.shape[d.index("B")] != 1:
        raise RuntimeError("%s takes one clip per call (B must be 1)" % name)
    t = reshuffle_dims(t, d, "BCFHW")[0]
    if t.shape[0] != 1 and t.shape[0] != 3:
        raise RuntimeError('The content must have either 1 or 3 colour channels.')
    return t


def _arguments(name, metric, test, reference, full_screen_resize, resize_resolution, dim_order, frames_per_second, grad,
               test_frames=1, reference_frames=1):
    """Everything that is refused before device work.  Returns (test, reference) as [C, N, H, W] views, the mode's code, the
    target (width, height) and the frame maps (m_t, m_r) -- None when test_frames and reference_frames are both left at 1 or
    both maps are the identity on streams of one frame count: today's call."""
    held = not (_default_frames(test_frames) and _default_frames(reference_frames))
    if full_screen_resize not in nat.RESIZE_MODES:
        raise RuntimeError("Unknown resize method '%s'" % (full_screen_resize,))
    if native_eotf(metric.display_photometry) is None:
        raise RuntimeError("%s needs a display model with a closed form (sRGB, gamma, PQ, linear or absolute): samples are "
                           "fractional after the resize, so a look-up table or a user photometry class has none" % name)
    if grad and isinstance(reference, torch.Tensor) and reference.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("%s: gradients with respect to the reference are not supported; detach the reference" % name)
    t = _clip(name, "test", test, dim_order, not grad, held)
    r = _clip(name, "reference", reference, dim_order, True, held)
    if t.shape[0] != r.shape[0]:
        raise RuntimeError("%s: test and reference differ in their channel counts (%d and %d)" % (name, t.shape[0], r.shape[0]))
    maps = None
    if held:
        m_t, m_r = frame_maps(test_frames, reference_frames, t.shape[1], r.shape[1])           # (held.frame_map's ValueErrors)
        if not (t.shape[1] == r.shape[1] and _is_identity(m_t, t.shape[1]) and _is_identity(m_r, r.shape[1])):
            maps = (m_t, m_r)
    elif t.shape[1] != r.shape[1]:
        raise RuntimeError("%s: test and reference differ in their frame counts (%d and %d)" % (name, t.shape[1], r.shape[1]))
    if not frames_per_second > 0:
        raise RuntimeError("When passing video sequences, you must set frames_per_second parameter")
    fl = filter_length(frames_per_second)
    if fl > nat.RESIZE_MAX_TAPS:
        raise RuntimeError("%s: frame rate too high: its temporal filter has %d taps, the resizing ingest covers %d "
                           "(120 frames per second have 30)" % (name, fl, nat.RESIZE_MAX_TAPS))
    if resize_resolution is None:
        resize_resolution = metric.display_geometry.resolution
    Wo, Ho = int(resize_resolution[0]), int(resize_resolution[1])
    if Wo < 1 or Ho < 1:
        raise RuntimeError("%s: bad resize_resolution %dx%d" % (name, Wo, Ho))
    return t, r, nat.RESIZE_MODES[full_screen_resize], (Wo, Ho), maps


def _same_size(t, r, size):
    return all((x.shape[3], x.shape[2]) == size for x in (t, r))


def _place(metric, x):
    """The clip [C, N, H, W] on the metric's device with dense planes (H x W contiguous); what has to be copied is copied inside
    autograd's view."""
    x = x.to(metric.device)
    Cn, N, H, W = x.shape
    ps, fs = x.stride(0), x.stride(1)
    # planes of H x W, frames inside a plane ([C][N]) or planes inside a frame ([N][C]), gaps allowed
    nested = (fs >= H * W and ps >= N * fs) or (ps >= H * W and fs >= Cn * ps)
    return x if x.stride(3) == 1 and x.stride(2) == W and nested else x.contiguous()


def _setup(metric, t, r, cfg):
    fps, mode, size, maps = cfg
    if maps is None:
        return ResizedClipSetup(metric, t, fps, r, mode, size)
    return ResizedHeldClipSetup(metric, t, fps, r, mode, size, *maps)


def _luminance_grad(metric, t, r, cfg, fix, Q, gamma):
    """The backward down to the luminance frames: (setup, gL [N, Ho, Wo] = gamma * dJOD/dLuminance of the test at the DISPLAY's
    rate and the target size, bytes of the adjoint's workspace).  t: the placed test clip [C, F, h, w]."""
    fps, mode, size, maps = cfg
    s = _setup(metric, t, r, cfg)
    N, HW, Cn, F = s.N, s.H * s.W, s.C, t.shape[1]
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, video_grad_planes("test"))
    tables = nat.resize_grad_table_bytes(t.shape[3], t.shape[2]) if maps is None else \
        nat.resize_grad_held_table_bytes(t.shape[3], t.shape[2], F)
    work_bytes = tables + 4 * min(F, ADJOINT_FRAMES) * Cn * HW
    # beside ClipBuffers' own: the clip-long luminance gradient, the result and the adjoint's workspace
    buf = level0_buffers("jod_video_resized", metric, s, None, gb, True, False, results=False,
                         extra_bytes=4 * N * HW + 4 * t.numel() + work_bytes)
    prm = s.params()
    gamma = gamma.to(device=metric.device, dtype=torch.float32).reshape(1).contiguous()
    lib = nat.lib()
    for b0, nb in batches(N, gb):
        buf.maps_pass(lib, metric, s, t, r, fix, b0, nb)
        level0_backward(buf, s, prm, Q, N, b0, nb, gamma, True, False)
    gL = torch.empty((N, s.H, s.W), dtype=torch.float32, device=metric.device)
    ff, fp = _fold_arrays(fold_list(s.widx, s.fl, N))
    i32p = C.POINTER(C.c_int32)
    nat.check(lib.fvvdp_video_grad_luminance(s.W, s.H, N, _ptr(buf.g0), ff.ctypes.data_as(i32p), fp.ctypes.data_as(i32p),
                                             nat.fptr(s.taps), s.fl, _ptr(gL), _ptr(buf.head), buf.head.numel() * 4, s.stream))
    return s, gL, work_bytes


def _backward(metric, t, r, cfg, fix, Q, gamma):
    """gamma * dJOD/dt for the placed test clip t [C, F, h, w] (F: its own frame count; N below: display frames)."""
    mode, maps = cfg[1], cfg[3]
    s, gL, work_bytes = _luminance_grad(metric, t, r, cfg, fix, Q, gamma)
    N, F = s.N, t.shape[1]
    lib = nat.lib()
    # the gradient is written with the test's strides (every sample of the view once; what lies between its planes is not touched)
    grad = torch.empty_strided(t.shape, t.stride(), dtype=torch.float32, device=metric.device)
    work = torch.empty(work_bytes, dtype=torch.uint8, device=metric.device)
    ts = resize_stream(t)
    if maps is None:
        nat.check(lib.fvvdp_resize_grad(s.W, s.H, N, _ptr(gL), C.byref(ts), _ptr(grad), mode, C.byref(s.e), nat.fptr(s.w), _ptr(work),
                                        work_bytes, s.stream))
    else:
        # gL stays at the display's rate; the sum over a source frame's display frames is the adjoint's first step
        nat.check(lib.fvvdp_resize_grad_held(s.W, s.H, N, F, _ptr(gL), s.m_t.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ts),
                                             _ptr(grad), mode, C.byref(s.e), nat.fptr(s.w), _ptr(work), work_bytes, s.stream))
    return grad


class JodVideoResizedFunction(torch.autograd.Function):
    """Test and reference clips [C, N, h, w] (placed: _place) -> JOD (0-d, fp32)."""

    @staticmethod
    def forward(ctx, test, reference, metric, cfg, fix):
        with torch.cuda.device(metric.device):
            jod, Q = forward_clip(_setup(metric, test, reference, cfg), fix)
        ctx.metric, ctx.cfg, ctx.fix = metric, cfg, fix
        ctx.save_for_backward(test, reference, Q)
        return jod.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_jod):
        test, reference, Q = ctx.saved_tensors
        g = None
        if ctx.needs_input_grad[0]:
            with torch.cuda.device(ctx.metric.device):
                g = _backward(ctx.metric, test, reference, ctx.cfg, ctx.fix, Q, grad_jod)
        return g, None, None, None, None


def jod_video_resized(metric, test, reference, full_screen_resize="bilinear", resize_resolution=None, dim_order="BCFHW",
                      frames_per_second=30, fixation_point=None, test_frames=1, reference_frames=1):
    """fvvdp.jod_video_resized (see there)."""
    name = "jod_video_resized"
    t, r, mode, size, maps = _arguments(name, metric, test, reference, full_screen_resize, resize_resolution, dim_order,
                                        frames_per_second, True, test_frames, reference_frames)
    if _same_size(t, r, size):
        if maps is not None:
            return metric.jod_video_held(test, reference, dim_order=dim_order, frames_per_second=frames_per_second,
                                         fixation_point=fixation_point, test_frames=maps[0], reference_frames=maps[1])
        return metric.jod_video(test, reference, dim_order=dim_order, frames_per_second=frames_per_second,
                                fixation_point=fixation_point)
    metric._check_device()
    t, r = _place(metric, t), _place(metric, r.detach())
    N = t.shape[1] if maps is None else len(maps[0])                  # display frames
    fix = metric._fixation(fixation_point, size[0], size[1], N) if metric.foveated else None
    return JodVideoResizedFunction.apply(t, r, metric, (float(frames_per_second), mode, size, maps), fix)


def predict_resized(metric, test, reference, full_screen_resize="bilinear", resize_resolution=None, dim_order="BCFHW",
                    frames_per_second=30, fixation_point=None, test_frames=1, reference_frames=1):
    """fvvdp.predict_resized (see there)."""
    name = "predict_resized"
    for a in (test, reference):
        if isinstance(a, torch.Tensor) and a.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("predict_resized is forward-only and this test or reference requires grad; detach it "
                               "(differentiable: fvvdp.jod_video_resized)")
    t, r, mode, size, maps = _arguments(name, metric, test, reference, full_screen_resize, resize_resolution, dim_order,
                                        frames_per_second, False, test_frames, reference_frames)
    if _same_size(t, r, size):
        if maps is not None:
            return metric.predict_held(test, reference, dim_order=dim_order, frames_per_second=frames_per_second,
                                       fixation_point=fixation_point, test_frames=maps[0], reference_frames=maps[1])
        return metric.predict(test, reference, dim_order=dim_order, frames_per_second=frames_per_second,
                              fixation_point=fixation_point)
    metric._check_device()
    t, r = _place(metric, t), _place(metric, r)
    N = t.shape[1] if maps is None else len(maps[0])                  # display frames
    fix = metric._fixation(fixation_point, size[0], size[1], N) if metric.foveated else None
    with torch.cuda.device(metric.device):
        s = _setup(metric, t, r, (float(frames_per_second), mode, size, maps))
        jod, Q = forward_clip(s, fix)
        stats = {"Q_per_ch": Q.cpu().numpy(), "rho_band": s.rho_band, "frames_per_second": frames_per_second, "width": s.W,
                 "height": s.H, "N_frames": s.N}
    return jod, stats
