"""Differentiable JOD of a planar YUV clip: fvvdp.jod_video_yuv and its autograd function (include/fvvdp_hip_yuv_grad.h).

The test clip is float32 code values in limited range, as a learned codec or post-filter produces them: three planes (Y, U, V) or
one packed tensor with the layout of fvvdp_video_source_yuv_frames.  The forward ingests the planes where they lie
(fvvdp_temporal_channels_yuv_planes: the unpack of fvvdp_temporal_channels_yuv with the sample in the place of (float)code, fused
with the temporal filter) and then makes the launches of jod_video.  The backward is jod_video's per batch -- the map-writing pass
and fvvdp_video_grad_frames into a clip-long level-0 gradient -- and ends, once per clip, with the temporal transpose down to the
luminance frames (fvvdp_video_grad_luminance) and the adjoint of the unpack (fvvdp_yuv_grad_planes): dJOD/dY, dJOD/dU, dJOD/dV.
No RGB clip exists at any point.  The launch layer is grad_passes.py's (YuvClipSetup, forward_clip, ClipBuffers)."""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from . import utils
from .display_model import native_eotf
from .fvvdp import filter_length
from .grad_passes import (YuvClipSetup, _fold_arrays, _ptr, batches, fold_list, forward_clip, grad_batch_size, level0_backward,
                          level0_buffers, yuv_planes)
from .video_grad import video_grad_planes
from .video_source_yuv import YCBCR2RGB

NAME = "jod_video_yuv"


def _format(bit_depth, chroma_ss, color_space):
    """(fvvdp_yuv_format, luminance weights) as fvvdp_video_source_yuv_frames chooses them for `color_space`."""
    fmt = nat.YuvFormat()
    fmt.bit_depth, fmt.chroma_420 = int(bit_depth), 1 if chroma_ss == "420" else 0
    matrix = YCBCR2RGB["bt2020nc" if color_space == "bt2020nc" else "bt709"]
    for i, v in enumerate(np.asarray(matrix, dtype=np.float32).reshape(-1)):
        fmt.ycbcr2rgb[i] = float(v)
    spaces = utils.config_files.load("color_spaces.json")
    w = np.asarray(spaces["BT.2020" if color_space == "bt2020nc" else "sRGB"]["RGB2Y"], dtype=np.float32)
    return fmt, w


def _as_float_planes(what, x, constant):
    """A tensor of samples as float32.  The test must be float32; a constant may also be the integer codes the YUV source class
    takes (uint8, or 10-16 bit values as uint16 / int16 bit patterns / int32), converted once -- exact up to 16 bit."""
    if isinstance(x, np.ndarray):
        if x.dtype == np.uint16:
            x = x.astype(np.int32)
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor):
        raise RuntimeError("%s: the %s must be a tensor, a tuple (Y, U, V) of tensors or (the reference) an array of codes" % (NAME, what))
    if x.dtype is torch.float32:
        return x
    if constant and x.dtype in (torch.uint8, torch.int16, torch.int32):
        if x.dtype is torch.int16:
            return (x.to(torch.int32) & 0xFFFF).to(torch.float32)
        return x.to(torch.float32)
    raise RuntimeError("%s needs float32 planes of code values (the reference: float32 or the integer codes of "
                       "fvvdp_video_source_yuv_frames); the %s is %s.  Half-precision and float64 planes are not supported"
                       % (NAME, what, x.dtype))


def _planes(what, x, width, height, c420, constant):
    """(Y [N, H, W], U, V [N, uvh, uvw]) float32 views of `x`: a tuple of three planes, or one packed [N, H*W + 2*uvh*uvw] tensor
    (Y plane, U plane, V plane per frame) with width= and height=."""
    if isinstance(x, (tuple, list)):
        if len(x) != 3:
            raise RuntimeError("%s: the %s must be three planes (Y, U, V), got %d" % (NAME, what, len(x)))
        y, u, v = (_as_float_planes(what, p, constant) for p in x)
        if y.dim() != 3 or u.dim() != 3 or v.dim() != 3:
            raise RuntimeError("%s: the planes of the %s must be [N, H, W] and [N, H/2, W/2] (4:2:0) or [N, H, W] (4:4:4)" % (NAME, what))
        N, H, W = y.shape
        if (width is not None and int(width) != W) or (height is not None and int(height) != H):
            raise RuntimeError("%s: the Y plane of the %s is %dx%d, not the width=%s, height=%s given" % (NAME, what, W, H, width, height))
    else:
        x = _as_float_planes(what, x, constant)
        if width is None or height is None:
            raise RuntimeError("%s: a packed tensor needs width= and height=" % NAME)
        W, H = int(width), int(height)
        N = None
    if W < 1 or H < 1:
        raise RuntimeError("%s: bad frame size %dx%d" % (NAME, W, H))
    if c420 and (W % 2 or H % 2):
        raise RuntimeError("%s: 4:2:0 video needs even width and height (%dx%d)" % (NAME, W, H))
    uvh, uvw = (H // 2, W // 2) if c420 else (H, W)
    if N is None:
        elems = H * W + 2 * uvh * uvw
        if x.dim() != 2 or x.shape[1] != elems:
            raise RuntimeError("%s: the packed %s must be [N, %d] (H*W + 2*uvh*uvw samples per frame of %dx%d), got %s"
                               % (NAME, what, elems, W, H, tuple(x.shape)))
        # three views of the packed tensor: no copy, and the gradient reaches the packed tensor through them
        y = x[:, :H * W].unflatten(1, (H, W))
        u = x[:, H * W:H * W + uvh * uvw].unflatten(1, (uvh, uvw))
        v = x[:, H * W + uvh * uvw:].unflatten(1, (uvh, uvw))
    elif tuple(u.shape) != (N, uvh, uvw) or tuple(v.shape) != (N, uvh, uvw):
        raise RuntimeError("%s: the chroma planes of the %s must be [%d, %d, %d] for a %dx%d luma plane (%s), got %s and %s"
                           % (NAME, what, N, uvh, uvw, W, H, "4:2:0" if c420 else "4:4:4", tuple(u.shape), tuple(v.shape)))
    return y, u, v


def _place(metric, planes):
    """The planes on the metric's device with contiguous rows, U and V with one frame stride; what has to be copied is copied
    inside autograd's view."""
    def rows(p):
        p = p.to(metric.device)
        ok = p.stride(2) == 1 and p.stride(1) == p.shape[2] and p.stride(0) >= p.shape[1] * p.shape[2]
        return p if ok else p.contiguous()
    y, u, v = (rows(p) for p in planes)
    if u.stride(0) != v.stride(0):
        u, v = u.contiguous(), v.contiguous()
    return y, u, v


def _backward(metric, t, r, cfg, fix, Q, gamma):
    """gamma * (dJOD/dY, dJOD/dU, dJOD/dV) for the placed test planes t."""
    fps, fmt, w = cfg
    s = YuvClipSetup(metric, t, fps, r, fmt, w)
    N, HW = s.N, s.H * s.W
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, video_grad_planes("test"))
    uv = t[1].shape[1] * t[1].shape[2]
    # beside ClipBuffers' own: the clip-long luminance gradient and the three gradient planes
    buf = level0_buffers(NAME, metric, s, None, gb, True, False, results=False, extra_bytes=4 * N * (2 * HW + 2 * uv))
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
    grads = tuple(torch.empty(p.shape, dtype=torch.float32, device=metric.device) for p in t)
    tp, gp = yuv_planes(t), yuv_planes(grads)
    nat.check(lib.fvvdp_yuv_grad_planes(s.W, s.H, N, _ptr(gL), C.byref(tp), C.byref(gp), C.byref(fmt), C.byref(s.e),
                                        nat.fptr(w), s.stream))
    return grads


class JodVideoYuvFunction(torch.autograd.Function):
    """Test planes Y, U, V and reference planes (placed: _place) -> JOD (0-d, fp32)."""

    @staticmethod
    def forward(ctx, ty, tu, tv, ry, ru, rv, metric, cfg, fix):
        fps, fmt, w = cfg
        with torch.cuda.device(metric.device):
            jod, Q = forward_clip(YuvClipSetup(metric, (ty, tu, tv), fps, (ry, ru, rv), fmt, w), fix)
        ctx.metric, ctx.cfg, ctx.fix = metric, cfg, fix
        ctx.save_for_backward(ty, tu, tv, ry, ru, rv, Q)
        return jod.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_jod):
        ty, tu, tv, ry, ru, rv, Q = ctx.saved_tensors
        g = (None, None, None)
        if any(ctx.needs_input_grad[:3]):
            with torch.cuda.device(ctx.metric.device):
                g = _backward(ctx.metric, (ty, tu, tv), (ry, ru, rv), ctx.cfg, ctx.fix, Q, grad_jod)
            g = tuple(x if need else None for x, need in zip(g, ctx.needs_input_grad[:3]))
        return g + (None,) * 6


def jod_video_yuv(metric, test, reference, frames_per_second=0, width=None, height=None, bit_depth=8, chroma_ss="420",
                  color_space="bt709", fixation_point=None, full_screen_resize=None):
    """fvvdp.jod_video_yuv (see there)."""
    if chroma_ss not in ("420", "444"):
        raise RuntimeError("%s: unrecognized chroma subsampling %s (4:2:0 and 4:4:4 are supported, 4:2:2 is not)" % (NAME, chroma_ss))
    if not (8 <= int(bit_depth) <= 16):
        raise RuntimeError("%s: bit depth must be 8..16" % NAME)
    if full_screen_resize is not None:
        raise RuntimeError("%s: full_screen_resize is not differentiable here: resize the planes before the call" % NAME)
    if native_eotf(metric.display_photometry) is None:
        raise RuntimeError("%s needs a display model with a closed form (sRGB, gamma, PQ, linear or absolute): YUV samples are "
                           "fractional after the colour matrix, so a look-up table or a user photometry class has none" % NAME)
    grad_on = torch.is_grad_enabled()
    for p in reference if isinstance(reference, (tuple, list)) else (reference,):
        if isinstance(p, torch.Tensor) and p.requires_grad and grad_on:
            raise RuntimeError("%s: gradients with respect to the reference are not supported; detach the reference" % NAME)
    c420 = chroma_ss == "420"
    t = _planes("test", test, width, height, c420, False)
    r = _planes("reference", reference, t[0].shape[2], t[0].shape[1], c420, True)
    if any(tuple(a.shape) != tuple(b.shape) for a, b in zip(t, r)):
        raise RuntimeError("Test and reference image/video tensors must be exactly the same shape")
    if t[0].shape[0] < 2:
        raise RuntimeError("%s needs a clip of at least 2 frames" % NAME)
    if not frames_per_second > 0:
        raise RuntimeError("When passing video sequences, you must set frames_per_second parameter")
    fl = filter_length(frames_per_second)
    if fl > nat.YUV_GRAD_MAX_TAPS:
        raise RuntimeError("%s: frame rate too high: its temporal filter has %d taps, the ingest of float planes covers %d "
                           "(120 frames per second have 30)" % (NAME, fl, nat.YUV_GRAD_MAX_TAPS))
    metric._check_device()
    t = _place(metric, t)
    r = _place(metric, tuple(p.detach() for p in r))
    N, H, W = t[0].shape
    fix = metric._fixation(fixation_point, W, H, N) if metric.foveated else None
    cfg = (float(frames_per_second),) + _format(bit_depth, chroma_ss, color_space)
    return JodVideoYuvFunction.apply(*t, *r, metric, cfg, fix)
