"""Differentiable video JOD: fvvdp.jod_video and its autograd function (include/fvvdp_hip_video_grad.h).

The forward runs the launches of fvvdp.predict for a device-resident float clip (fvvdp_temporal_channels per frame batch,
fvvdp_bands_forward, the pooling of fvvdp_bands_forward_pool on the last batch), so the JOD is bit-identical to it.  The
backward re-runs them per backward batch with every band's maps written, fvvdp_video_grad_frames turns the maps and the
forward's Q_per_ch into the gradient of level 0's two test planes (a clip-long buffer), and one fvvdp_video_grad_input applies
the transpose of the sliding-window temporal filter and the display model's derivative.  Neither pass reads context scratch
left by the other, and neither synchronises with the host."""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .display_model import native_eotf, native_geometry
from .image_grad import _sizes
from .video_source import fvvdp_video_source_array, reshuffle_dims

# Device memory one backward batch may hold in maps and workspace (the pyramid scratch of the context comes on top): 52 B per
# pyramid pixel and frame, i.e. 0.58 GB per 3840x2160 frame.  Chosen on the arithmetic alone (seven 4K frames per batch keep
# every launch of the batch above 10^7 band pixels, the clip-long buffers of a 60-frame 4K clip -- 10 GB -- fit beside it many
# times in 288 GB); not tuned on a measurement.
VIDEO_GRAD_BYTES_BUDGET = 4e9


def fold_list(idx, fl, N):
    """The head of the window index list (its first `fl` entries, chosen by the temporal padding) transposed: for every frame
    j in [0, N) the ascending list of head positions that show it.  Positions p >= fl are not listed: position p shows frame
    p - fl + 1, one per frame j >= 1."""
    idx = np.asarray(idx)
    if idx.shape != (N + fl - 1,) or not np.array_equal(idx[fl:], np.arange(1, N)[:len(idx) - fl]):
        raise RuntimeError("window index list must be a head of %d entries followed by frames 1 .. %d" % (fl, N - 1))
    out = [[] for _ in range(N)]
    for p in range(fl):
        out[int(idx[p])].append(p)
    return out


def _fold_arrays(folds):
    """fold_list's result as the two sorted arrays fvvdp_video_grad_input takes (frame, position)."""
    ff = np.asarray([j for j, ps in enumerate(folds) for _ in ps], dtype=np.int32)
    fp = np.asarray([p for ps in folds for p in ps], dtype=np.int32)
    return ff, fp


def filter_length(fps):
    """Taps of the temporal filters at `fps` frames per second (fvvdp.py:236 of the reference)."""
    return int(np.ceil(250.0 / (1000.0 / fps)))


class _Setup:
    """What forward and backward share for one [1, C, N, H, W] clip: pyramid size, display model, taps, window list, context."""

    def __init__(self, metric, t, fps):
        from .fvvdp import band_frequencies, window_frame_indices
        _, self.C, self.N, self.H, self.W = t.shape
        self.n_bands, self.rho_band = band_frequencies(self.W, self.H, metric.pix_per_deg)
        if self.n_bands < 1:
            raise RuntimeError("Frame %dx%d is too small for this display (no band-pass level)" % (self.W, self.H))
        self.dtype, self.e = metric._image_eotf(torch.float32)
        self.w = metric._rgb2y()
        # the temporal filters exactly as _predict_on_device caches them
        metric.filter_len = self.fl = filter_length(fps)
        fkey = (float(fps), self.fl, float(metric.sustained_sigma), float(metric.sustained_beta))
        if fkey not in metric._filters:
            F, _ = metric.get_temporal_filters(fps)
            metric._filters[fkey] = (F, np.ascontiguousarray(F.numpy(), dtype=np.float32))
        metric.F, self.taps = metric._filters[fkey]
        self.widx = window_frame_indices(self.N, self.fl, metric.temp_padding)
        self.batch = metric._batch_size(self.W, self.H, 4, self.N, self.fl)
        self.ctx = metric._context(self.W, self.H, self.n_bands, 4, self.batch, self.rho_band)
        self.stream = C.c_void_p(torch.cuda.current_stream(metric.device).cuda_stream)
        self.pp = nat.PoolParams(metric.beta_sch, metric.beta_tch, metric.beta_t, metric.w_transient, metric.jod_a,
                                 float(10.0 ** metric.log_jod_exp))

    def ingest(self, lib, t, r, b0, nb, oob):
        """Level 0 of slots [0, nb) for output frames [b0, b0 + nb): the launch _make_feeder's feed makes."""
        HW = self.H * self.W
        idx = np.ascontiguousarray(self.widx[b0:b0 + self.fl - 1 + nb])
        nat.check(lib.fvvdp_temporal_channels(self.ctx.handle, C.c_void_p(t.data_ptr()), C.c_void_p(r.data_ptr()), self.dtype,
                                              self.C, self.N * HW, HW, C.byref(self.e), nat.fptr(self.w),
                                              idx.ctypes.data_as(C.POINTER(C.c_int32)), nat.fptr(self.taps), self.fl, nb, 0,
                                              C.c_void_p(oob.data_ptr()), self.stream))

    def fov(self, metric, fix, b0, nb):
        """(fixation pointer, geometry pointer, keep-alive) of a foveated batch, as _predict_on_device passes them."""
        if not metric.foveated:
            return None, None, None
        fxa = np.ascontiguousarray(fix[b0:b0 + nb], dtype=np.float32)
        g = None
        if native_geometry(metric.display_geometry) is not None:
            g = C.byref(metric._geom_struct())
        else:
            metric._set_view_maps(self.ctx, self.n_bands, self.W, self.H)
            fxa = metric._gaze_view_dirs(fxa, self.W, self.H)
        return nat.fptr(fxa), g, fxa


def _forward(metric, t, r, fps, fix):
    """JOD (0-d) and Q_per_ch [n_bands, 2, N] on the device: the launches of predict(..., sync=False), no flag read back."""
    s = _Setup(metric, t, fps)
    N, dev = s.N, metric.device
    nq = s.n_bands * 2 * N
    res = torch.zeros(nq + 2, dtype=torch.float32, device=dev)          # Q_per_ch | range flag | JOD, as predict lays it out
    Q = res[:nq].view(s.n_bands, 2, N)
    oob = res[nq:nq + 1].view(torch.int32)
    lib = nat.lib()
    for b0 in range(0, N, s.batch):
        nb = min(s.batch, N - b0)
        s.ingest(lib, t, r, b0, nb, oob)
        fx, g, _keep = s.fov(metric, fix, b0, nb)
        if b0 + nb == N:
            nat.check(lib.fvvdp_bands_forward_pool(s.ctx.handle, nb, C.c_void_p(Q.data_ptr()), N, b0, fx, g, None,
                                                   C.byref(s.pp), C.c_void_p(res[nq + 1:].data_ptr()), s.stream))
        else:
            nat.check(lib.fvvdp_bands_forward(s.ctx.handle, nb, C.c_void_p(Q.data_ptr()), N, b0, fx, g, None, s.stream))
    return res[nq + 1], Q


def grad_batch_size(metric, W, H, n_bands, batch):
    """Frames per backward batch: the context's batch, capped by VIDEO_GRAD_BYTES_BUDGET of maps + workspace
    (metric.grad_batch overrides the cap, as for images)."""
    gb = getattr(metric, "grad_batch", None)
    if gb is not None:
        return max(1, min(int(gb), batch))
    return max(1, min(batch, int(VIDEO_GRAD_BYTES_BUDGET // _bytes_per_frame(W, H, n_bands))))


def _bytes_per_frame(W, H, n_bands):
    """Maps (D 2 + contrast 4 + L_bkg 1 + S 2 planes) and workspace (layer + sweep gradients of both channels) of one frame."""
    return sum(w * h for w, h in _sizes(W, H, n_bands)) * 4 * (9 + 4)


def _backward(metric, t, r, fps, fix, Q, gamma):
    """gamma * dJOD/dt for the contiguous device clip t [1, C, N, H, W]."""
    s = _Setup(metric, t, fps)
    N, dev, HW = s.N, metric.device, s.H * s.W
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch)
    lib = nat.lib()
    nbytes = C.c_size_t()
    nat.check(lib.fvvdp_video_grad_workspace(s.W, s.H, s.n_bands, gb, C.byref(nbytes)))
    # everything this pass allocates, against the free device memory: a sentence instead of an out-of-memory error
    px = sum(w * h for w, h in _sizes(s.W, s.H, s.n_bands)[:s.n_bands])
    need = gb * px * 4 * 9 + nbytes.value + N * HW * 8 + t.numel() * 4 + s.fl * HW * 4
    free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    if need > free:
        raise RuntimeError("jod_video: the backward of this clip needs %.1f GB of device memory (maps and workspace of %d "
                           "frames, the clip-long level-0 gradient and the result) and %.1f GB are free; set a smaller "
                           "metric.grad_batch or a shorter clip" % (need / 1e9, gb, free / 1e9))
    grad = torch.empty_like(t)
    g0 = torch.empty((N, 2, s.H, s.W), dtype=torch.float32, device=dev)
    head = torch.empty((s.fl, s.H, s.W), dtype=torch.float32, device=dev)
    sizes = _sizes(s.W, s.H, s.n_bands)
    maps_arr = (nat.BandMaps * s.n_bands)()
    keep = []
    for b in range(s.n_bands):
        w, h = sizes[b]
        D = torch.empty((gb, 2, h, w), dtype=torch.float32, device=dev)
        Cn = torch.empty((gb, 4, h, w), dtype=torch.float32, device=dev)
        L = torch.empty((gb, h, w), dtype=torch.float32, device=dev)
        S = torch.empty((gb, 2, h, w), dtype=torch.float32, device=dev)
        keep += [D, Cn, L, S]
        maps_arr[b].d_D, maps_arr[b].d_contrast, maps_arr[b].d_lbkg, maps_arr[b].d_S = (
            D.data_ptr(), Cn.data_ptr(), L.data_ptr(), S.data_ptr())
    work = torch.empty((nbytes.value + 3) // 4, dtype=torch.float32, device=dev)
    q_scratch = torch.empty((s.n_bands, 2, gb), dtype=torch.float32, device=dev)
    oob = torch.zeros(1, dtype=torch.int32, device=dev)
    prm = metric.native_params()
    gamma = gamma.to(device=dev, dtype=torch.float32).reshape(1).contiguous()
    for b0 in range(0, N, gb):
        nb = min(gb, N - b0)
        s.ingest(lib, t, r, b0, nb, oob)
        fx, g, _keep = s.fov(metric, fix, b0, nb)
        nat.check(lib.fvvdp_bands_forward(s.ctx.handle, nb, C.c_void_p(q_scratch.data_ptr()), nb, 0, fx, g, maps_arr, s.stream))
        nat.check(lib.fvvdp_video_grad_frames(s.W, s.H, s.n_bands, nb, C.byref(prm), C.byref(s.pp), C.c_void_p(Q.data_ptr()), N,
                                              b0, C.c_void_p(gamma.data_ptr()), maps_arr, C.c_void_p(g0.data_ptr()),
                                              C.c_void_p(work.data_ptr()), nbytes.value, s.stream))
    ff, fp = _fold_arrays(fold_list(s.widx, s.fl, N))
    nat.check(lib.fvvdp_video_grad_input(s.W, s.H, N, C.c_void_p(g0.data_ptr()), ff.ctypes.data_as(C.POINTER(C.c_int32)),
                                         fp.ctypes.data_as(C.POINTER(C.c_int32)), nat.fptr(s.taps), s.fl,
                                         C.c_void_p(t.data_ptr()), C.c_void_p(grad.data_ptr()), s.C, N * HW, HW, C.byref(s.e),
                                         nat.fptr(s.w), C.c_void_p(head.data_ptr()), head.numel() * 4, s.stream))
    return grad


class JodVideoFunction(torch.autograd.Function):
    """test [1, C, N, H, W] (contiguous fp32 on the metric's device), reference (the same, constant) -> JOD (0-d)."""

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
        grad = None
        if ctx.needs_input_grad[0]:
            with torch.cuda.device(ctx.metric.device):
                grad = _backward(ctx.metric, test, reference, ctx.fps, ctx.fix, Q, grad_jod)
        return grad, None, None, None, None


def jod_video(metric, test, reference, dim_order="BCFHW", frames_per_second=0, fixation_point=None):
    """fvvdp.jod_video (see there)."""
    if isinstance(reference, torch.Tensor) and reference.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("jod_video: gradients with respect to the reference are not supported; detach the reference")
    if native_eotf(metric.display_photometry) is None:
        raise RuntimeError("jod_video needs a display model with a closed form for float input (sRGB, gamma, PQ, linear or "
                           "absolute); a user photometry class has none")
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
        raise RuntimeError("jod_video needs a clip: an F axis of at least 2 frames in dim_order (a single frame is a still "
                           "image: use jod_images)")
    if "B" in d and t.shape[d.index("B")] != 1:
        raise RuntimeError("jod_video takes one clip per call (B must be 1)")
    if t.dtype != torch.float32 or r.dtype != torch.float32:
        raise RuntimeError("jod_video needs float32 test and reference clips (got %s and %s)" % (t.dtype, r.dtype))
    if not frames_per_second > 0:
        raise RuntimeError("When passing video sequences, you must set frames_per_second parameter")
    fl = filter_length(frames_per_second)
    if fl > nat.VIDEO_GRAD_MAX_TAPS:
        raise RuntimeError("jod_video: frame rate too high for the backward: its temporal filter has %d taps, the transpose "
                           "kernel covers %d (256 frames per second)" % (fl, nat.VIDEO_GRAD_MAX_TAPS))
    t, r = reshuffle_dims(t, d, "BCFHW"), reshuffle_dims(r, d, "BCFHW")
    if t.shape[1] != 1 and t.shape[1] != 3:
        raise RuntimeError('The content must have either 1 or 3 colour channels.')
    metric._check_device()
    # the layout change and the move to the device stay visible to autograd: the gradient reaches the caller's own tensor
    t = t.to(metric.device).contiguous()
    r = r.detach().to(metric.device).contiguous()
    fix = None
    if metric.foveated:
        fix = metric._fixation(fixation_point, t.shape[4], t.shape[3], t.shape[2])
    return JodVideoFunction.apply(t, r, metric, float(frames_per_second), fix)
