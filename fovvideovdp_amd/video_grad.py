"""Differentiable video JOD: fvvdp.jod_video and its autograd function (include/fvvdp_hip_video_grad.h).

The forward makes the launches of fvvdp.predict for a device-resident float clip (fvvdp_temporal_channels per frame batch,
fvvdp_bands_forward, the pooling of fvvdp_bands_forward_pool on the last batch) with arguments from the same methods of the
metric, so the JOD is bit-identical to it.  The backward re-runs them per backward batch with every band's maps written,
fvvdp_video_grad_frames turns the maps and the forward's Q_per_ch into the gradient of level 0's two test planes (a clip-long
buffer), and one fvvdp_video_grad_input applies the transpose of the sliding-window temporal filter and the display model's
derivative.  With wrt="reference" / "both" the same maps plus the slope planes of the CSF look-up go to
fvvdp_video_ref_grad_frames (include/fvvdp_hip_ref_grad.h) and a second fvvdp_video_grad_input runs on the reference clip: one
ingest and one pyramid pass per backward batch whatever `wrt`.  Neither pass reads context scratch left by the other, and neither synchronises with the host."""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .fvvdp import filter_length, window_frame_indices      # filter_length: imported from here by tools
from .image_grad import check_wrt, float_pair, grad_batch_size, grad_planes, place, refuse_unsupported, slope_planes
from .video_source import fvvdp_video_source_array, reshuffle_dims

# fp32 planes per pyramid pixel and frame: maps (D 2 + contrast 4 + L_bkg 1 + S 2) and workspace (layer + sweep gradients of
# both channels)
GRAD_PLANES = 9 + 4


def video_grad_planes(wrt):
    """fp32 values per pyramid pixel and frame of a backward batch, per `wrt` (image_grad.grad_planes): 13, 17, 21."""
    return grad_planes(wrt, GRAD_PLANES, 9, 2)


def backward_bytes(gb, px, work_bytes, N, HW, numel, fl, n_inputs=1, slopes=False):
    """Device memory a backward pass allocates: the maps (and slope planes) of gb frames at px pyramid pixels each, the
    workspaces, the side buffer of the head, and per differentiated input the clip-long level-0 gradient and the result."""
    return gb * px * 4 * (9 + (2 if slopes else 0)) + work_bytes + fl * HW * 4 + n_inputs * (N * HW * 8 + numel * 4)


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


class _Setup:
    """What forward and backward share for one [1, C, N, H, W] clip: pyramid size, display model, taps, window list, context."""

    def __init__(self, metric, t, fps):
        _, self.C, self.N, self.H, self.W = t.shape
        self.n_bands, self.rho_band = metric._band_count(self.W, self.H)
        self.dtype, self.e = metric._image_eotf(t.dtype)          # float32, float16 or bfloat16 (float_pair)
        self.w = metric._rgb2y()
        self.fl, self.taps = metric._temporal_taps(fps)
        self.widx = window_frame_indices(self.N, self.fl, metric.temp_padding)
        self.batch = metric._batch_size(self.W, self.H, 4, self.N, self.fl)
        self.ctx = metric._context(self.W, self.H, self.n_bands, 4, self.batch, self.rho_band)
        self.stream = C.c_void_p(torch.cuda.current_stream(metric.device).cuda_stream)
        self.pp = metric._pool_params()

    def ingest(self, lib, t, r, b0, nb, oob):
        """Level 0 of slots [0, nb) for output frames [b0, b0 + nb): the launch _make_feeder's feed makes."""
        HW = self.H * self.W
        idx = np.ascontiguousarray(self.widx[b0:b0 + self.fl - 1 + nb])
        nat.check(lib.fvvdp_temporal_channels(self.ctx.handle, C.c_void_p(t.data_ptr()), C.c_void_p(r.data_ptr()), self.dtype,
                                              self.C, self.N * HW, HW, C.byref(self.e), nat.fptr(self.w),
                                              idx.ctypes.data_as(C.POINTER(C.c_int32)), nat.fptr(self.taps), self.fl, nb, 0,
                                              C.c_void_p(oob.data_ptr()), self.stream))


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
        fx, g, _keep = metric._fov_args(s.ctx, fix, b0, nb, s.n_bands, s.W, s.H)
        if b0 + nb == N:
            nat.check(lib.fvvdp_bands_forward_pool(s.ctx.handle, nb, C.c_void_p(Q.data_ptr()), N, b0, fx, g, None,
                                                   C.byref(s.pp), C.c_void_p(res[nq + 1:].data_ptr()), s.stream))
        else:
            nat.check(lib.fvvdp_bands_forward(s.ctx.handle, nb, C.c_void_p(Q.data_ptr()), N, b0, fx, g, None, s.stream))
    return res[nq + 1], Q


class _Buffers:
    """What a backward pass over the clip t allocates, shared by jod_video and jod_gazes (`name`): per differentiated input the
    result and the clip-long level-0 gradient, the head's side buffer, the maps and scratch of a backward batch of gb frames and
    a workspace of `work_bytes` (with `ref_bytes` > 0 the slope planes and the workspace of the reference's backward as well).
    Checked against the free device memory first: a sentence instead of an out-of-memory error.  results False: a caller that
    reduces the level-0 gradients instead of mapping them to the clip (display_grad.py) needs no result tensors."""

    def __init__(self, name, metric, s, t, gb, work_bytes, need_t=True, ref_bytes=0, results=True):
        N, dev, HW = s.N, metric.device, s.H * s.W
        need_r = ref_bytes > 0
        px = sum(w * h for w, h in metric._level_sizes(s.W, s.H, s.n_bands)[:s.n_bands])
        need = backward_bytes(gb, px, work_bytes + ref_bytes, N, HW, t.numel() if results else 0, s.fl,
                              int(need_t) + int(need_r), need_r)
        free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        if need > free:
            raise RuntimeError("%s: the backward of this clip needs %.1f GB of device memory (maps and workspace of %d "
                               "frames, the clip-long level-0 gradient and the result) and %.1f GB are free; set a smaller "
                               "metric.grad_batch or a shorter clip" % (name, need / 1e9, gb, free / 1e9))
        self.grad = self.g0 = self.work = self.grad_r = self.g0_r = self.work_r = None
        if need_t:
            self.grad = torch.empty_like(t) if results else None
            self.g0 = torch.empty((N, 2, s.H, s.W), dtype=torch.float32, device=dev)
            self.work = torch.empty((work_bytes + 3) // 4, dtype=torch.float32, device=dev)
        if need_r:
            self.grad_r = torch.empty_like(t) if results else None
            self.g0_r = torch.empty((N, 2, s.H, s.W), dtype=torch.float32, device=dev)
            self.work_r = torch.empty((ref_bytes + 3) // 4, dtype=torch.float32, device=dev)
            self.slopes, self._slopes = slope_planes(metric, gb, s.W, s.H, s.n_bands)
        self.head = torch.empty((s.fl, s.H, s.W), dtype=torch.float32, device=dev)
        self.maps_arr, self._maps = metric._band_maps(gb, s.W, s.H, s.n_bands, contrast_planes=4)
        self.work_bytes, self.ref_bytes = work_bytes, ref_bytes
        self.q_scratch = torch.empty((s.n_bands, 2, gb), dtype=torch.float32, device=dev)
        self.oob = torch.zeros(1, dtype=torch.int32, device=dev)

    def maps_pass(self, lib, metric, s, t, r, fix, b0, nb):
        """Ingest of frames [b0, b0 + nb) and the pyramid pass that writes every band's maps, under the gaze trace `fix`."""
        s.ingest(lib, t, r, b0, nb, self.oob)
        fx, g, _keep = metric._fov_args(s.ctx, fix, b0, nb, s.n_bands, s.W, s.H)
        if self.ref_bytes:
            nat.check(lib.fvvdp_ctx_set_slope_maps(s.ctx.handle, self.slopes))
        try:
            nat.check(lib.fvvdp_bands_forward(s.ctx.handle, nb, C.c_void_p(self.q_scratch.data_ptr()), nb, 0, fx, g,
                                              self.maps_arr, s.stream))
        finally:
            if self.ref_bytes:
                nat.check(lib.fvvdp_ctx_set_slope_maps(s.ctx.handle, None))

    def input_grad(self, lib, s, t, g0=None, grad=None):
        """A clip-long level-0 gradient (default: the test's) -> the gradient of the clip t: temporal transpose and the display
        model's derivative at t's samples."""
        g0 = self.g0 if g0 is None else g0
        grad = self.grad if grad is None else grad
        N, HW = s.N, s.H * s.W
        ff, fp = _fold_arrays(fold_list(s.widx, s.fl, N))
        nat.check(lib.fvvdp_video_grad_input_st(s.W, s.H, N, C.c_void_p(g0.data_ptr()), ff.ctypes.data_as(C.POINTER(C.c_int32)),
                                                fp.ctypes.data_as(C.POINTER(C.c_int32)), nat.fptr(s.taps), s.fl,
                                                C.c_void_p(t.data_ptr()), C.c_void_p(grad.data_ptr()), s.dtype, s.C, N * HW, HW,
                                                C.byref(s.e), nat.fptr(s.w), C.c_void_p(self.head.data_ptr()),
                                                self.head.numel() * 4, s.stream))
        return grad


def _backward(metric, t, r, fps, fix, Q, gamma, need_t=True, need_r=False):
    """(gamma * dJOD/dt, gamma * dJOD/dr) for the contiguous device clips t, r [1, C, N, H, W]; None for the one not asked for.
    The ingest and the map-writing pyramid pass run once per backward batch, whichever gradients follow."""
    s = _Setup(metric, t, fps)
    N, dev = s.N, metric.device
    wrt = "both" if need_t and need_r else ("reference" if need_r else "test")
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, video_grad_planes(wrt))
    lib = nat.lib()
    nbytes, rbytes = C.c_size_t(0), C.c_size_t(0)
    if need_t:
        nat.check(lib.fvvdp_video_grad_workspace(s.W, s.H, s.n_bands, gb, C.byref(nbytes)))
    if need_r:
        nat.check(lib.fvvdp_ref_grad_workspace(s.W, s.H, s.n_bands, gb, 2, C.byref(rbytes)))
    buf = _Buffers("jod_video", metric, s, t, gb, nbytes.value, need_t, rbytes.value)
    prm = metric.native_params()
    gamma = gamma.to(device=dev, dtype=torch.float32).reshape(1).contiguous()
    for b0 in range(0, N, gb):
        nb = min(gb, N - b0)
        buf.maps_pass(lib, metric, s, t, r, fix, b0, nb)
        if need_t:
            nat.check(lib.fvvdp_video_grad_frames(s.W, s.H, s.n_bands, nb, C.byref(prm), C.byref(s.pp), C.c_void_p(Q.data_ptr()),
                                                  N, b0, C.c_void_p(gamma.data_ptr()), buf.maps_arr,
                                                  C.c_void_p(buf.g0.data_ptr()), C.c_void_p(buf.work.data_ptr()), buf.work_bytes,
                                                  s.stream))
        if need_r:
            nat.check(lib.fvvdp_video_ref_grad_frames(s.W, s.H, s.n_bands, nb, C.byref(prm), C.byref(s.pp),
                                                      C.c_void_p(Q.data_ptr()), N, b0, C.c_void_p(gamma.data_ptr()), buf.maps_arr,
                                                      buf.slopes, C.c_void_p(buf.g0_r.data_ptr()),
                                                      C.c_void_p(buf.work_r.data_ptr()), buf.ref_bytes, s.stream))
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
