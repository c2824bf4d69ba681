"""The launch layer the differentiable entry points share (image_grad, video_grad, gaze_grad, param_grad, display_grad).

One copy of what they all do between their own kernels: the setup of a call on a stack of stills or on a clip (pyramid size,
display block, taps, context, launch constants; overrides for the display block, the model constants and the taps are given at
construction), the forward loops of predict_images / predict (forward_images, forward_clip), the map-writing pass behind every
backward (Setup.write_maps, under the slope_maps bracket), the buffers and the memory check of a clip's backward (ClipBuffers),
the level-0 backward pair (level0_backward), the workspace idiom, and the validation of a parameter vector with the two
helpers of the entry points that differentiate one (_refuse, _apply).  Each pyramid launch is made at one place, with arguments
from the same methods of the metric as fvvdp._predict_image_group and fvvdp._predict_on_device use, which is what keeps every
forward bit-identical to predict_images / predict."""
import contextlib
import ctypes as C
import math

import numpy as np
import torch

from . import _native as nat
from .fvvdp import _PipelinedSourceFeeder, fvvdp as _fvvdp, window_frame_indices

# Device memory one backward batch (of image pairs, or of video frames) may hold in maps and workspace; the pyramid scratch of
# the context comes on top.  For video that is 52 B per pyramid pixel and frame, 0.58 GB per 3840x2160 frame.  Chosen on the
# arithmetic alone (seven 4K frames per batch keep every launch of the batch above 10^7 band pixels, the clip-long buffers of a
# 60-frame 4K clip -- 10 GB -- fit beside it many times in 288 GB); not tuned on a measurement.
GRAD_BYTES_BUDGET = 4e9


def _ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset)


def batches(total, size):
    """(b0, nb) of the batches of up to `size` that cover [0, total)."""
    return [(b0, min(size, total - b0)) for b0 in range(0, total, size)]


def grad_batch_size(metric, W, H, n_bands, batch, planes):
    """Pairs or frames per backward batch: the context's batch, capped by GRAD_BYTES_BUDGET of maps + workspace at `planes`
    fp32 values per pyramid pixel (metric.grad_batch overrides the cap, e.g. to run several backward batches on a small
    stack)."""
    gb = getattr(metric, "grad_batch", None)
    if gb is not None:
        return max(1, min(int(gb), batch))
    px = sum(w * h for w, h in metric._level_sizes(W, H, n_bands))
    return max(1, min(batch, int(GRAD_BYTES_BUDGET // (px * 4 * planes))))


def slope_planes(metric, n, width, height, n_bands):
    """The slope planes kappa [n][2][h_b][w_b] of every band (fvvdp_ctx_set_slope_maps) and the pointer array both entry points
    take; the caller keeps the tensors alive."""
    keep = [torch.empty((n, 2, h, w), dtype=torch.float32, device=metric.device)
            for w, h in metric._level_sizes(width, height, n_bands)[:n_bands]]
    return (C.c_void_p * n_bands)(*[k.data_ptr() for k in keep]), keep


@contextlib.contextmanager
def slope_maps(ctx, slopes):
    """`with slope_maps(ctx, slopes):` -- the pyramid passes inside also write the slopes of the CSF look-up into `slopes`; the
    context forgets the planes on the way out, whatever happened.  Nothing at all when slopes is None."""
    if slopes is not None:
        nat.check(nat.lib().fvvdp_ctx_set_slope_maps(ctx.handle, slopes))
    try:
        yield
    finally:
        if slopes is not None:
            nat.check(nat.lib().fvvdp_ctx_set_slope_maps(ctx.handle, None))


_NO_SLOPES = contextlib.nullcontext()          # for the launches that never have any: no generator per launch


def workspace_bytes(size_fn, *args):
    """What the library's `size_fn(*args, &bytes)` asks for."""
    n = C.c_size_t(0)
    nat.check(size_fn(*args, C.byref(n)))
    return n.value


def work_tensor(nbytes, dtype=torch.float32):
    """A tensor of `dtype` that covers nbytes, on the current device (every pass runs under torch.cuda.device(metric.device))."""
    size = torch.finfo(dtype).bits // 8
    return torch.empty((nbytes + size - 1) // size, dtype=dtype, device="cuda")


def workspace(size_fn, *args, dtype=torch.float32):
    """(bytes, tensor): workspace_bytes and a work_tensor of it (apart where a memory check stands between the two)."""
    n = workspace_bytes(size_fn, *args)
    return n, work_tensor(n, dtype)


class Maps:
    """Every band's maps (D, contrast of `planes` planes, L_bkg, S) for backward batches of up to gb pairs or frames, the scratch
    the map-writing pass pools into and, after add_slopes, the slope planes of the same batches."""

    def __init__(self, metric, W, H, n_bands, planes, gb):
        self.size = (metric, gb, W, H, n_bands)
        self.maps_arr, self._maps = metric._band_maps(gb, W, H, n_bands, contrast_planes=planes)
        self.slopes = None
        self.q_scratch = torch.empty((n_bands, 2, gb), dtype=torch.float32, device=metric.device)
        self.jod_scratch = torch.empty(gb, dtype=torch.float32, device=metric.device)

    def add_slopes(self, planes=None):
        """The pass writes the slope planes too: `planes` (slope_planes' pair, made earlier) or new ones, made now."""
        self.slopes, self._slopes = slope_planes(*self.size) if planes is None else planes
        return self


class _Setup:
    """What the passes of one call share: pyramid size, context, stream, model and pooling constants."""

    def _finish(self, metric, planes, prm, pp):
        self.metric, self.planes = metric, planes
        self.ctx = metric._context(self.W, self.H, self.n_bands, planes, self.batch, self.rho_band)
        self.stream = C.c_void_p(torch.cuda.current_stream(metric.device).cuda_stream)
        self.prm, self.pp = prm, metric._pool_params() if pp is None else pp

    def params(self):
        """The model constants the kernels after the pyramid take: the ones given, else the metric's own as they are now."""
        return self.metric.native_params() if self.prm is None else self.prm


class ImageSetup(_Setup):
    """A call on one [B, C, H, W] stack t (and reference r: ingest takes both as arguments, the passes below read them here).
    eotf: the display block in the place of the metric's own; prm, pp: fvvdp_params / fvvdp_pool_params likewise."""

    def __init__(self, metric, t, r=None, eotf=None, prm=None, pp=None):
        self.t, self.r = t, r
        self.B, self.C, self.H, self.W = t.shape
        self.n_bands, self.rho_band = metric._band_count(self.W, self.H)
        self.dtype, own = metric._image_eotf(t.dtype)             # float32, float16 or bfloat16 (image_grad.float_pair)
        self.e = own if eotf is None else eotf
        self.w = metric._rgb2y()
        self.batch = metric._batch_size(self.W, self.H, 2, self.B)
        self._finish(metric, 2, prm, pp)

    def ingest(self, lib, t, r, b0, nb):
        tp = (C.c_void_p * nb)(*[t[k].data_ptr() for k in range(b0, b0 + nb)])
        rp = (C.c_void_p * nb)(*[r[k].data_ptr() for k in range(b0, b0 + nb)])
        nat.check(lib.fvvdp_images_channels(self.ctx.handle, tp, rp, nb, self.dtype, self.C, self.H * self.W, C.byref(self.e),
                                            nat.fptr(self.w), 0, None, self.stream))
        return tp

    def launch(self, fix, b0, nb, Q, columns, col, jod, maps=None):
        """Ingest of pairs [b0, b0 + nb), pyramid pass and pooling: Q_per_ch into columns [col, col + nb) of Q [bands, 2, columns],
        the JODs to the pointer `jod`; with `maps` every band's maps (and its slope planes, if it has them) are written too.
        Returns the ingest's array of test pointers."""
        lib = nat.lib()
        tp = self.ingest(lib, self.t, self.r, b0, nb)
        fx, g, _keep = self.metric._fov_args(self.ctx, fix, b0, nb, self.n_bands, self.W, self.H)
        with _NO_SLOPES if maps is None or maps.slopes is None else slope_maps(self.ctx, maps.slopes):
            nat.check(lib.fvvdp_images_forward_pool(self.ctx.handle, nb, _ptr(Q), columns, col, fx, g, maps and maps.maps_arr,
                                                    C.byref(self.pp), jod, self.stream))
        return tp

    def write_maps(self, maps, fix, b0, nb):
        """The map-writing pass of pairs [b0, b0 + nb): a forward into scratch."""
        return self.launch(fix, b0, nb, maps.q_scratch, nb, 0, _ptr(maps.jod_scratch), maps)


def image_strides(x):
    """(image stride, plane stride) in elements of the stack [B, C, h, w]; an axis of size 1 has no stride to speak of: what a
    dense stack would have."""
    hw = x.shape[2] * x.shape[3]
    ps = x.stride(1) if x.shape[1] > 1 else hw
    return (x.stride(0) if x.shape[0] > 1 else x.shape[1] * ps), ps


def image_resize_stream(x, b0=0):
    """fvvdp_resize_stream of a device stack [B, C, h, w] (float32 or uint8; rows and planes dense) from image b0 on: image k is
    the stream's frame k."""
    fs, ps = image_strides(x)
    return nat.ResizeStream(x.data_ptr() + b0 * fs * x.element_size(), nat.FVVDP_U8 if x.dtype is torch.uint8 else nat.FVVDP_F32,
                            x.shape[1], x.shape[3], x.shape[2], fs, ps)


class ResizedImageSetup(ImageSetup):
    """ImageSetup for a pair of stacks with image sizes of their own (images_resize): t and r are [B, C, h, w] device tensors as
    image_resize_stream takes them, mode the FVVDP_RESIZE_* code, size the target (width, height) -- self.W and self.H, the size
    the pyramid runs at; the ingest is fvvdp_images_channels_resized.  launch, write_maps and forward_images are ImageSetup's."""

    def __init__(self, metric, t, r, mode, size, prm=None, pp=None):
        self.t, self.r, self.mode = t, r, mode
        self.B, self.C = t.shape[0], t.shape[1]
        self.W, self.H = size
        self.n_bands, self.rho_band = metric._band_count(self.W, self.H)
        self.dtype, self.e = metric._image_eotf(torch.float32)
        self.w = metric._rgb2y()
        self.batch = metric._batch_size(self.W, self.H, 2, self.B)
        self._finish(metric, 2, prm, pp)

    def ingest(self, lib, t, r, b0, nb):
        """(no pointer table, so none is returned; no range flag -- the clip to [0, 1] belongs to the resize)"""
        ts, rs = image_resize_stream(t, b0), image_resize_stream(r, b0)
        nat.check(lib.fvvdp_images_channels_resized(self.ctx.handle, C.byref(ts), C.byref(rs), nb, self.mode, C.byref(self.e),
                                                    nat.fptr(self.w), 0, self.stream))


def forward_images(s, fix):
    """JOD [B] and Q_per_ch [n_bands, 2, B] on the device: the launches of predict_images, no flags read back, no heat maps."""
    Q = torch.zeros((s.n_bands, 2, s.B), dtype=torch.float32, device=s.metric.device)
    jod = torch.empty(s.B, dtype=torch.float32, device=s.metric.device)
    for b0, nb in batches(s.B, s.batch):
        s.launch(fix, b0, nb, Q, s.B, b0, _ptr(jod, 4 * b0))
    return jod, Q


class ClipSetup(_Setup):
    """A call on one [1, C, N, H, W] clip t (and reference r, as ImageSetup): also the taps (`taps`: others than the metric's
    own at fps), the window list and the batch schedule of the forward.  The subclasses below bring sources of other kinds and
    the ingest that takes them; taps, window list, schedule, launch and write_maps are the ones here."""

    def __init__(self, metric, t, fps, r=None, eotf=None, prm=None, pp=None, taps=None):
        self.t, self.r, self.C = t, r, t.shape[1]
        # (samples: float32, float16 or bfloat16 -- image_grad.float_pair)
        self._clip(metric, t.shape[2], t.shape[4], t.shape[3], fps, 4, t.dtype, eotf=eotf, prm=prm, pp=pp, taps=taps)

    def _clip(self, metric, N, W, H, fps, planes, samples, eotf=None, w=None, prm=None, pp=None, taps=None):
        """The constructor tail of every clip setup, for N frames of W x H at fps and samples of the torch dtype `samples`; eotf,
        w (luminance weights), prm, pp, taps: overrides of the metric's own."""
        self.N, self.W, self.H = N, W, H
        self.n_bands, self.rho_band = metric._band_count(W, H)
        self.dtype, own = metric._image_eotf(samples)
        self.e = own if eotf is None else eotf
        self.w = metric._rgb2y() if w is None else w
        self.fl, own = metric._temporal_taps(fps)
        self.taps = own if taps is None else taps
        self.widx = window_frame_indices(N, self.fl, metric.temp_padding)
        self.batch = metric._batch_size(W, H, planes, N, self.fl)
        self.schedule = [nb for _, nb in batches(N, self.batch)]
        self._finish(metric, planes, prm, pp)

    def window(self, b0, nb, widx=None):
        """What output frames [b0, b0 + nb) read of the window list (widx: of another list laid out alike), contiguous."""
        return np.ascontiguousarray((self.widx if widx is None else widx)[b0:b0 + self.fl - 1 + nb])

    def ingest(self, lib, t, r, b0, nb, oob):
        """Level 0 of slots [0, nb) for output frames [b0, b0 + nb): the launch _make_feeder's feed makes."""
        HW = self.H * self.W
        idx = self.window(b0, nb)
        nat.check(lib.fvvdp_temporal_channels(self.ctx.handle, _ptr(t), _ptr(r), self.dtype, self.C, self.N * HW, HW,
                                              C.byref(self.e), nat.fptr(self.w), idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                              nat.fptr(self.taps), self.fl, nb, 0, _ptr(oob), self.stream))

    def launch(self, fix, b0, nb, oob, Q, columns, col, jod=None, maps=None, clips=None):
        """Ingest of frames [b0, b0 + nb) (range flag into oob) and the pyramid pass: Q_per_ch into columns [col, col + nb) of Q
        [bands, 2, columns]; jod (a pointer): the batch completes the clip and pools it into the JOD as well; maps: as
        ImageSetup.launch; clips: (t, r) to ingest in the place of the setup's own."""
        lib = nat.lib()
        self.ingest(lib, *(clips or (self.t, self.r)), b0, nb, oob)
        fx, g, _keep = self.metric._fov_args(self.ctx, fix, b0, nb, self.n_bands, self.W, self.H)
        with _NO_SLOPES if maps is None or maps.slopes is None else slope_maps(self.ctx, maps.slopes):
            if jod is not None:
                nat.check(lib.fvvdp_bands_forward_pool(self.ctx.handle, nb, _ptr(Q), columns, col, fx, g, maps and maps.maps_arr,
                                                       C.byref(self.pp), jod, self.stream))
            else:
                nat.check(lib.fvvdp_bands_forward(self.ctx.handle, nb, _ptr(Q), columns, col, fx, g, maps and maps.maps_arr,
                                                  self.stream))

    def write_maps(self, maps, fix, b0, nb, oob, clips=None):
        """The map-writing pass of frames [b0, b0 + nb): a forward into scratch."""
        self.launch(fix, b0, nb, oob, maps.q_scratch, nb, 0, None, maps, clips)


class PlanClipSetup(ClipSetup):
    """ClipSetup from a clip plan (metric._clip_plan(vs)): the sources are whatever the plan's feeder accepts -- integer, host --,
    the ingest is the feeder's and the forward walks the plan's schedule, whose chunk heights group the partial sums.  A single
    frame has 2 planes and one tap.  `name`: the entry point, for the refusal of a source without a closed-form display model."""

    @staticmethod
    def refuse_user_photometry(name, pl):
        if isinstance(pl.feeder, _PipelinedSourceFeeder):
            raise RuntimeError("%s needs a display model with a closed form for float input (sRGB, gamma, PQ, "
                               "linear or absolute); a user photometry class has none" % name)

    def __init__(self, name, metric, pl, prm=None, pp=None, taps=None):
        self.refuse_user_photometry(name, pl)
        self.t = self.r = None
        self.N, self.H, self.W, self.n_bands, self.rho_band = pl.N_frames, pl.height, pl.width, pl.n_bands, pl.rho_band
        self.fl, self.taps, self.widx = pl.fl, pl.taps if taps is None else taps, pl.widx
        self.feeder, self.batch, self.schedule = pl.feeder, pl.batch, pl.schedule
        self._finish(metric, pl.planes, prm, pp)

    def ingest(self, lib, t, r, b0, nb, oob):
        self.feeder(self.ctx, self.window(b0, nb), self.taps, self.fl, nb, oob, self.stream)


def yuv_planes(planes):
    """fvvdp_yuv_planes of the device tensors (Y [N, H, W], U, V [N, uvh, uvw]; rows contiguous, U and V with one frame stride)."""
    y, u, v = planes
    return nat.YuvPlanes(y.data_ptr(), u.data_ptr(), v.data_ptr(), y.stride(0), u.stride(0))


class YuvClipSetup(ClipSetup):
    """ClipSetup for a clip of float32 YUV planes (yuv_grad.jod_video_yuv): t and r are (Y, U, V) tuples as yuv_planes takes them,
    fmt the fvvdp_yuv_format, w the luminance weights of the YUV colour space; the ingest is fvvdp_temporal_channels_yuv_planes."""

    def __init__(self, metric, t, fps, r, fmt, w, prm=None, pp=None):
        self.t, self.r, self.fmt, self.C = t, r, fmt, 3
        N, H, W = t[0].shape
        self._clip(metric, N, W, H, fps, 4, torch.float32, w=w, prm=prm, pp=pp)

    def ingest(self, lib, t, r, b0, nb, oob):
        idx = self.window(b0, nb)
        tp, rp = yuv_planes(t), yuv_planes(r)
        nat.check(lib.fvvdp_temporal_channels_yuv_planes(self.ctx.handle, C.byref(tp), C.byref(rp), C.byref(self.fmt),
                                                         C.byref(self.e), nat.fptr(self.w),
                                                         idx.ctypes.data_as(C.POINTER(C.c_int32)), nat.fptr(self.taps), self.fl, nb,
                                                         0, _ptr(oob), self.stream))


def resize_stream(x):
    """fvvdp_resize_stream of a device clip [C, N, h, w] (float32 or uint8; rows and planes dense)."""
    return nat.ResizeStream(x.data_ptr(), nat.FVVDP_U8 if x.dtype is torch.uint8 else nat.FVVDP_F32, x.shape[0], x.shape[3],
                            x.shape[2], x.stride(1), x.stride(0))


class ResizedClipSetup(ClipSetup):
    """ClipSetup for a pair of clips with frame sizes of their own (resize_grad): t and r are [C, N, h, w] device tensors as
    resize_stream takes them, mode the FVVDP_RESIZE_* code, size the target (width, height) -- self.W and self.H, the size the
    pyramid runs at; the ingest is fvvdp_temporal_channels_resized."""

    def __init__(self, metric, t, fps, r, mode, size, prm=None, pp=None):
        self.t, self.r, self.mode, self.C = t, r, mode, t.shape[0]
        self._clip(metric, t.shape[1], size[0], size[1], fps, 4, torch.float32, prm=prm, pp=pp)

    def ingest(self, lib, t, r, b0, nb, oob):
        """(oob: the range flag of the other ingests stays as it is -- the clip to [0, 1] belongs to the resize)"""
        idx = self.window(b0, nb)
        ts, rs = resize_stream(t), resize_stream(r)
        nat.check(lib.fvvdp_temporal_channels_resized(self.ctx.handle, C.byref(ts), C.byref(rs), self.mode, C.byref(self.e),
                                                      nat.fptr(self.w), idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                                      nat.fptr(self.taps), self.fl, nb, 0, self.stream))


class ResizedHeldClipSetup(ResizedClipSetup):
    """ResizedClipSetup for a pair of clips with frame sizes AND frame counts of their own (resize_grad, with test_frames= /
    reference_frames=): t and r are [C, F_s, h, w] device tensors, m_t and m_r the frame maps (int32 [N]: display frame -> source
    frame).  As in HeldClipSetup self.N is the number of DISPLAY frames, at whose rate the window list, the schedule and the gaze
    run; the ingest is fvvdp_temporal_channels_resized_held on the window list sent through each stream's map."""

    def __init__(self, metric, t, fps, r, mode, size, m_t, m_r, prm=None, pp=None):
        self.t, self.r, self.mode, self.C = t, r, mode, t.shape[0]
        self.m_t, self.m_r = np.ascontiguousarray(m_t, dtype=np.int32), np.ascontiguousarray(m_r, dtype=np.int32)
        self._clip(metric, len(self.m_t), size[0], size[1], fps, 4, torch.float32, prm=prm, pp=pp)
        self.idx_t, self.idx_r = self.m_t[self.widx], self.m_r[self.widx]      # the per-stream lists handed to the ingest

    def ingest(self, lib, t, r, b0, nb, oob):
        i32p = C.POINTER(C.c_int32)
        it, ir = self.window(b0, nb, self.idx_t), self.window(b0, nb, self.idx_r)
        ts, rs = resize_stream(t), resize_stream(r)
        nat.check(lib.fvvdp_temporal_channels_resized_held(self.ctx.handle, C.byref(ts), C.byref(rs), t.shape[1], r.shape[1], self.mode,
                                                           C.byref(self.e), nat.fptr(self.w), it.ctypes.data_as(i32p),
                                                           ir.ctypes.data_as(i32p), nat.fptr(self.taps), self.fl, nb, 0, self.stream))


def held_stream(x):
    """fvvdp_held_stream of a device clip [1, C, F, H, W] whose frames are dense (H x W contiguous; held.dense_planar)."""
    return nat.HeldStream(x.data_ptr(), *held_strides(x), x.shape[2])


def held_strides(x):
    """(chan_stride, frame_stride) of the clip [1, C, F, H, W]; an axis of size 1 has no stride to speak of: one frame's size."""
    hw = x.shape[3] * x.shape[4]
    return (x.stride(1) if x.shape[1] > 1 else hw), (x.stride(2) if x.shape[2] > 1 else hw)


class HeldClipSetup(ClipSetup):
    """ClipSetup for a pair of clips with frame counts of their own (held.py): t and r are [1, C, F_s, H, W] device tensors as
    held_stream takes them, of one dtype; m_t and m_r the frame maps (int32 [N]: display frame -> source frame).  self.N is the
    number of DISPLAY frames, at whose rate the window list, the schedule and the gaze run; the ingest is
    fvvdp_temporal_channels_held on the window list sent through each stream's map."""

    def __init__(self, metric, t, fps, r, m_t, m_r, prm=None, pp=None):
        self.t, self.r, self.C = t, r, t.shape[1]
        self.m_t, self.m_r = np.ascontiguousarray(m_t, dtype=np.int32), np.ascontiguousarray(m_r, dtype=np.int32)
        self._clip(metric, len(self.m_t), t.shape[4], t.shape[3], fps, 4, t.dtype, prm=prm, pp=pp)
        self.idx_t, self.idx_r = self.m_t[self.widx], self.m_r[self.widx]      # the per-stream lists handed to the ingest

    def ingest(self, lib, t, r, b0, nb, oob):
        i32p = C.POINTER(C.c_int32)
        it, ir = self.window(b0, nb, self.idx_t), self.window(b0, nb, self.idx_r)
        ts, rs = held_stream(t), held_stream(r)
        nat.check(lib.fvvdp_temporal_channels_held(self.ctx.handle, C.byref(ts), C.byref(rs), self.dtype, self.C, C.byref(self.e),
                                                   nat.fptr(self.w), it.ctypes.data_as(i32p), ir.ctypes.data_as(i32p),
                                                   nat.fptr(self.taps), self.fl, nb, 0, _ptr(oob), self.stream))


def held_fold_arrays(m, widx, fl):
    """The head of the display-rate window list (its first `fl` positions) keyed by SOURCE frame through the frame map m: the two
    arrays fvvdp_video_grad_input_held takes -- (source frame, position), every head position exactly once, sorted by frame and
    then by position."""
    m, widx = np.asarray(m), np.asarray(widx)
    order = sorted((int(m[int(widx[p])]), p) for p in range(fl))
    return np.asarray([f for f, _ in order], dtype=np.int32), np.asarray([p for _, p in order], dtype=np.int32)


def forward_clip(s, fix):
    """JOD (0-d) and Q_per_ch [n_bands, 2, N] on the device: the launches of predict(..., sync=False), no flag read back."""
    nq = s.n_bands * 2 * s.N
    res = torch.zeros(nq + 2, dtype=torch.float32, device=s.metric.device)   # Q_per_ch | range flag | JOD, as predict lays it out
    Q = res[:nq].view(s.n_bands, 2, s.N)
    oob = res[nq:nq + 1].view(torch.int32)
    b0 = 0
    for nb in s.schedule:
        s.launch(fix, b0, nb, oob, Q, s.N, b0, _ptr(res[nq + 1:]) if b0 + nb == s.N else None)
        b0 += nb
    return res[nq + 1], Q


def backward_bytes(gb, px, work_bytes, N, HW, numel, fl, n_inputs=1, slopes=False, extra_bytes=0):
    """Device memory a backward pass allocates: the maps (and slope planes) of gb frames at px pyramid pixels each, the
    workspaces, the side buffer of the head, per differentiated input the clip-long level-0 gradient and the result, and
    whatever the caller holds beside them (extra_bytes)."""
    return (gb * px * 4 * (9 + (2 if slopes else 0)) + work_bytes + fl * HW * 4 + n_inputs * (N * HW * 8 + numel * 4)
            + extra_bytes)


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


class ClipBuffers:
    """What a backward pass over the clip of the setup s allocates, for the entry point `name`: per differentiated input the
    result (a tensor like t; not with results=False) and the clip-long level-0 gradient, the head's side buffer (head), the
    Maps of a backward batch of gb frames (maps; False: they come through use_maps) and a workspace of `work_bytes`; with
    `ref_bytes` > 0 the slope planes and the workspace of the reference's backward as well.  Checked against the free device
    memory first, the caller's own extra_bytes included: a sentence instead of an out-of-memory error (lum_bytes: the share
    of extra_bytes that the sentence of calibration_jod_video's tap gradient names)."""

    def __init__(self, name, metric, s, t, gb, work_bytes, need_t=True, ref_bytes=0, results=True, head=True, maps=True,
                 extra_bytes=0, lum_bytes=0):
        N, dev, HW = s.N, metric.device, s.H * s.W
        need_r = ref_bytes > 0
        px = sum(w * h for w, h in metric._level_sizes(s.W, s.H, s.n_bands)[:s.n_bands])
        need = backward_bytes(gb, px, work_bytes + ref_bytes, N, HW, t.numel() if results else 0, s.fl if head else 0,
                              int(need_t) + int(need_r), need_r, extra_bytes)
        free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        if need > free:
            what, held = "the backward of this clip", "the clip-long level-0 gradient and the result"
            if lum_bytes:
                what = "the gradient for the temporal parameters of this clip"
                held = ("the clip-long level-0 gradients of both sides and %.2f GB of luminance frames under a batch's windows"
                        % (lum_bytes / 1e9))
            raise RuntimeError("%s: %s needs %.1f GB of device memory (maps and workspace of %d frames, %s) and %.1f GB are "
                               "free; set a smaller metric.grad_batch or a shorter clip"
                               % (name, what, need / 1e9, gb, held, free / 1e9))
        self.grad = self.g0 = self.work = self.grad_r = self.g0_r = self.work_r = None
        if need_t:
            self.grad = torch.empty_like(t) if results else None
            self.g0 = torch.empty((N, 2, s.H, s.W), dtype=torch.float32, device=dev)
            self.work = work_tensor(work_bytes)
        if need_r:
            self.grad_r = torch.empty_like(t) if results else None
            self.g0_r = torch.empty((N, 2, s.H, s.W), dtype=torch.float32, device=dev)
            self.work_r = work_tensor(ref_bytes)
        # (slope planes, head, maps: the order the caching allocator has always been asked in)
        self._slopes = slope_planes(metric, gb, s.W, s.H, s.n_bands) if need_r else None
        self.head = torch.empty((s.fl, s.H, s.W), dtype=torch.float32, device=dev) if head else None
        self.maps = self.use_maps(Maps(metric, s.W, s.H, s.n_bands, 4, gb)) if maps else None
        self.work_bytes, self.ref_bytes = work_bytes, ref_bytes
        self.oob = torch.zeros(1, dtype=torch.int32, device=dev)

    def use_maps(self, maps):
        """`maps` become the maps of the batch (a caller that said maps=False brings its own, made after buffers of its own)."""
        self.maps = maps if self._slopes is None else maps.add_slopes(self._slopes)
        return self.maps

    def maps_pass(self, lib, metric, s, t, r, fix, b0, nb):
        """Ingest of frames [b0, b0 + nb) of the clips t, r and the pyramid pass that writes every band's maps, under the gaze
        trace `fix`."""
        s.write_maps(self.maps, fix, b0, nb, self.oob, (t, r))

    def input_grad(self, lib, s, t, g0=None, grad=None):
        """A clip-long level-0 gradient (default: the test's) -> the gradient of the clip t: temporal transpose and the display
        model's derivative at t's samples."""
        g0 = self.g0 if g0 is None else g0
        grad = self.grad if grad is None else grad
        N, HW = s.N, s.H * s.W
        ff, fp = _fold_arrays(fold_list(s.widx, s.fl, N))
        nat.check(lib.fvvdp_video_grad_input_st(s.W, s.H, N, _ptr(g0), ff.ctypes.data_as(C.POINTER(C.c_int32)),
                                                fp.ctypes.data_as(C.POINTER(C.c_int32)), nat.fptr(s.taps), s.fl, _ptr(t), _ptr(grad),
                                                s.dtype, s.C, N * HW, HW, C.byref(s.e), nat.fptr(s.w), _ptr(self.head),
                                                self.head.numel() * 4, s.stream))
        return grad


def level0_buffers(name, metric, s, t, gb, need_t=True, need_r=False, **kw):
    """ClipBuffers with the workspaces of the level-0 backward passes the caller will make (level0_backward)."""
    lib = nat.lib()
    vb = workspace_bytes(lib.fvvdp_video_grad_workspace, s.W, s.H, s.n_bands, gb) if need_t else 0
    rb = workspace_bytes(lib.fvvdp_ref_grad_workspace, s.W, s.H, s.n_bands, gb, 2) if need_r else 0
    return ClipBuffers(name, metric, s, t, gb, vb, need_t, rb, **kw)


def level0_backward(buf, s, prm, Q, total, b0, nb, gamma, need_t=True, need_r=True):
    """The maps of frames [b0, b0 + nb) in buf (slope planes included, for the reference) and the forward's Q_per_ch [bands, 2,
    total] -> gamma times the gradient of level 0's two planes, into rows [b0, b0 + nb) of buf.g0 (test) / buf.g0_r."""
    lib = nat.lib()
    if need_t:
        nat.check(lib.fvvdp_video_grad_frames(s.W, s.H, s.n_bands, nb, C.byref(prm), C.byref(s.pp), _ptr(Q), total, b0, _ptr(gamma),
                                              buf.maps.maps_arr, _ptr(buf.g0), _ptr(buf.work), buf.work_bytes, s.stream))
    if need_r:
        nat.check(lib.fvvdp_video_ref_grad_frames(s.W, s.H, s.n_bands, nb, C.byref(prm), C.byref(s.pp), _ptr(Q), total, b0,
                                                  _ptr(gamma), buf.maps.maps_arr, buf.maps.slopes, _ptr(buf.g0_r), _ptr(buf.work_r),
                                                  buf.ref_bytes, s.stream))


# ---- parameter vectors (theta, phi, psi) and the entry points that differentiate one ------------------------------------------
def vector_values(arg_name, names, x):
    """x (a 1-D tensor or sequence laid out as the tuple `names` of the fvvdp class, e.g. "PARAMETER_NAMES") -> list of finite
    Python floats; `arg_name` is what the messages call it.  A host tensor is read without touching the GPU."""
    keys = getattr(_fvvdp, names)
    t = x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float64))
    if t.dim() != 1 or t.shape[0] != len(keys):
        raise RuntimeError("%s must be a 1-D vector of the %d parameters of %s, got shape %s"
                           % (arg_name, len(keys), names, tuple(t.shape)))
    if not t.is_floating_point():
        raise RuntimeError("%s must be a float32 or float64 tensor, got %s" % (arg_name, t.dtype))
    vals = [float(v) for v in t.to(device="cpu", dtype=torch.float64).tolist()]
    bad = [keys[i] for i, v in enumerate(vals) if not math.isfinite(v)]
    if bad:
        raise RuntimeError("%s has non-finite entries: %s" % (arg_name, ", ".join(bad)))
    return vals


def _refuse(name, what, metric, test, reference, other, heat_maps=""):
    """Sources that require grad and heat-map metrics: refused by the entry point `name`, which differentiates `what` only."""
    for a in (test, reference):
        if isinstance(a, torch.Tensor) and a.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("%s differentiates the JOD with respect to %s only and this test or reference "
                               "requires grad; detach it (gradients for the images or frames: %s)" % (name, what, other))
    if metric.do_heatmap:
        raise RuntimeError("%s makes no heat maps: build the metric with heatmap=None%s" % (name, heat_maps))


def _apply(function, metric, x, run, *args):
    """function.apply(x, metric, run, *args) when the vector x asks for a gradient; else the forward alone, run(False)[0]."""
    if isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled():
        return function.apply(x, metric, run, *args)
    with torch.cuda.device(metric.device):
        return run(False)[0]
