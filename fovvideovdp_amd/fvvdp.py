"""`class fvvdp`: the reference's public metric API (pyfvvdp/fvvdp.py:58) on top of the MI355X HIP hot path.

What stays in Python (as in the reference): configuration, display models, temporal-filter taps, the collapse of
the CSF look-up table to per-band 1-D tables, frame batching, and the final pooling / JOD regression
(do_pooling_and_jods).  What runs in hand-written HIP kernels (libfvvdp_hip.so, include/fvvdp_hip.h): unpacking +
display photometry + luminance + temporal filtering, the Gaussian/contrast pyramid, CSF weighting, mutual masking
and spatial pooling.  There is no CPU implementation of the hot path in this package: without a GPU or without the
built library `predict*` raises.
"""
import ctypes as C
import json
import logging
import math

import numpy as np
import torch

from . import _native as nat
from . import utils
from .display_model import (code_value_tables, fvvdp_display_geometry, fvvdp_display_photometry, native_eotf,
                            native_geometry)
from .video_source import fvvdp_video_source_array, reshuffle_dims
from .video_source_yuv import fvvdp_video_source_yuv_frames


def _interpolants(x_q, x):
    """Bracketing knots and fraction of the reference's LUT interpolation, incl. its +1e-6 in the denominator."""
    imax = torch.bucketize(x_q, x)
    imax[imax >= x.shape[0]] = x.shape[0] - 1
    imin = (imax - 1).clamp(0, x.shape[0] - 1)
    ifrc = (x_q - x[imin]) / (x[imax] - x[imin] + 0.000001)
    ifrc[imax == imin] = 0.
    ifrc[ifrc < 0.0] = 0.
    return imin, imax, ifrc


_BAND_CACHE = {}


def band_frequencies(W, H, ppd):
    """Number of band-pass levels and their centre frequencies [cpd] for a W x H frame at `ppd` pixels/degree
    (same rule as the reference's pyramid constructor, pyfvvdp/fvvdp_lpyr_dec.py:15-49).  Memoised per (W, H, ppd);
    callers get their own copy of the array."""
    key = (int(W), int(H), float(ppd))
    if key not in _BAND_CACHE:
        if len(_BAND_CACHE) > 256:
            _BAND_CACHE.clear()
        _BAND_CACHE[key] = _band_frequencies(W, H, ppd)
    height, freqs = _BAND_CACHE[key]
    return height, freqs.copy()


def _band_frequencies(W, H, ppd):
    max_levels = int(np.floor(np.log2(min(H, W)))) - 1
    octave = 0.3228 * np.power(2.0, -np.arange(0.0, 14.0))
    bands = np.concatenate([[1.0], octave]) * ppd / 2.0
    too_low = np.nonzero(bands <= 0.5)[0]
    max_band = int(too_low[0]) if too_low.size else max_levels
    height = int(np.clip(max_band + 1, 0, max_levels))
    freqs = np.array([1.0] + [0.3228 * 2.0 ** (-f) for f in range(height)]) * ppd / 2.0
    return height, freqs


def filter_length(fps):
    """Taps of the temporal filters at `fps` frames per second (fvvdp.py:236 of the reference)."""
    return int(np.ceil(250.0 / (1000.0 / fps)))


def temporal_filters(frames_per_s, filter_len, sigma, beta):
    """Sustained (log-Gaussian) and transient (its scaled derivative) temporal filters, fp32 [2, filter_len], for the frame rate,
    filter length, sustained_sigma and sustained_beta given (Python floats): the body of fvvdp.get_temporal_filters
    (fvvdp.py:609-630 of the reference), which calibration_jod_video(temporal=...) evaluates under values of its own."""
    t = torch.linspace(0.0, filter_len / frames_per_s, filter_len)
    F = torch.zeros((2, t.shape[0]))
    sigma = torch.tensor([sigma])
    beta = torch.tensor([beta])
    F[0] = torch.exp(-torch.pow(torch.log(t + 1e-4) - torch.log(beta), 2.0) / (2.0 * (sigma ** 2.0)))
    F[0] = F[0] / torch.sum(F[0])
    k2 = 0.062170507756932
    Fdiff = F[0, 1:] - F[0, :-1]
    F[1] = k2 * torch.cat([Fdiff / (t[1] - t[0]), torch.tensor([0.0])], 0)
    return F


def window_frame_indices(N, fl, temp_padding):
    """Source frame for every virtual time step: fl-1 history entries (temporal padding before frame 0) followed
    by the newest frame of each of the N outputs.  Matches the window the reference builds at frame 0 and then
    slides (pyfvvdp/fvvdp.py:258-291), including `circular` never showing frame 0 at output 0."""
    if temp_padding == "replicate":
        first = [0] * fl
    elif temp_padding == "circular":
        first = [(N - 1 - fl + kk) % N for kk in range(fl)]
    elif temp_padding == "pingpong":
        seq = list(range(0, N)) + list(range(N - 2, 0, -1))
        hist = []
        while len(hist) < (fl - 1):
            hist = hist + seq
        first = (hist[-(fl - 1):] if fl > 1 else []) + [0]
    else:
        raise RuntimeError('Unknown padding method "{}"'.format(temp_padding))
    return np.asarray(first + list(range(1, N)), dtype=np.int32)


def _refuse_grad(a):
    if isinstance(a, torch.Tensor) and a.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("Gradients through the metric are not supported on the HIP path (forward-only kernels); "
                           "detach the inputs or wrap the call in torch.no_grad() (differentiable still images: "
                           "fvvdp.jod_images; differentiable clips: fvvdp.jod_video)")


def _sample_type(dt):
    """torch dtype of the source samples -> (sample type code of the native ingest, bits of an integer code or 0).  float16 and
    bfloat16 samples are read as they are (2 bytes each) and widened exactly in the kernels: every result equals the float32
    path on the upcast input, bit for bit."""
    if dt is torch.uint8:
        return nat.FVVDP_U8, 8
    if dt is torch.int16:
        return nat.FVVDP_U16, 16
    if dt is torch.float32:
        return nat.FVVDP_F32, 0
    if dt is torch.float16:
        return nat.FVVDP_F16, 0
    if dt is torch.bfloat16:
        return nat.FVVDP_BF16, 0
    raise RuntimeError("Only uint8, uint16 and float32 is currently supported")


def _is_float_type(dtype):
    return dtype in (nat.FVVDP_F32, nat.FVVDP_F16, nat.FVVDP_BF16)


def _image_stack(test, reference, dim_order):
    """Stacked image pairs in `dim_order` (a B axis; F absent or of size 1) -> (test, reference) tensors [B, C, H, W] (views
    where possible; numpy uint16 carried as int16 like fvvdp_video_source_array)."""
    if tuple(test.shape) != tuple(reference.shape):
        raise RuntimeError('Test and reference image/video tensors must be exactly the same shape')
    d = dim_order.upper()
    if len(d) != len(test.shape):
        raise RuntimeError('Input tensor much have exactly as many dimensions as there are characters in the "dims" parameter')
    if len(set(d)) != len(d) or set(d) - set("BCFHW") or "H" not in d or "W" not in d:
        raise RuntimeError('dim_order must be made of distinct letters of "BCFHW" and contain H and W, got "%s"' % dim_order)
    if "B" not in d:
        raise RuntimeError('predict_images needs a B axis (the image pairs) in dim_order, got "%s"' % dim_order)
    t = fvvdp_video_source_array._as_tensor(test)
    r = fvvdp_video_source_array._as_tensor(reference)
    if "F" in d:
        if t.shape[d.index("F")] != 1:
            raise RuntimeError("still images only: the F axis must have size 1 (use predict() for video)")
        t, r = t.select(d.index("F"), 0), r.select(d.index("F"), 0)
        d = d.replace("F", "")
    t, r = reshuffle_dims(t, d, "BCHW"), reshuffle_dims(r, d, "BCHW")
    if t.shape[0] < 1:
        raise RuntimeError("no image pairs")
    if t.shape[1] != 1 and t.shape[1] != 3:
        raise RuntimeError('The content must have either 1 or 3 colour channels.')
    return t, r


def _image_pair(test, reference, dim_order):
    """One image pair in `dim_order` (B and F absent or of size 1) -> (test, reference) [C, H, W]."""
    d = dim_order.upper()
    if tuple(test.shape) != tuple(reference.shape):
        raise RuntimeError('Test and reference image/video tensors must be exactly the same shape')
    if "B" not in d:
        test, reference, d = test[None], reference[None], "B" + d
    t, r = _image_stack(test, reference, d)
    if t.shape[0] != 1:
        raise RuntimeError("predict_image_pairs takes one image pair per list entry (B must be 1)")
    return t[0], r[0]


class _Context:
    """Owns one native context (scratch for `batch` frames of a W x H pyramid)."""

    def __init__(self, W, H, height, planes, batch, rho_band, prm):
        self.key = (W, H, height, planes, batch)
        self.handle = C.c_void_p()
        rb = (C.c_double * (height + 1))(*[float(r) for r in rho_band])
        nat.check(nat.lib().fvvdp_ctx_create(C.byref(self.handle), W, H, height, planes, batch, rb, C.byref(prm)))

    def close(self):
        if self.handle:
            nat.lib().fvvdp_ctx_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class fvvdp:
    def __init__(self, display_name="standard_4k", display_photometry=None, display_geometry=None, color_space="sRGB",
                 foveated=False, heatmap=None, quiet=False, device=None, temp_padding="replicate",
                 use_checkpoints=False, batch_frames=None):
        assert heatmap in [None, "none", "raw", "threshold", "supra-threshold"], "Unsupported heatmap type"
        assert temp_padding in ["replicate", "circular", "pingpong"], "Unsupported temporal padding method"
        self.quiet = quiet
        self.foveated = foveated
        self.heatmap = heatmap
        self.color_space = color_space
        self.temp_padding = temp_padding
        self.use_checkpoints = use_checkpoints
        self.do_heatmap = (self.heatmap is not None) and (self.heatmap != "none")
        # use_checkpoints only changes how the reference's autograd graph is stored (fvvdp.py:302-304); the HIP path is
        # forward-only, so the flag is accepted and ignored; asking for gradients is what is refused (predict*)
        if device is None:
            device = torch.device('cuda:0') if (torch.cuda.is_available() and torch.cuda.device_count() > 0) else torch.device('cpu')
        self.device = self._indexed(torch.device(device))
        self.batch_frames = batch_frames
        self._ctx = None
        self._lut_dev = code_value_tables()
        self._chan_w = {}
        self._copy_stream = None
        self._filters = {}
        self.timing = None
        self.set_display_model(display_name, display_photometry=display_photometry, display_geometry=display_geometry)
        self.load_config()
        self.csf_cache_dirs = ["csf_cache"]
        self.omega = [0, 5]
        self.csf_lut = [utils.load_csf_lut(om, self.csf_sigma, self.k_cm, self.csf_cache_dirs) for om in self.omega]

    # ---- configuration ------------------------------------------------------------------------------------
    @staticmethod
    def _indexed(device):
        """'cuda' -> 'cuda:<current index>': tensors report an indexed device, comparisons against a bare 'cuda' are never equal
        (resident arrays were counted as uploads and copied device-to-device)."""
        if device.type == "cuda" and device.index is None and torch.cuda.is_available():
            return torch.device("cuda", torch.cuda.current_device())
        return device

    def update_device(self, device):
        self.device = self._indexed(torch.device(device))
        if self._ctx is not None:
            self._ctx.close()
        self._ctx = None
        self._lut_dev.clear()
        self._chan_w = {}
        self._copy_stream = None

    def _drop_context(self):
        """Everything baked into the native context at creation (band frequencies, CSF tables, model constants,
        geometry maps) is stale once the display or the parameters change: the next call builds a fresh one."""
        if self._ctx is not None:
            self._ctx.close()
        self._ctx = None
        self._chan_w = {}                # [1, w_transient] of do_pooling_and_jods: a model parameter like the rest

    def load_config(self):
        parameters = utils.config_files.load("fvvdp_parameters.json")
        self.parameters_file = utils.config_files.find("fvvdp_parameters.json")
        for name in ("mask_p", "mask_c", "pu_dilate", "w_transient", "beta", "beta_t", "beta_tch", "beta_sch",
                     "sustained_sigma", "sustained_beta", "csf_sigma", "sensitivity_correction", "masking_model",
                     "local_adapt", "contrast", "jod_a", "log_jod_exp", "mask_q_sust", "mask_q_trans", "k_cm",
                     "filter_len", "version"):
            setattr(self, name, parameters[name])
        if (self.local_adapt != "gpyr" or self.contrast != "weber" or self.pu_dilate != 0 or
                self.masking_model != "min_mutual_masking_perc_norm2"):
            raise RuntimeError("Only the shipped model variant (local_adapt=gpyr, contrast=weber, pu_dilate=0, "
                               "min_mutual_masking_perc_norm2) is implemented by the HIP path")
        self.debug = False
        self._drop_context()

    def set_display_model(self, display_name="standard_4k", display_photometry=None, display_geometry=None):
        if display_photometry is None:
            self.display_photometry = fvvdp_display_photometry.load(display_name)
            self.display_name = display_name
        else:
            self.display_photometry = display_photometry
            self.display_name = "unspecified"
        if display_geometry is None:
            self.display_geometry = fvvdp_display_geometry.load(display_name)
        else:
            self.display_geometry = display_geometry
        self.pix_per_deg = self.display_geometry.get_ppd()
        self._drop_context()
        self._lut_dev.clear()

    # ---- public prediction API ------------------------------------------------------------------------------
    def predict(self, test_cont, reference_cont, dim_order="BCFHW", frames_per_second=0, fixation_point=None, sync=True):
        vs = fvvdp_video_source_array(test_cont, reference_cont, frames_per_second, dim_order=dim_order,
                                      display_photometry=self.display_photometry, color_space_name=self.color_space)
        return self.predict_video_source(vs, fixation_point=fixation_point, sync=sync)

    def predict_video_source(self, vid_source, fixation_point=None, frame_range=None, pool=True, sync=True):
        """Returns (Q_JOD 0-d tensor on the compute device, stats dict).

        Extensions (not in the reference):
        `frame_range=(f0, f1)` (frame sharding across GPUs) evaluates only output frames [f0, f1); the temporal
        window of frame f0 is still filled from the frames before it.  With `pool=False` the JOD regression is skipped
        and Q_JOD is None (the caller pools after combining shards).
        `sync=False` queues the whole call on the current stream and returns without waiting for the GPU:
        `stats['Q_per_ch']` is then a DEVICE tensor [bands, 2, frames] (not numpy) and the out-of-range flag is left in
        `stats['range_flag']` (int32 device tensor; `fvvdp.finish(stats)` converts both and emits the warning);
        `stats['result_buffer']` is the flat device buffer behind them (Q_per_ch | flag | JOD), the row a multi-GPU caller
        all-reduces.  Many
        pairs can be queued back to back this way (one per call); the context's scratch is reused in stream order.
        """
        if self.device.type != "cuda":
            raise RuntimeError("fovvideovdp_amd needs an AMD GPU (torch device 'cuda'); there is no CPU fallback")
        for name in ("test_video", "reference_video"):
            t = getattr(vid_source, name, None)
            if isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled():
                raise RuntimeError("Gradients through the metric are not supported on the HIP path (forward-only kernels); "
                                   "detach the inputs or wrap the call in torch.no_grad()")
        with torch.cuda.device(self.device):       # the library launches on the calling thread's current device
            return self._predict_on_device(vid_source, fixation_point, frame_range, pool, sync)

    def predict_batch(self, pairs, dim_order="BCFHW", frames_per_second=0, fixation_point=None):
        """Extension (BASELINE configs[4]: many independent pairs per GPU): queues every (test, reference) pair of `pairs` on the
        caller's stream without host synchronisation (the context's scratch is reused in stream order).  Returns
        [(Q_JOD, stats)] as `predict(..., sync=False)` does: `stats['Q_per_ch']` are device tensors, `fvvdp.finish(stats)`
        brings one to the host."""
        return [self.predict(t, r, dim_order=dim_order, frames_per_second=frames_per_second, fixation_point=fixation_point,
                             sync=False) for (t, r) in pairs]

    # ---- batched still images (extension; include/fvvdp_hip_images.h) ------------------------------------------------
    def predict_images(self, test, reference, dim_order="BCHW", fixation_point=None, sync=True):
        """Extension: scores B still-image pairs in one pass.  `test` and `reference` are stacked arrays or tensors (host or
        device) whose `dim_order` has a B axis and no F axis (or F == 1).  Returns (Q_JOD, stats): Q_JOD a [B] device tensor,
        stats['Q_per_ch'] [B, bands, 2, 1] (numpy; with `sync=False` a device tensor that `fvvdp.finish(stats)` completes),
        stats['range_flags'] one out-of-range flag per pair, stats['heatmap'] [B, ch, 1, H, W] fp16 when the metric makes heat
        maps.  `fixation_point`: [x, y] or [B, 2] for a foveated metric.  Pair k's result does not depend on the batch."""
        self._check_device()
        _refuse_grad(test)
        _refuse_grad(reference)
        t, r = _image_stack(test, reference, dim_order)
        B = t.shape[0]
        # the whole stack on the device once, as contiguous [B][C][H][W] (no copy for a resident contiguous stack)
        self.last_h2d_bytes = sum(a.numel() * a.element_size() for a in (t, r) if a.device != self.device)
        if t.dtype != r.dtype:
            t, r = self._to_unit_float(t), self._to_unit_float(r)
        t, r = t.to(self.device).contiguous(), r.to(self.device).contiguous()
        fix = None
        if self.foveated:
            fix = self._fixation(fixation_point, t.shape[3], t.shape[2], B)
        with torch.cuda.device(self.device):
            return self._predict_image_group([t[k] for k in range(B)], [r[k] for k in range(B)], fix, sync)

    def jod_images(self, test, reference, dim_order="BCHW", fixation_point=None, wrt="test"):
        """Extension: the JOD of B still-image pairs as a differentiable [B] fp32 tensor on the metric's device, for losses
        such as `10 - metric.jod_images(x, ref)`.  Values are bit-identical to predict_images(test.detach(), reference, ...)[0].
        When `test` requires grad (and grad mode is on), backward() puts dJOD_k/dtest_k into `test`, whatever its layout or
        device; the reference is a constant (a reference that requires grad is refused).  float32, float16 or bfloat16 samples
        (see below), behind a display model with a closed form (sRGB, gamma, PQ, linear, absolute); samples the display model clamps (outside
        [0, 1], or beyond a luminance clip) get a zero gradient.  Foveated metrics take `fixation_point` as predict_images.
        Nothing is synchronised with the host (a user geometry model's gaze conversion aside): the out-of-range warning of predict_images is not issued and no heat maps are
        made, whatever `heatmap` the metric was built with.  Double backward is not supported.  The backward re-runs the
        forward with per-band maps in batches of up to `self.grad_batch` pairs (None: as many as about 4 GB of maps allow).
        `wrt` names the input(s) the gradient is taken for.  "test" (default): as above.  "reference": backward() puts
        dJOD_k/dreference_k into `reference` (any layout or device, as `test` above), `test` is a constant and one that requires
        grad is refused.  "both": one backward delivers both gradients to whichever of the two inputs require grad, from one
        re-ingest and one map-writing pass; the test gradient is bit-identical to wrt="test".  Anything else: ValueError.  The
        reference gradient covers its own band contrast, its role as the adaptation luminance L_bkg and, through L_bkg, the
        CSF look-up (the slope of the LUT's interpolation); reference samples the display model clamps get zeros.
        Half precision: `test` and `reference` may both be float16 or both bfloat16 (what a network under torch.autocast
        emits).  The kernels read the 2-byte samples as they are and widen them exactly, so the JOD (fp32) equals the float32
        path on the upcast input bit for bit; the half tensors are what is saved for backward; and the gradient comes back in
        the dtype of the input -- the float32 gradient rounded once, to nearest even -- so it reaches a half-precision leaf or an
        autocast graph without a cast.  A mixed pair (a half test with a float32 reference, or the reverse): the narrower side
        is upcast with torch's .float() inside autograd's view, the float32 kernels run, and the gradient arrives in the
        caller's dtype through torch's own cast node.  float16 gradients of a JOD are small (most of them below the smallest
        normal float16, 6.1e-5, for a large image): scale the loss as torch.amp.GradScaler does -- the incoming grad_output
        multiplies in fp32 before the one rounding, so the scale is not lost.  bfloat16 has float32's exponent range and needs
        no scaling.  float64 is refused."""
        from .image_grad import jod_images
        return jod_images(self, test, reference, dim_order, fixation_point, wrt)

    def jod_video(self, test, reference, dim_order="BCFHW", frames_per_second=0, fixation_point=None, wrt="test"):
        """Extension: the JOD of one clip as a differentiable 0-d fp32 tensor on the metric's device, for losses such as
        `10 - metric.jod_video(x, ref, frames_per_second=30)`.  The value is bit-identical to
        predict(test.detach(), reference, dim_order, frames_per_second, fixation_point)[0].  When `test` requires grad (and grad
        mode is on), backward() puts dJOD/dtest into `test`, whatever its layout or device; the reference is a constant (a
        reference that requires grad is refused).  float32, float16 or bfloat16 samples (half precision and mixed pairs: as
        jod_images describes them) behind a display model with a closed form (sRGB, gamma, PQ, linear, absolute), C = 1 or 3, one clip (B = 1) of at least 2 frames (a single frame: jod_images), every temporal
        padding, frame rates of up to 256 per second (a temporal filter of up to 64 taps), foveated or not (`fixation_point`
        as predict takes it).  Samples the display model clamps get a zero gradient, and so does a frame that no temporal
        window shows (`circular` padding of a clip more than one frame longer than the filter: frame 0).  Nothing is
        synchronised with the host (a user geometry model's gaze conversion aside): no out-of-range warning, no heat maps.
        Double backward is not supported.
        The backward re-runs the forward with per-band maps in batches of up to `self.grad_batch` frames (None: as many as
        about 4 GB of maps allow); the gradient does not depend on the batching, bit for bit.
        `wrt` as jod_images takes it: "test" (default), "reference" (dJOD/dreference into `reference`; `test` is a constant
        and one that requires grad is refused) or "both" (one backward, both gradients, one re-ingest and one map-writing
        pass per backward batch; the test gradient is bit-identical to wrt="test").  The reference side accepts what the test
        side accepts; a frame no temporal window shows gets zeros there too."""
        from .video_grad import jod_video
        return jod_video(self, test, reference, dim_order, frames_per_second, fixation_point, wrt)

    def jod_video_yuv(self, test, reference, frames_per_second=0, width=None, height=None, bit_depth=8, chroma_ss="420",
                      color_space="bt709", fixation_point=None, full_screen_resize=None):
        """Extension: jod_video for a clip of planar YUV, as a learned codec, in-loop filter or post-filter produces it, for
        losses such as `10 - metric.jod_video_yuv((Y, U, V), ref, frames_per_second=30)`.  `test` and `reference`: a tuple
        (Y, U, V) of float32 tensors -- Y [N, H, W]; U, V [N, H/2, W/2] for chroma_ss="420", [N, H, W] for "444" -- or one packed
        float32 tensor [N, H*W + 2*uvh*uvw] with the layout of fvvdp_video_source_yuv_frames together with width= and height=
        (read as three views of itself: no copy).  The samples are limited-range CODE VALUES on the scale of `bit_depth` (Y
        nominally in [16, 235] * 2^(bit_depth - 8)), fractions allowed: the arithmetic is the integer source's with the sample in
        the place of (float)code, so a normalised range is the caller's one multiply.  The reference may also be the integer
        codes that source class takes (converted once, exactly); it is a constant, and one that requires grad is refused.
        Returns the JOD as a 0-d fp32 tensor on the metric's device; when a test plane requires grad, backward() puts dJOD/dY,
        dJOD/dU, dJOD/dV into the caller's tensors (or the packed one), on host or device.  The unpack -- the two clamps,
        bilinear x2 chroma for 4:2:0, the `color_space` matrix ("bt709" or "bt2020nc", with the luminance weights of sRGB or
        BT.2020), the clip to [0, 1] -- runs inside the ingest kernel and its adjoint in one gather kernel: no RGB clip exists
        at any point.  A sample gets an exact zero gradient where a clamp binds (Y or chroma outside its range, an RGB value
        clipped), and so does a frame no temporal window shows.  Accepted: the metric's display model when it has a closed form
        (sRGB, gamma, PQ, linear, absolute), every temporal padding, foveated or not (`fixation_point` as predict takes it),
        N >= 2, temporal filters of up to 32 taps (120 frames per second have 30).  Refused, each with a sentence: longer
        filters, half-precision or float64 planes, 4:2:0 with odd width or height, full_screen_resize, a look-up-table or user
        photometry, shapes that do not match, 4:2:2.  Double backward is not supported.  The value does not depend on whether
        grad is on, the gradient not on `self.grad_batch`, and both repeat bit for bit."""
        from .yuv_grad import jod_video_yuv
        return jod_video_yuv(self, test, reference, frames_per_second, width, height, bit_depth, chroma_ss, color_space,
                             fixation_point, full_screen_resize)

    def predict_resized(self, test, reference, full_screen_resize="bilinear", resize_resolution=None, dim_order="BCFHW",
                        frames_per_second=30, fixation_point=None, test_frames=1, reference_frames=1):
        """Extension: predict for a test and a reference clip that each have a frame size of their OWN -- a bitrate-ladder rung,
        a render-resolution sweep or a super-resolution output shown full screen.  Both clips have the same frame and channel
        counts (C = 1 or 3) and are float32, or uint8 scaled by 1/255, on host or device, in any `dim_order` predict takes.
        `resize_resolution=(width, height)` is the size the metric judges at (default: the display geometry's resolution).  A
        stream of another size is resized inside the ingest kernel with the arithmetic of torch.nn.functional.interpolate
        (`full_screen_resize`: "bilinear", "bicubic", "nearest" or "area"; align_corners=False, no antialiasing); a stream that
        has the target size is read as it is.  Per stream and target pixel: interpolate every channel, clip to [0, 1] (the clip
        belongs to the resize, as in the reference's reader: no out-of-range warning), display model, luminance.  No clip at the
        target size is stored.  Returns (Q_JOD, stats) as predict does, stats at the target size.  When both clips already have
        the target size the call is predict's, unchanged.  Accepted: closed-form display models (sRGB, gamma, PQ, linear,
        absolute), every temporal padding, foveated or not (`fixation_point` in target pixels), clips of at least 2 frames,
        temporal filters of up to 32 taps (120 frames per second).  Refused, each with a sentence and before any device work: an
        unknown mode, half-precision, float64 or 16-bit samples, a look-up-table or user photometry, differing frame or channel
        counts, longer filters, single images.
        `test_frames` / `reference_frames` (predict_held's keywords, with predict_held's meaning: an int k -- display frame v
        shows frame v // k -- or a non-decreasing integer sequence with one entry per display frame) give each stream a frame
        COUNT of its own as well: a rung at half the resolution AND half the rate.  The result equals predict_resized on
        test.index_select(frames, m_t) and reference.index_select(frames, m_r) bit for bit (JOD and Q_per_ch), no expanded clip
        is made, and a held frame is interpolated and sent through the display model once.  `frames_per_second`, the temporal
        padding and `fixation_point` then refer to display frames, and stats['N_frames'] is their count (at least 2; a stream
        may have a single frame).  Map errors are predict_held's ValueErrors.  Left at 1, or with identity maps on equal frame
        counts, the call is the one described above; non-trivial maps on two clips of the target size are predict_held's."""
        from .resize_grad import predict_resized
        return predict_resized(self, test, reference, full_screen_resize, resize_resolution, dim_order, frames_per_second,
                               fixation_point, test_frames, reference_frames)

    def jod_video_resized(self, test, reference, full_screen_resize="bilinear", resize_resolution=None, dim_order="BCFHW",
                          frames_per_second=30, fixation_point=None, test_frames=1, reference_frames=1):
        """Extension: jod_video for clips with frame sizes of their own (see predict_resized for the resize), for losses such as
        `10 - metric.jod_video_resized(net(x_small), ref_full, frames_per_second=30)`.  Returns the JOD as a 0-d fp32 tensor on the
        metric's device; under torch.no_grad() it equals predict_resized's bit for bit.  When `test` (float32) requires grad,
        backward() puts dJOD/dtest into the caller's tensor AT THE TEST'S OWN RESOLUTION, on host or device, whatever its layout:
        the adjoint of the resize is one gather per test sample in a fixed order (no atomics), so the gradient does not depend on
        `self.grad_batch` and repeats bit for bit.  A sample gets an exact zero where every target pixel it reaches is clipped or
        clamped by the display model, where a downscale skips it, and in a frame no temporal window shows.  The reference (float32
        or uint8) is a constant; one that requires grad is refused.  When both clips already have the target size the call is
        jod_video's.  Double backward is not supported.
        `test_frames` / `reference_frames`: as predict_resized takes them, for losses such as
        `10 - metric.jod_video_resized(net(x_540p30), ref_2160p60, frames_per_second=60, test_frames=2)`.  The JOD has
        predict_resized's bits, and backward() puts the adjoint of exactly that function -- hold, resize, clip -- into the
        caller's tensor at the test's own resolution AND own frame count: the luminance gradient is summed over the display
        frames that show a source frame (ascending, no atomics) before the resize's adjoint runs once per source frame.  A
        frame no display frame shows gets exact zeros."""
        from .resize_grad import jod_video_resized
        return jod_video_resized(self, test, reference, full_screen_resize, resize_resolution, dim_order, frames_per_second,
                                 fixation_point, test_frames, reference_frames)

    def predict_images_resized(self, test, reference, full_screen_resize="bilinear", resize_resolution=None, dim_order="BCHW",
                               fixation_point=None):
        """Extension: predict_images for a test and a reference stack that each have an image size of their OWN -- the outputs
        of a super-resolution or down-scaling network, a render-resolution sweep of stills, images shown full screen.  `test` is
        [B, C, h, w] and `reference` [B, C, h', w'] in `dim_order` (a B axis; no F axis, or F == 1), the same B and C (C = 1 or
        3), each float32, or uint8 scaled by 1/255, on host or device, in any layout.  `resize_resolution=(width, height)` is the
        size the metric judges at (default: the display geometry's resolution).  A stack of another size is resized inside the
        ingest kernel with the arithmetic of torch.nn.functional.interpolate (`full_screen_resize`: "bilinear", "bicubic",
        "nearest" or "area"; align_corners=False, no antialiasing); a stack that has the target size is read as it is, and
        clipped like the other.  Per stack and target pixel: interpolate every channel, clip to [0, 1] (the clip belongs to the
        resize: no range flags), display model, luminance.  No image at the target size is stored.  Returns (Q_JOD, stats):
        Q_JOD a [B] device tensor, stats['Q_per_ch'] [B, bands, 2, 1] (numpy), stats['rho_band'], 'width' and 'height' at the
        target size; no heat maps, whatever `heatmap` the metric has.  `fixation_point`: [x, y] or [B, 2] in target pixels for
        a foveated metric.  Pair k's result does not depend on the batch, bit for bit.  When both stacks already have the target
        size the call is predict_images's, unchanged.  Refused, each with a sentence and before any device work: an unknown
        mode, half-precision, float64 or 16-bit samples, a look-up-table or user photometry, differing B or C, an F axis longer
        than 1 (clips: predict_resized), a width or height outside 1 .. 32768, inputs that require grad."""
        from .images_resize import predict_images_resized
        return predict_images_resized(self, test, reference, full_screen_resize, resize_resolution, dim_order, fixation_point)

    def jod_images_resized(self, test, reference, full_screen_resize="bilinear", resize_resolution=None, dim_order="BCHW",
                           fixation_point=None, wrt="test"):
        """Extension: jod_images for stacks with image sizes of their own (see predict_images_resized for the resize), for losses
        such as `10 - metric.jod_images_resized(net(x_small), ref_full).mean()`.  Returns [B] fp32 JODs on the metric's device;
        under torch.no_grad() they equal predict_images_resized's bit for bit.  `wrt` as jod_images takes it.  "test" (default):
        backward() puts grad[k] dJOD_k/dtest_k into the caller's `test` AT THE TEST'S OWN RESOLUTION, on host or device, whatever
        its layout; the reference is a constant, and one that requires grad is refused.  "reference": the gradient goes into
        `reference` at the reference's own resolution, and a test that requires grad is refused.  "both": one backward -- one
        re-ingest and one map-writing pass per backward batch -- delivers both gradients to whichever of the two require grad;
        the test gradient is bit-identical to wrt="test".  Anything else: ValueError.  A differentiated side is float32; a
        float16 or bfloat16 tensor is upcast with torch's .float() inside autograd's view, so the gradient arrives in the
        caller's dtype through torch's cast node (there are no half-precision kernels here); the constant side may be uint8.
        The adjoint of the resize is one gather per sample in a fixed order (no atomics): the gradient does not depend on
        `self.grad_batch`, on placement or on layout, and repeats bit for bit.  A sample gets an exact zero where every target
        pixel it reaches is clipped or clamped by the display model, and where a downscale skips it; an identical pair resized
        identically gives JOD == 10 and exact zeros.  When both stacks already have the target size the call is jod_images's.
        Double backward is not supported."""
        from .images_resize import jod_images_resized
        return jod_images_resized(self, test, reference, full_screen_resize, resize_resolution, dim_order, fixation_point, wrt)

    def predict_image_pairs_resized(self, pairs, full_screen_resize="bilinear", resize_resolution=None, dim_order="HWC",
                                    fixation_points=None):
        """Extension: predict_image_pairs for a list of (test, reference) whose two images may each have any size: a folder of
        images of mixed sizes scored full screen.  The pairs are grouped by (test size, reference size, dtypes, C) and every
        group is one predict_images_resized pass.  Returns [(Q_JOD, stats)] in input order, Q_JOD 0-d and Q_per_ch [bands, 2, 1];
        row k equals the call on pair k alone, bit for bit.  `fixation_points`: None, or one [x, y] (or None) per pair in target
        pixels.  Forward only."""
        from .images_resize import predict_image_pairs_resized
        return predict_image_pairs_resized(self, pairs, full_screen_resize, resize_resolution, dim_order, fixation_points)

    def predict_held(self, test, reference, dim_order="BCFHW", frames_per_second=0, fixation_point=None, test_frames=1,
                     reference_frames=1):
        """Extension: predict for a test and a reference clip that each have a frame COUNT of their own -- a 30 fps encode on a
        120 Hz panel, a 40 fps render against a 120 fps ground truth, 24 fps film with 3:2 pulldown, a ladder rung at half the
        frame rate.  Each stream is shown by sample-and-hold through a frame map: `test_frames` / `reference_frames` is an int
        k >= 1 (display frame v shows frame v // k) or a 1-D integer sequence, array or tensor m of one entry per display frame
        (display frame v shows frame m[v]; non-decreasing, inside the stream; a repeat holds the frame, a skipped frame is never
        shown and has no influence).  Both maps must lead to one number N >= 2 of display frames (else ValueError, naming both
        counts).  `frames_per_second` is the rate of the N display frames; the taps, the temporal padding and `fixation_point`
        ([x, y] or [N, 2]) refer to display frames.  The result equals
        predict(test.index_select(frames, m_t), reference.index_select(frames, m_r), ...) bit for bit (JOD and Q_per_ch), and
        no expanded clip is ever made: the ingest reads each stream through its map, a dense planar device clip in place.
        Accepted: every array sample type predict takes (uint8, uint16, float32, float16, bfloat16; a mixed pair is unpacked
        to float32 first), C = 1 or 3, host or device, any `dim_order`, foveated or not, every temporal padding,
        `batch_frames=`, display rates of up to 128 frames per second (32 taps).  Refused, each with a sentence and before any
        device work: a float, decreasing, out-of-range or wrong-length map, k < 1, N < 2, longer filters, a heat-map metric,
        video source objects (and with them frame sharding), float samples behind a user photometry class.  When both maps
        are the identity the call is predict's, unchanged."""
        from .held import predict_held
        return predict_held(self, test, reference, dim_order, frames_per_second, fixation_point, test_frames, reference_frames)

    def jod_video_held(self, test, reference, dim_order="BCFHW", frames_per_second=0, fixation_point=None, test_frames=1,
                       reference_frames=1, wrt="test"):
        """Extension: jod_video for clips with frame counts of their own (see predict_held for the frame maps), for losses such
        as `10 - metric.jod_video_held(net(x15), ref60, frames_per_second=60, test_frames=4)`.  Returns the JOD as a 0-d fp32
        tensor on the metric's device, bit-identical to predict_held's.  backward() puts dJOD/dtest into the caller's tensor AT
        THE TEST'S OWN FRAME COUNT: the adjoint of index_select along the frames runs inside the last kernel of the backward
        (a fixed sum per source frame over the display frames that show it, no atomics), so no gradient at the display's rate
        exists, the result does not depend on `self.grad_batch` and repeats bit for bit.  A frame no display frame shows gets
        exact zeros.  Accepted: what jod_video accepts (float32 / float16 / bfloat16 with the gradient in the dtype of the
        input, closed-form display models, wrt="test" | "reference" | "both", every padding, foveated or not), display rates
        of up to 128 frames per second.  The tensors saved for backward are the source clips.  When both maps are the
        identity the call is jod_video's."""
        from .held import jod_video_held
        return jod_video_held(self, test, reference, dim_order, frames_per_second, fixation_point, test_frames, reference_frames,
                              wrt)

    def diff_map_images(self, test, reference, dim_order="BCHW", fixation_point=None, units="jod"):
        """Extension: the difference maps of B still-image pairs as a differentiable [B, H, W] fp32 tensor on the metric's
        device, for per-pixel losses such as `(mask * metric.diff_map_images(x, ref)).sum()`, a worst-pixel or top-k loss, or a
        saliency-weighted one.  units="jod": the reference's raw difference map before its float16 rounding,
        v_0^beta_jod |jod_a| with v_0 the map the bands add up in; rounded with .to(torch.float16) it equals stats['heatmap'] of
        predict_images on a metric built with heatmap="raw", bit for bit, whatever the batch.  units="linear": v_0 itself, with
        no power and no |jod_a|.  beta_jod = 10^log_jod_exp is about 0.59 < 1, so the derivative of the JOD-unit map grows
        without bound as the map goes to 0: a loss on nearly invisible regions wants the well-conditioned linear form.
        Anything else: ValueError.
        When `test` requires grad (and grad mode is on) the result has a grad_fn, and backward() with a cotangent G of the
        result's shape -- whatever torch expression stands on the map -- puts sum_px G dmap/dtest into `test`, whatever its
        layout or device.  The reference is a constant (one that requires grad is refused: detach it).  Sources, display models,
        half precision and mixed pairs as jod_images takes them, the gradient in the dtype of `test`; `fixation_point` as
        predict_images.  A gradient entry is 0 where jod_images' is (a band pixel with D == 0, the d_max clamp, the contrast
        clamp, samples the display model clamps) and, for units="jod", where v_0 == 0 (an identical pair; the plain chain rule
        gives inf * 0 there): the result is finite for finite inputs and a finite cotangent.  Works whatever `heatmap` the
        metric was built with, makes no coloured maps and does not synchronise with the host.  Double backward is not
        supported.  The backward re-runs the forward with per-band maps in batches of up to `self.grad_batch` pairs; a pair's
        gradient does not depend on the batching, bit for bit."""
        from .map_grad import diff_map_images
        return diff_map_images(self, test, reference, dim_order, fixation_point, units)

    def diff_map_video(self, test, reference, dim_order="BCFHW", frames_per_second=0, fixation_point=None, units="jod"):
        """Extension: the difference maps of one clip as a differentiable [N, H, W] fp32 tensor on the metric's device; as
        diff_map_images, with predict in the place of predict_images (rounded to float16 the units="jod" map equals
        stats['heatmap'][0, 0] of predict on a heatmap="raw" metric, bit for bit, whatever `batch_frames`) and what jod_video
        accepts: one clip (B = 1) of at least 2 frames, C = 1 or 3, float32 / float16 / bfloat16, closed-form display models,
        foveated or not, every temporal padding, temporal filters of up to 64 taps.  units="linear" is the map before the power
        and |jod_a|; its gradient stays bounded where the JOD-unit map's does not (see diff_map_images).  backward() takes a
        cotangent [N, H, W] and puts sum_px G dmap/dtest into `test`.  The backward batches like jod_video's
        (`self.grad_batch`, the same check against the free device memory) and does not depend on the batching, bit for bit."""
        from .map_grad import diff_map_video
        return diff_map_video(self, test, reference, dim_order, frames_per_second, fixation_point, units)

    def predict_gazes(self, test, reference, fixation_points, dim_order="BCFHW", frames_per_second=0):
        """Extension: one (test, reference) clip or image scored under G gaze traces in one pass (foveated metric, stock
        display geometry).  `fixation_points`: [G, 2] (one fixed gaze per row) or [G, N_frames, 2] (one trace per gaze), in
        frame pixels as predict's `fixation_point`.  Returns (Q_JOD, stats): Q_JOD a [G] fp32 device tensor,
        stats['Q_per_ch'] [G, bands, 2, frames] (numpy), the other keys as predict makes them.  Row g is bit-identical to
        predict(test, reference, dim_order, frames_per_second, fixation_point=fixation_points[g]) on this metric, whatever
        the other gazes are: the temporal channels are made once per batch of frames and the pyramid pass evaluates what
        does not depend on the gaze once per group of up to 8 gazes (include/fvvdp_hip_gaze.h).  Every source predict
        accepts (uint8 / uint16 / float32 / float16 / bfloat16, C = 1 or 3, a single frame, batch_frames shorter than the clip).  Refused: a metric
        that is not foveated or makes heat maps, a user display_geometry class, inputs that require grad.  A band whose slice
        of the CSF table does not fit the LDS (every band of standard_hmd or htc_vive_pro, band 0 of a 2160-row frame on
        sdr_4k_30) runs the single-gaze kernel once per gaze: same results, only the temporal channels are shared."""
        from .gazes import predict_gazes
        return predict_gazes(self, test, reference, fixation_points, dim_order, frames_per_second)

    def predict_tests(self, tests, reference, dim_order="BCFHW", frames_per_second=0, fixation_point=None):
        """Extension: T test clips scored against ONE reference in one pass -- a bitrate ladder, one source through several
        codecs or presets, a rendering-quality sweep.  `tests`: a list or tuple of T >= 1 clips, each with the shape, dtype and
        `dim_order` of `reference`.  Returns (Q_JOD, stats): Q_JOD a [T] fp32 device tensor, stats['Q_per_ch']
        [T, bands, 2, frames] (numpy), the other keys as predict makes them.  Row k is bit-identical to
        predict(tests[k], reference, dim_order, frames_per_second) on this metric, whatever the other tests are, however many
        there are, whatever `batch_frames` is and at every frame size.  The reference is ingested and its level 0 written once per pair of tests
        instead of once per test, and the pyramid pass evaluates what depends on the reference only (its own pyramid, L_bkg,
        the CSF look-up) once per group of up to five tests (include/fvvdp_hip_tests.h).  Every array source predict accepts
        (uint8 / uint16 / float32 / float16 / bfloat16, C = 1 or 3, every temporal padding, code-value tables and user
        photometry on integer input, batch_frames shorter than the clip), clips of at least 2 frames.  The out-of-range
        warning is issued once per call.  Refused, each with a sentence: a foveated metric or a `fixation_point` (loop
        predict), a metric that makes heat maps, a single frame (predict_images with the reference repeated), tests whose
        shape or dtype differs from the reference's, inputs that require grad, fvvdp_video_source objects and YUV frame
        sources.  Scratch: ceil((T + 1) / 2) x predict's; beyond `self.tests_scratch_bytes` (None: 96 GB or 40 % of the device)
        the tests are taken in several passes, each with the reference -- same results."""
        from .multitest import predict_tests
        return predict_tests(self, tests, reference, dim_order, frames_per_second, fixation_point)

    def predict_tests_foveated(self, tests, reference, dim_order="BCFHW", frames_per_second=0, fixation_point=None):
        """Extension: predict_tests for a foveated metric -- T foveated variants of ONE reference under the same gaze trace in
        one pass: a foveated renderer at several shading rates, a foveated codec at several bitrates.  `tests` as predict_tests
        takes them; `fixation_point`: None (the centre), [x, y] or [N_frames, 2] in frame pixels, as predict takes it.  Returns
        (Q_JOD, stats): Q_JOD a [T] fp32 device tensor, stats['Q_per_ch'] [T, bands, 2, frames] (numpy), the other keys as predict
        makes them, and stats['shared_pass'].  Row k is bit-identical to
        predict(tests[k], reference, dim_order, frames_per_second, fixation_point=fixation_point) on this metric, whatever the
        other tests are, however many there are and in whatever order, whatever `batch_frames` is.  The ingest is predict_tests'
        (the reference once per pair of tests); the pyramid pass evaluates what depends on the reference and the gaze only
        (its own pyramid, L_bkg, the eccentricity, the cell of the CSF table and its 3-D interpolation) once per group of up to
        five tests (include/fvvdp_hip_tests_fov.h).  Accepted: what predict_tests accepts (uint8 / uint16 / float32 / float16 /
        bfloat16 arrays, C = 1 or 3, host or device, any `dim_order`, every temporal padding, passes under
        `self.tests_scratch_bytes`); one out-of-range warning per call.  Refused, each with a sentence and before any device
        work: a metric that is not foveated (predict_tests), a heat-map metric, a user display_geometry class, source objects and
        YUV frame sources, a single frame, tests whose shape or dtype differs from the reference's, inputs that require grad, a
        `fixation_point` of another shape, float input behind a user photometry class.  Coverage: the shared pass needs every
        band's slice of the CSF table in the LDS (stats['shared_pass'] True).  Where a band's does not fit (every band of
        standard_hmd or htc_vive_pro, band 0 of a 2160-row frame on sdr_4k_30) the whole call is the loop of
        predict(..., sync=False) with one host synchronisation: same bits, no gain, stats['shared_pass'] False."""
        from .tests_fov import predict_tests_foveated
        return predict_tests_foveated(self, tests, reference, dim_order, frames_per_second, fixation_point)

    def jod_gazes(self, test, reference, fixation_points, dim_order="BCFHW", frames_per_second=0):
        """Extension: the JODs of one clip under G gaze traces as a differentiable [G] fp32 tensor on the metric's device, for
        losses over a gaze distribution such as `(10 - metric.jod_gazes(x, ref, grid, frames_per_second=30)).mean()` or the
        worst case over a fixation grid.  `fixation_points` as predict_gazes takes them: [G, 2] or [G, N_frames, 2] in frame
        pixels.  Row g is bit-identical to predict_gazes(test.detach(), reference, fixation_points, ...)[0][g], and so to
        predict(..., fixation_point=fixation_points[g]).  backward() puts sum_g grad[g] dJOD_g/dtest into `test`, whatever its
        layout or device; the reference and the gazes are constants.  The backward shares among the gazes whatever does not
        depend on the gaze -- the ingest, the map-writing pyramid pass, the coarse-to-fine sweep, level 0 and the temporal
        transpose run once per backward batch or clip, only the pooling coefficients and the pointwise layer gradient once
        per gaze (include/fvvdp_hip_gaze_grad.h) -- and its memory does not grow with G.  Accepted: what jod_video accepts
        (float32, float16 or bfloat16 samples -- half precision and mixed pairs as jod_images describes them, the gradient in
        the dtype of `test` --, C = 1 or 3, one clip of at least 2 frames, closed-form display models, every temporal padding,
        filters of up to 64 taps).  Refused: what predict_gazes refuses (a metric that is not foveated or makes heat maps,
        a user display_geometry class).  Nothing is synchronised with the host: no out-of-range warning.  Double backward
        is not supported.  The gradient does not depend on `self.grad_batch` nor on the grouping of the gazes, bit for bit."""
        from .gaze_grad import jod_gazes
        return jod_gazes(self, test, reference, fixation_points, dim_order, frames_per_second)

    def jod_tests(self, tests, reference, dim_order="BCFHW", frames_per_second=0, wrt="tests"):
        """Extension: the JODs of T test clips against ONE reference as a differentiable [T] fp32 tensor on the metric's device,
        for losses over a ladder such as `(10 - metric.jod_tests(recons, src, frames_per_second=30)).mean()` -- a multi-rate
        codec's T reconstructions of one source, a pre-filter in front of T encoders, a renderer at several quality settings.
        `tests` as predict_tests takes them: a list or tuple of T >= 1 clips shaped like `reference`.  Row k is bit-identical to
        predict_tests(tests, reference, ...)[0][k], and so to jod_video(tests[k], reference) and to predict: the forward makes
        predict_tests' launches.  `wrt`: "tests" (default) -- backward() puts grad[k] dJOD_k/dtests[k] into every test that
        requires grad, bit-identical to jod_video's gradient, a test that does not require grad costs no backward work, and
        the reference is a constant (one that requires grad is refused); "reference" -- backward() puts
        sum_k grad[k] dJOD_k/dreference into `reference`, the tests are constants (one that requires grad is refused); "both"
        -- both from one backward.  Anything else: ValueError.  The reference's backward shares among the tests whatever is
        linear after the pointwise layer gradient: the layer gradients of up to four tests are summed by one launch that reads
        the planes that depend on the reference only once, and the coarse-to-fine sweep, level 0, the temporal transpose and
        the display model's derivative run once per backward batch or clip instead of once per test
        (include/fvvdp_hip_tests_grad.h); its memory does not grow with T.  Accepted, on every clip: what jod_video accepts
        (float32, float16 or bfloat16 samples, C = 1 or 3, one clip of at least 2 frames with B = 1, closed-form display
        models, every temporal padding, filters of up to 64 taps, any layout, on host or device); when the float dtypes of
        the clips differ all are upcast with .float() inside autograd's view, and every gradient arrives in its caller
        tensor's dtype.  Refused, each with a sentence: what predict_tests refuses (a foveated metric, a heat-map metric,
        source objects, a single frame, a `tests` that is no non-empty list or tuple) and what jod_video refuses (integer or
        float64 samples, user photometry, too many taps, shapes that differ).  Nothing is synchronised with the host: no
        out-of-range warning.  Double backward is not supported.  The gradients do not depend on `self.grad_batch`, on the
        grouping of the tests into launches nor on `self.tests_grad_sets` (the map sets a backward batch keeps resident,
        default 4), bit for bit."""
        from .tests_grad import jod_tests
        return jod_tests(self, tests, reference, dim_order, frames_per_second, wrt)

    # ---- the model parameters as variables (extension; include/fvvdp_hip_params.h, param_grad.py) ---------------------
    # the parameters a calibration can fit, in the order of the vectors below: the first six act per band pixel (masking model,
    # sensitivity gain, spatial pooling exponent), the last six in do_pooling_and_jods
    PARAMETER_NAMES = ("mask_p", "mask_q_sust", "mask_q_trans", "mask_c", "sensitivity_correction", "beta",
                       "beta_sch", "beta_tch", "beta_t", "w_transient", "jod_a", "log_jod_exp")

    def parameter_tensor(self):
        """Extension: the current values of PARAMETER_NAMES as a 1-D float64 host tensor."""
        from .param_grad import parameter_tensor
        return parameter_tensor(self)

    def set_parameters(self, theta):
        """Extension: writes a vector laid out as PARAMETER_NAMES into the metric's attributes (what load_config sets)."""
        from .param_grad import set_parameters
        set_parameters(self, theta)

    def calibration_jod_images(self, test, reference, theta, dim_order="BCHW", fixation_point=None):
        """Extension: the JODs of B still-image pairs evaluated UNDER the parameter vector `theta` (laid out as
        PARAMETER_NAMES), as a [B] fp32 tensor on the metric's device, for fitting the model to subjective data.  The metric's
        own attributes are not touched, also when the call raises, and its native context is reused whatever theta is.  The
        values are bit-identical to predict_images on a metric whose attributes hold theta.  When `theta` requires grad (and
        grad mode is on), backward() puts sum_k grad[k] dJOD_k/dtheta into theta.grad, in theta's dtype and on its device;
        theta may be float32 or float64, on the host (read without synchronising the GPU) or on a device.  Sources: what
        predict_images accepts as arrays (uint8 / uint16 / float32, C = 1 or 3); they are constants (one that requires grad is
        refused: jod_images), no out-of-range warning is issued and no heat maps are made (a heat-map metric is refused).
        With a gradient the forward costs a plain pass plus a map-writing pass and one reduction kernel over the maps
        (fvvdp_param_sums), in batches of up to `self.grad_batch` pairs; backward() is arithmetic on [bands, 2, B] arrays."""
        from .param_grad import calibration_jod_images
        return calibration_jod_images(self, test, reference, theta, dim_order, fixation_point)

    def calibration_jod_video(self, test, reference, theta, dim_order="BCFHW", frames_per_second=0, fixation_point=None,
                              temporal=None):
        """Extension: the JOD of one clip evaluated under the parameter vector `theta`, a 0-d fp32 tensor on the metric's
        device; as calibration_jod_images, with predict in the place of predict_images (one clip, B = 1; every temporal padding;
        `fixation_point` as predict takes it) and jod_video for gradients with respect to the frames.  The gradient with respect
        to theta does not depend on `self.grad_batch`, bit for bit.
        temporal: None (the metric's own temporal filters: the launches and the bits of a call without it), or a vector `phi`
        laid out as TEMPORAL_PARAMETER_NAMES (sustained_sigma, sustained_beta; float32 or float64, host or device): the clip is
        evaluated under temporal filters made from phi by the expressions of get_temporal_filters, so the JOD is bit-identical to
        predict on a metric whose attributes hold theta and phi; the metric's attributes are not touched and its context is
        reused.  When phi requires grad, backward() puts dJOD/dphi into phi.grad, in phi's dtype and on its device; theta and phi
        may require grad together or either alone, and theta's gradient is bit-identical whether or not phi is given.  With a
        gradient for phi every backward batch makes one ingest and one map-writing pass (shared with theta's sums), the two
        level-0 backward passes of jod_video(wrt="both"), the luminance of the frames under the batch's windows and the
        tap-gradient kernel (include/fvvdp_hip_taps.h); only dJOD/dtaps [2, filter_len] is kept.  phi.grad depends on
        `self.grad_batch` through the grouping of fp32 sums only (see fvvdp_tap_grad).  Filters above 64 taps are refused when
        phi requires grad."""
        from .param_grad import calibration_jod_video
        return calibration_jod_video(self, test, reference, theta, dim_order, frames_per_second, fixation_point, temporal)

    # the two continuous parameters of the temporal filters (extension; include/fvvdp_hip_taps.h, param_grad.py): not part of
    # PARAMETER_NAMES -- they enter through the host-side taps, and only a clip has a temporal filter
    TEMPORAL_PARAMETER_NAMES = ("sustained_sigma", "sustained_beta")

    def temporal_parameter_tensor(self):
        """Extension: the current values of TEMPORAL_PARAMETER_NAMES as a 1-D float64 host tensor."""
        from .param_grad import temporal_parameter_tensor
        return temporal_parameter_tensor(self)

    def set_temporal_parameters(self, phi):
        """Extension: writes a vector laid out as TEMPORAL_PARAMETER_NAMES into the metric's attributes, as Python floats."""
        from .param_grad import set_temporal_parameters
        set_temporal_parameters(self, phi)

    # the numeric constructor arguments of fvvdp_display_photo_eotf (extension; include/fvvdp_hip_display.h, display_grad.py): a
    # vector of their own, `psi` -- they enter through the display block, a per-call argument of every ingest
    DISPLAY_PARAMETER_NAMES = ("Y_peak", "contrast", "E_ambient", "k_refl", "gamma")

    def display_parameter_tensor(self):
        """Extension: the values of DISPLAY_PARAMETER_NAMES of the metric's fvvdp_display_photo_eotf as a 1-D float64 host
        tensor."""
        from .display_grad import display_parameter_tensor
        return display_parameter_tensor(self)

    def set_display_parameters(self, psi):
        """Extension: gives the metric a new fvvdp_display_photo_eotf with the values of `psi` (laid out as
        DISPLAY_PARAMETER_NAMES) and the metric's own EOTF kind, through set_display_model; the geometry stays."""
        from .display_grad import set_display_parameters
        set_display_parameters(self, psi)

    def display_jod_images(self, test, reference, psi, dim_order="BCHW", fixation_point=None):
        """Extension: the JODs of B still-image pairs shown on a display whose photometry is fvvdp_display_photo_eotf(**psi) with
        the metric's own EOTF kind (psi laid out as DISPLAY_PARAMETER_NAMES), as a [B] fp32 tensor on the metric's device.  The
        geometry and the colour space are the metric's.  The metric's photometry object and its native context are not touched,
        also when the call raises, and nothing is cached per psi.  The values are bit-identical to predict_images on a metric
        built with that photometry from the same Python floats.  When `psi` requires grad (and grad mode is on), backward()
        puts sum_k grad[k] dJOD_k/dpsi into psi.grad, in psi's dtype (float32 or float64) and on its device (host or GPU).
        Sources: float32, C = 1 or 3; they are constants (one that requires grad is refused: jod_images); integer sources, a
        photometry other than the stock fvvdp_display_photo_eotf and a heat-map metric are refused; no out-of-range warning is
        issued.  Without a gradient the call makes the launches of predict_images only.  With one the forward adds, per batch
        of up to `self.grad_batch` pairs, an ingest, a map-writing pass and the two backward passes of jod_images(wrt="both")
        with a reduction in the place of their last kernel (fvvdp_images_display_sums); backward() is arithmetic on
        [B, 2, 3] doubles."""
        from .display_grad import display_jod_images
        return display_jod_images(self, test, reference, psi, dim_order, fixation_point)

    def display_jod_video(self, test, reference, psi, dim_order="BCFHW", frames_per_second=0, fixation_point=None):
        """Extension: the JOD of one clip shown on a display with the photometry psi, a 0-d fp32 tensor on the metric's device;
        as display_jod_images, with predict in the place of predict_images and what jod_video accepts: one float32 clip of at
        least 2 frames, every temporal padding, temporal filters of up to 64 taps.  With a gradient the forward adds the backward
        batches of jod_video(wrt="both") without its two gradient-writing launches: the clip-long level-0 gradients of both
        sides are reduced to three sums each by fvvdp_video_display_sums (include/fvvdp_hip_display.h).  psi.grad does not
        depend on `self.grad_batch`, bit for bit."""
        from .display_grad import display_jod_video
        return display_jod_video(self, test, reference, psi, dim_order, frames_per_second, fixation_point)

    def predict_image_pairs(self, pairs, dim_order="HWC", sync=True, fixation_points=None):
        """Extension: a list of (test, reference) image pairs of arbitrary sizes and sample types (`dim_order` without B and F,
        or with them of size 1).  The pairs are grouped by (shape, dtypes) and every group is scored in batches by
        predict_images' path, reading device-resident images where they lie.  Returns [(Q_JOD, stats)] in input order, each
        shaped as predict() shapes the result of that pair (Q_JOD 0-d, Q_per_ch [bands, 2, 1]); with `sync=True`
        stats['out_of_range'] tells whether a sample of the pair lay outside [0, 1].  Foveated metric: `fixation_points` is
        None (every pair: its image centre, as predict()) or one [x, y] (or None) per pair, in that pair's pixels."""
        self._check_device()
        items = []
        for t, r in pairs:
            t, r = _image_pair(t, r, dim_order)
            _refuse_grad(t)
            _refuse_grad(r)
            items.append((t, r))
        if fixation_points is not None and len(fixation_points) != len(items):
            raise RuntimeError("fixation_points must hold one [x, y] (or None) per image pair")
        groups = {}
        for i, (t, r) in enumerate(items):
            groups.setdefault((tuple(t.shape), t.dtype, r.dtype), []).append(i)
        out = [None] * len(items)
        with torch.cuda.device(self.device):
            for idx in groups.values():
                fix = None
                if self.foveated:
                    H, W = items[idx[0]][0].shape[1:]
                    fix = np.concatenate([self._fixation(None if fixation_points is None else fixation_points[i], W, H, 1)
                                          for i in idx])
                q, st = self._predict_image_group([items[i][0] for i in idx], [items[i][1] for i in idx], fix, sync,
                                                  labels=idx)
                for j, i in enumerate(idx):
                    s = {k: v for k, v in st.items() if k not in ("Q_per_ch", "range_flags", "heatmap", "result_buffer")}
                    s['N_frames'] = 1
                    if sync:
                        s['Q_per_ch'] = np.ascontiguousarray(st['Q_per_ch'][j])
                        s['out_of_range'] = bool(st['range_flags'][j])
                    else:                            # as predict(..., sync=False): fvvdp.finish(s) completes it
                        s['Q_per_ch'] = st['Q_per_ch'][j]
                        s['range_flag'] = st['range_flags'][j:j + 1]
                    if 'heatmap' in st:
                        s['heatmap'] = st['heatmap'][j:j + 1]
                    out[i] = (q[j], s)
        return out

    def _check_device(self):
        if self.device.type != "cuda":
            raise RuntimeError("fovvideovdp_amd needs an AMD GPU (torch device 'cuda'); there is no CPU fallback")

    def _image_eotf(self, dt):
        """(sample type code, fvvdp_eotf) of the display model for samples of torch dtype `dt` (the choice _make_feeder makes
        for a still image)."""
        dtype, nbits = _sample_type(dt)
        use_closed = _is_float_type(dtype) or (dtype == nat.FVVDP_U16 and not getattr(self, "exact_uint16", False))
        desc = native_eotf(self.display_photometry) if use_closed else None
        e = nat.Eotf()
        if desc is None:
            if _is_float_type(dtype):
                raise RuntimeError("predict_images needs a display model with a closed form for float input "
                                   "(a user photometry class works with predict())")
            lut = self._code_lut(self.display_photometry, nbits)
            e.kind, e.d_lut = nat.EOTF_LUT, lut.data_ptr()
            e.L_min, e.L_max = self._lut_dev.table_range(lut)
        else:
            e.kind = desc[0]
            e.Y_peak = desc[1].get("Y_peak", 0.0)
            e.Y_black = desc[1].get("Y_black", 0.0)
            e.gamma = desc[1].get("gamma", 1.0)
            e.L_min = desc[1].get("L_min", 0.0)
            e.L_max = desc[1].get("L_max", 0.0)
        return dtype, e

    def _predict_image_group(self, ts, rs, fix, sync, labels=None):
        """Pairs of one shape ([C, H, W] tensors, host or device) -> (Q_JOD [n], stats).  Batches of up to _batch_size pairs:
        per batch one ingest launch (fvvdp_images_channels), the pyramid launches, one finalisation and one pooling launch
        (fvvdp_images_forward_pool); one device->host copy at the end when `sync`.  `fix`: [n, 2] gaze per pair (foveated
        metric; None = the image centre).  `labels`: the number the out-of-range warning gives each pair (default: its index)."""
        C_ch, height, width = ts[0].shape
        B = len(ts)
        if C_ch != 1 and C_ch != 3:
            raise RuntimeError('The content must have either 1 or 3 colour channels.')
        n_bands, rho_band = self._band_count(width, height)
        if self.foveated and fix is None:
            fix = self._fixation(None, width, height, B)
        if self.do_heatmap and not sync:
            raise RuntimeError("sync=False is not available together with heat-map output")
        # every image on the device as one contiguous [C][H][W] array: resident contiguous images are read where they lie
        dev = self.device
        mixed = ts[0].dtype != rs[0].dtype
        placed = []
        for a in list(ts) + list(rs):
            a = self._to_unit_float(a) if mixed else a.to(dev)
            placed.append(a.contiguous())
        td, rd = placed[:B], placed[B:]
        dtype, e = self._image_eotf(td[0].dtype)
        if e.kind == nat.EOTF_ABSOLUTE and _is_float_type(dtype):
            lo = torch.stack([torch.maximum(a.max(), b.max()) for a, b in zip(td, rd)]).max()
            if float(lo) < 1:
                logging.warning('Pixel values are very low. Perhaps images are not scaled in the absolute units of cd/m^2.')
        w = self._rgb2y()
        batch = self._batch_size(width, height, 2, B)
        heatmap = None
        if self.do_heatmap:
            batch = max(1, min(batch, int(2e9 // (width * height * 4 * 12))))
            heatmap = self._host_buffer([1, 1 if self.heatmap == "raw" else 3, B, height, width])
        ctx = self._context(width, height, n_bands, 2, batch, rho_band)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        nq = n_bands * 2 * B
        res = torch.zeros(nq + 2 * B, dtype=torch.float32, device=dev)       # Q_per_ch | range flags (int32 bits) | JOD
        Q = res[:nq].view(n_bands, 2, B)
        flags = res[nq:nq + B].view(torch.int32)
        jod = res[nq + B:]
        pp = self._pool_params()
        lib = nat.lib()
        for b0 in range(0, B, batch):
            nb = min(batch, B - b0)
            tp = (C.c_void_p * nb)(*[a.data_ptr() for a in td[b0:b0 + nb]])
            rp = (C.c_void_p * nb)(*[a.data_ptr() for a in rd[b0:b0 + nb]])
            nat.check(lib.fvvdp_images_channels(ctx.handle, tp, rp, nb, dtype, C_ch, height * width, C.byref(e), nat.fptr(w), 0,
                                                C.c_void_p(flags.data_ptr() + 4 * b0), stream))
            maps_arr, dmaps = self._band_maps(nb, width, height, n_bands) if self.do_heatmap else (None, None)
            fx, g, _keep = self._fov_args(ctx, fix, b0, nb, n_bands, width, height)
            nat.check(lib.fvvdp_images_forward_pool(ctx.handle, nb, C.c_void_p(Q.data_ptr()), B, b0, fx, g, maps_arr,
                                                    C.byref(pp), C.c_void_p(jod.data_ptr() + 4 * b0), stream))
            if self.do_heatmap:
                self._heatmap_batch(ctx, nb, dmaps, 2, width, height, stream, heatmap, b0)
        stats = {}
        if sync:
            res_h = self._to_host(res)
            if self.do_heatmap and self._copy_stream is not None:
                self._copy_stream.synchronize()
            stats['Q_per_ch'] = np.ascontiguousarray(res_h[:nq].view(n_bands, 2, B).numpy().transpose(2, 0, 1))[..., None]
            stats['range_flags'] = res_h[nq:nq + B].view(torch.int32).numpy() != 0
            for k in np.nonzero(stats['range_flags'])[0]:
                logging.warning("Pixel outside the valid range 0-1 (image pair %d)" % int(k if labels is None else labels[k]))
        else:
            stats['Q_per_ch'] = Q.permute(2, 0, 1).unsqueeze(-1)
            stats['range_flags'] = flags
            stats['result_buffer'] = res
        stats['rho_band'] = rho_band
        stats['frames_per_second'] = 0
        stats['width'] = width
        stats['height'] = height
        if self.do_heatmap:
            stats['heatmap'] = heatmap[0].permute(1, 0, 2, 3).unsqueeze(2)     # [B, ch, 1, H, W]
        return jod, stats

    def _rgb2y(self):
        key = ("rgb2y", self.color_space)
        if key not in self._filters:
            cs = utils.config_files.load("color_spaces.json")
            if self.color_space not in cs:
                raise RuntimeError("Unknown color space: \"" + self.color_space + "\"")
            self._filters[key] = np.asarray(cs[self.color_space]['RGB2Y'], dtype=np.float32)
        return self._filters[key]

    @staticmethod
    def finish(stats):
        """Completes a `sync=False` result in place: device -> host copy of Q_per_ch (one synchronisation) and the
        reference's out-of-range warning."""
        if isinstance(stats.get('Q_per_ch'), torch.Tensor) and 'range_flags' in stats:       # predict_images(..., sync=False)
            flags = stats.pop('range_flags')
            stats.pop('result_buffer', None)
            q = stats['Q_per_ch']
            both = torch.cat([q.reshape(-1), flags.view(torch.float32)]).cpu()
            stats['Q_per_ch'] = both[:q.numel()].view(q.shape).numpy()
            stats['range_flags'] = both[q.numel():].view(torch.int32).numpy() != 0
            for k in np.nonzero(stats['range_flags'])[0]:
                logging.warning("Pixel outside the valid range 0-1 (image pair %d)" % int(k))
            return stats
        if isinstance(stats.get('Q_per_ch'), torch.Tensor):
            flag = stats.pop('range_flag', None)
            stats.pop('result_buffer', None)
            q = stats['Q_per_ch']
            both = torch.cat([q.reshape(-1), flag.view(torch.float32)]).cpu() if flag is not None else q.reshape(-1).cpu()
            stats['Q_per_ch'] = both[:q.numel()].view(q.shape).numpy()
            if flag is not None and int(both[q.numel():].view(torch.int32)[0]) != 0:
                logging.warning("Pixel outside the valid range 0-1")
        return stats

    def _clip_plan(self, vid_source, frame_range=None):
        """How a call walks a clip -- shared by predict and predict_gazes, whose results are bit-identical only on the same plan:
        frame size and range [f0, f1), bands, planes, temporal filter and window index list, the feeder that fills level 0 (host
        sources upload only the frames the range needs; resets self.last_h2d_bytes), the frames per batch (= the context's
        size) and the batch schedule, whose chunk heights group the partial sums."""
        from types import SimpleNamespace
        height, width, N_frames = vid_source.get_video_size()
        f0, f1 = (0, N_frames) if frame_range is None else frame_range
        if not (0 <= f0 < f1 <= N_frames):
            raise RuntimeError("frame_range out of bounds")
        n_bands, rho_band = self._band_count(width, height)
        is_image = (N_frames == 1)
        planes = 2 if is_image else 4
        if is_image:
            fl, taps = 1, np.ones((2, 1), dtype=np.float32)
        else:
            fl, taps = self._temporal_taps(vid_source.get_frames_per_second())
            if fl > nat.MAX_TAPS:
                raise RuntimeError("frame rate too high: temporal filter longer than %d taps" % nat.MAX_TAPS)
        n_out = f1 - f0
        wkey = (N_frames, fl, self.temp_padding, f0, f1, is_image)
        wc = self._filters.get(wkey)
        if wc is None:
            widx = window_frame_indices(N_frames, fl, self.temp_padding) if not is_image else np.zeros(1, np.int32)
            wc = (widx, np.unique(widx[f0:f1 + fl - 1]))
            if len(self._filters) > 64:
                self._filters.clear()
            self._filters[wkey] = wc
        widx, need = wc
        # source frames this call touches: the windows of output frames [f0, f1) (frame sharding: a rank's own frames plus
        # the fl-1 frames of temporal halo before them) -- host-resident sources upload these and nothing else
        self.last_h2d_bytes = 0
        feeder = self._make_feeder(vid_source, width, height, need)
        batch = self._batch_size(width, height, planes, n_out, fl)
        schedule = None
        if self.batch_frames is None and getattr(feeder, "preferred_batch", None):
            batch = max(1, min(batch, feeder.preferred_batch))
            if not self.do_heatmap:
                schedule = feeder.batch_schedule(n_out, batch)
        if self.do_heatmap:
            batch = max(1, min(batch, int(2e9 // (width * height * 4 * 12))))     # D maps + context image per frame
        if schedule is None:
            schedule = [min(batch, f1 - b0) for b0 in range(f0, f1, batch)]
        return SimpleNamespace(height=height, width=width, N_frames=N_frames, f0=f0, f1=f1, n_bands=n_bands, rho_band=rho_band,
                               planes=planes, fl=fl, taps=taps, widx=widx, feeder=feeder, batch=batch, schedule=schedule)

    def _predict_on_device(self, vid_source, fixation_point, frame_range, pool, sync=True):
        height, width, N_frames = vid_source.get_video_size()
        fix = self._fixation(fixation_point, width, height, N_frames) if self.foveated else None
        pl = self._clip_plan(vid_source, frame_range)
        f0, f1, n_bands, rho_band, planes, fl, taps, widx = pl.f0, pl.f1, pl.n_bands, pl.rho_band, pl.planes, pl.fl, pl.taps, pl.widx
        feeder, batch, schedule = pl.feeder, pl.batch, pl.schedule
        n_out = f1 - f0
        heatmap = None
        if self.do_heatmap:
            dmap_channels = 1 if self.heatmap == "raw" else 3
            # fp16 on the host like the reference (fvvdp.py:216-221); every element is written below, and page-locked
            # memory lets the batches stream back at link speed while the next batch is computed
            heatmap = self._host_buffer([1, dmap_channels, n_out, height, width])
        ctx = self._context(width, height, n_bands, planes, batch, rho_band)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        # results + the out-of-range flag share one buffer: a single device->host copy (and sync) per call
        nq = n_bands * 2 * n_out
        res = torch.zeros(nq + 2, dtype=torch.float32, device=self.device)      # Q_per_ch | range flag | JOD
        Q = res[:nq].view(n_bands, 2, n_out)
        oob = res[nq:nq + 1].view(torch.int32)

        # pooling + JOD regression (do_pooling_and_jods, fvvdp.py:337-357) ride on the last batch
        pp = self._pool_params()
        b0 = f0
        bi = -1
        while bi + 1 < len(schedule):
            bi += 1
            nb = schedule[bi]
            idx = np.ascontiguousarray(widx[b0:b0 + fl - 1 + nb])          # history + newest frames of this batch
            try:
                feeder(ctx, idx, taps, fl, nb, oob, stream)
            except _SourceRecyclesBuffers:
                # A user source overwrote frames that the kernels of the PREVIOUS batch may still have been reading (it decodes
                # into buffers it reuses).  The feeder has switched to copying every frame on arrival; the previous batch is
                # evaluated again from intact frames (its Q columns are simply rewritten, in stream order), then this one.
                if bi > 0:
                    bi -= 1
                    b0 -= schedule[bi]
                bi -= 1
                continue
            # per-band difference maps as extra kernel outputs
            maps_arr, dmaps = self._band_maps(nb, width, height, n_bands) if self.do_heatmap else (None, None)
            fx, g, _keep = self._fov_args(ctx, fix, b0, nb, n_bands, width, height)
            if pool and b0 + nb == f1:               # the batch that completes the clip also pools (one launch fewer)
                nat.check(nat.lib().fvvdp_bands_forward_pool(ctx.handle, nb, C.c_void_p(Q.data_ptr()), n_out, b0 - f0,
                                                             fx, g, maps_arr, C.byref(pp), C.c_void_p(res[nq + 1:].data_ptr()),
                                                             stream))
            else:
                nat.check(nat.lib().fvvdp_bands_forward(ctx.handle, nb, C.c_void_p(Q.data_ptr()), n_out, b0 - f0,
                                                        fx, g, maps_arr, stream))
            if self.do_heatmap:
                self._heatmap_batch(ctx, nb, dmaps, planes, width, height, stream, heatmap, b0 - f0)
            b0 += nb

        Q_jod = res[nq + 1] if pool else None                 # pooled with the last batch (fvvdp_bands_forward_pool)
        stats = {}
        if sync:
            res_h = self._to_host(res)                       # the one host synchronisation of the call
            if self.do_heatmap and self._copy_stream is not None:
                self._copy_stream.synchronize()              # ... plus the side stream that carries the maps
            stats['Q_per_ch'] = res_h[:nq].view(n_bands, 2, n_out).numpy()
        else:
            if self.do_heatmap:
                raise RuntimeError("sync=False is not available together with heat-map output")
            stats['Q_per_ch'] = Q
            stats['range_flag'] = oob
            stats['result_buffer'] = res          # [Q_per_ch (bands x 2 x frames) | range flag (int32 bits) | JOD]: one row per pair
        stats['rho_band'] = rho_band
        stats['frames_per_second'] = vid_source.get_frames_per_second()
        stats['width'] = width
        stats['height'] = height
        stats['N_frames'] = N_frames
        if self.do_heatmap:
            stats['heatmap'] = heatmap
        if sync and int(res_h[nq:nq + 1].view(torch.int32)[0]) != 0:
            logging.warning("Pixel outside the valid range 0-1")
        if hasattr(feeder, "release"):
            feeder.release(synced=sync)
        return (Q_jod, stats)

    def _to_host(self, res):
        """Result buffer -> host through a page-locked staging buffer kept by the metric (a pageable `.cpu()` costs ~0.1 ms more per
        call: 4K x 60, 4.25 against 4.15 ms); the caller gets its own copy.  Falls back to `.cpu()` where page-locking is refused."""
        n = res.numel()
        pin = self.__dict__.get("_res_pin")
        if pin is False:                       # page-locking was refused once: do not ask again
            return res.detach().cpu()
        if pin is None or pin.numel() < n:
            try:
                pin = torch.empty(max(n, 4096), dtype=torch.float32, pin_memory=True)
            except RuntimeError:
                pin = False
            self._res_pin = pin
        if pin is False:
            return res.detach().cpu()
        pin[:n].copy_(res.detach(), non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return pin[:n].clone()

    @staticmethod
    def _host_buffer(shape):
        nbytes = 2 * int(np.prod(shape))
        if nbytes <= (4 << 30):                   # long clips: do not page-lock tens of GB of host memory
            try:
                return torch.empty(shape, dtype=torch.float16, pin_memory=True)
            except RuntimeError:                  # page-locking refused (ulimit): plain pageable memory
                pass
        return torch.empty(shape, dtype=torch.float16)

    def _heatmap_batch(self, ctx, nb, dmaps, planes, width, height, stream, heatmap, k0):
        """Difference maps of `nb` frames -> heatmap[0, :, k0:k0+nb] (fp16, host) (fvvdp.py:469-476).  The maps are
        finished on the device in the output layout and copied back asynchronously, one contiguous run per channel."""
        ptrs = (C.c_void_p * len(dmaps))(*[d.data_ptr() for d in dmaps])
        dmap = torch.empty((nb, height, width), dtype=torch.float32, device=self.device)
        beta_jod = float(np.power(10.0, self.log_jod_exp))
        nat.check(nat.lib().fvvdp_heatmap_reconstruct(ctx.handle, nb, ptrs, float(self.w_transient), beta_jod,
                                                      abs(float(self.jod_a)), C.c_void_p(dmap.data_ptr()), stream))
        if self.heatmap == "raw":
            self._copy_back(dmap.to(torch.float16).unsqueeze(0), [heatmap[0, 0, k0:k0 + nb]])
            return
        # colouring on the device (fvvdp_heatmap_colorize): tone-mapped context frame x colour map, fp16, output layout
        from .visualize_diff_map import color_tables_host
        knots, rgb = color_tables_host(self.heatmap)
        lin01 = torch.linspace(0.0, 1.0, 1024).numpy()
        out = torch.empty((3, nb, height, width), dtype=torch.float16, device=self.device)
        nat.check(nat.lib().fvvdp_heatmap_colorize(ctx.handle, nb, C.c_void_p(dmap.data_ptr()), nat.fptr(knots), nat.fptr(rgb),
                                                   len(knots), nat.fptr(lin01), C.c_void_p(out.data_ptr()),
                                                   nb * height * width, stream))
        self._copy_back(out, [heatmap[0, ch, k0:k0 + nb] for ch in range(3)])

    def _copy_back(self, src, dst_list):
        """Device -> host copies of finished maps on a side stream, so that the next batch's kernels run meanwhile
        (page-locked destination; with pageable memory the copy is synchronous anyway)."""
        main = torch.cuda.current_stream(self.device)
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        done = torch.cuda.Event()
        done.record(main)
        with torch.cuda.stream(self._copy_stream):
            self._copy_stream.wait_event(done)
            for i, dst in enumerate(dst_list):
                dst.copy_(src[i], non_blocking=True)
        src.record_stream(self._copy_stream)      # the caching allocator must not hand `src` out before the copy ran

    # ---- pooling and JOD regression (Python, as in the reference) ------------------------------------------
    def do_pooling_and_jods(self, Q_per_ch, rho_band):
        """Q_per_ch [bands, temporal channels, frames] -> JOD (0-d tensor).  Minkowski pooling over spatial bands
        (beta_sch), temporal channels (beta_tch, transient weighted by w_transient) and frames (beta_t, mean).
        A leading batch dimension [K, bands, channels, frames] pools K videos at once -> [K]."""
        Q = Q_per_ch
        d = Q.dim() - 3                        # 0, or 1 with a leading batch of videos
        if Q.shape[d + 1] == 2:
            key = (str(Q.device), Q.dtype)             # cached: a host->device upload per call costs a stream sync
            if key not in self._chan_w:
                self._chan_w[key] = torch.tensor([1.0, self.w_transient], dtype=Q.dtype, device=Q.device).view(1, 2, 1)
            Q = Q * self._chan_w[key]
        Q_sc = self.lp_norm(Q, self.beta_sch, d + 0, False)
        Q_tc = self.lp_norm(Q_sc, self.beta_tch, d + 1, False)
        Q_all = self.lp_norm(Q_tc, self.beta_t, d + 2, True)
        Q_all = Q_all.reshape(Q_all.shape[0]) if d == 1 else Q_all.squeeze()
        beta_jod = 10.0 ** self.log_jod_exp
        sign = -1 if self.jod_a < 0 else 1
        Q_jod = sign * ((abs(self.jod_a) ** (1.0 / beta_jod)) * Q_all) ** beta_jod + 10.0
        return Q_jod if d == 1 else Q_jod.squeeze()

    def lp_norm(self, x, p, dim=0, normalize=True):
        N = x.shape[dim] if normalize else 1.0
        return torch.norm(x, p, dim=dim, keepdim=True) / (float(N) ** (1. / p))

    def get_temporal_filters(self, frames_per_s):
        """Sustained (log-Gaussian) and transient (its scaled derivative) temporal filters, fp32 [2, filter_len];
        tap k weights the frame k steps in the past.  Evaluated on the host."""
        F = temporal_filters(frames_per_s, self.filter_len, self.sustained_sigma, self.sustained_beta)
        omega = torch.tensor([0, 5])
        return F, omega

    def short_name(self):
        return "FovVideoVDP"

    def quality_unit(self):
        return "JOD"

    def get_info_string(self):
        standard_str = ', (' + self.display_name + ')' if self.display_name.startswith('standard_') else ''
        fv_mode = 'foveated' if self.foveated else 'non-foveated'
        return '"FovVideoVDP v{}, {:.4g} [pix/deg], Lpeak={:.5g}, Lblack={:.4g} [cd/m^2], {}{}"'.format(
            self.version, self.pix_per_deg, self.display_photometry.get_peak_luminance(),
            self.display_photometry.get_black_level(), fv_mode, standard_str)

    def write_features_to_json(self, stats, dest_fname):
        Q_per_ch = stats['Q_per_ch']
        fmap = {}
        for key, value in stats.items():
            if key not in ["Q_per_ch", "heatmap"]:
                fmap[key] = value.tolist() if isinstance(value, np.ndarray) else value
        for cc in range(Q_per_ch.shape[1]):
            for bb in range(Q_per_ch.shape[0]):
                fmap[f"t{cc}_b{bb}"] = Q_per_ch[bb, cc, :].tolist()
        with open(dest_fname, 'w', encoding='utf-8') as f:
            json.dump(fmap, f, ensure_ascii=False, indent=4)

    # ---- host-side preparation for the kernels --------------------------------------------------------------
    def native_params(self):
        p = nat.Params()
        p.mask_p = self.mask_p
        p.mask_q[0], p.mask_q[1] = self.mask_q_sust, self.mask_q_trans
        mk = self.__dict__.get("_mask_k")
        if mk is None or mk[0] != self.mask_c:                  # fp32 power like the reference's (fvvdp.py:585), once per value
            mk = (self.mask_c, float(torch.pow(torch.tensor(10.0), torch.tensor(self.mask_c))))
            self._mask_k = mk
        p.mask_k = mk[1]
        p.beta = self.beta
        p.sens_gain = 10.0 ** (self.sensitivity_correction / 20.0)
        p.lbkg_min, p.contrast_max, p.d_max = 0.1, 1000.0, 1e4
        return p

    def csf_tables_1d(self, rho_band, n_bands):
        """Non-foveated mode: the rho and eccentricity coordinates of the CSF query are constant per band, so the
        trilinear LUT interpolation reduces to a 1-D table over log2(L_bkg) per (band, temporal channel).  The
        rho-axis blend is done here with the same fp32 operations the per-pixel interpolation would use."""
        tab = np.zeros((n_bands, 2, nat.LUT_N), dtype=np.float32)
        for cc in range(2):
            lut = {k: torch.from_numpy(v) for k, v in self.csf_lut[cc].items()}
            for bb in range(n_bands):
                rho = torch.tensor([rho_band[bb]], dtype=torch.float32)
                rho_q = torch.log2(torch.clamp(rho, lut["rho"][0], lut["rho"][-1]))
                imin, imax, ifrc = _interpolants(rho_q, lut["rho_log"])
                v = lut["S_log"]                       # [Y, rho, ecc]; ecc = 0 sits exactly on knot 0
                t = v[:, imin[0], 0] * (1.0 - ifrc[0]) + v[:, imax[0], 0] * ifrc[0]
                tab[bb, cc] = t.numpy()
        return np.ascontiguousarray(self.csf_lut[0]["Y_log"], dtype=np.float32), tab

    def _context_key(self, W, H, n_bands, planes, batch, rho_band):
        """Everything the native context bakes in at creation, by VALUE: size, band frequencies (display resolution /
        distance), mode, model constants and the identity of the CSF tables.  (The reference re-reads all of these on
        every call, pyfvvdp/fvvdp.py:147-161,209-213,442-447.)"""
        prm = self.native_params()
        pv = (prm.mask_p, prm.mask_q[0], prm.mask_q[1], prm.mask_k, prm.beta, prm.sens_gain, prm.lbkg_min,
              prm.contrast_max, prm.d_max)
        lut_id = tuple((id(l["S_log"]), l["S_log"].shape) for l in self.csf_lut)
        return (W, H, n_bands, planes, batch, tuple(float(r) for r in rho_band), bool(self.foveated), pv, lut_id,
                str(self.device), self.timing is not None)

    def _context(self, W, H, n_bands, planes, batch, rho_band):
        key = self._context_key(W, H, n_bands, planes, batch, rho_band)
        if self._ctx is not None:
            have = self._ctx.key
            # a context made for a longer batch serves a shorter one (clips of different lengths in one folder: no new scratch,
            # no second choice of the level-0 ranges); everything else it bakes in must match by value
            if have[:4] == key[:4] and have[5:] == key[5:] and have[4] >= batch:
                return self._ctx
        self._drop_context()
        with torch.cuda.device(self.device):
            ctx = _Context(W, H, n_bands, planes, batch, rho_band, self.native_params())
            ctx.key = key
            ctx.luts = self.csf_lut           # keeps the arrays whose id() is part of the key alive
            if self.foveated:
                for cc in range(2):
                    l = self.csf_lut[cc]
                    nat.check(nat.lib().fvvdp_ctx_set_csf_3d(ctx.handle, cc, nat.fptr(l["S_log"]), nat.fptr(l["Y_log"]),
                                                             nat.fptr(l["rho_log"]), nat.fptr(l["ecc_sqrt"])))
            else:
                y_log, tab = self.csf_tables_1d(rho_band, n_bands)
                nat.check(nat.lib().fvvdp_ctx_set_csf_1d(ctx.handle, nat.fptr(y_log), nat.fptr(tab)))
            if self.timing is not None:
                nat.check(nat.lib().fvvdp_ctx_timing_enable(ctx.handle, 1))
        self._ctx = ctx
        return ctx

    def _batch_size(self, W, H, planes, n_out, fl=1):
        cap = 128
        if fl > 32:
            # 33..64 taps: the two-pass temporal path converts the batch's fl-1+batch source frames to fp32 luminance first
            # (2 streams x 4 B per pixel, context-owned) and addresses them through a 320-entry index table
            cap = max(1, min(cap, 320 - (fl - 1)))
        if self.batch_frames is not None:
            return max(1, min(int(self.batch_frames), n_out, cap if fl > 32 else n_out))
        per_frame = W * H * planes * 4 * 1.34          # all Gaussian levels of one frame
        budget = 24e9                                  # resident pyramid scratch (of 288 GB HBM3E)
        if fl > 32:
            budget -= (fl - 1) * W * H * 8.0           # luminance frames of the temporal window
            per_frame += W * H * 8.0                   # ... and of every frame of the batch
        return max(1, min(n_out, cap, int(max(budget, per_frame) // per_frame)))

    # ---- launch arguments shared by predict, predict_images and the launch layer of the gradients (grad_passes.py) ----------
    def _band_count(self, width, height):
        """(number of band-pass levels, their centre frequencies) of a frame on this display; refuses a frame with none."""
        n_bands, rho_band = band_frequencies(width, height, self.pix_per_deg)
        if n_bands < 1:
            raise RuntimeError("Frame %dx%d is too small for this display (no band-pass level)" % (width, height))
        return n_bands, rho_band

    @staticmethod
    def _level_sizes(width, height, n_bands):
        """(w, h) of pyramid levels 0 .. n_bands: the band-pass levels and the base band's level below them."""
        out = [(width, height)]
        for _ in range(n_bands):
            w, h = out[-1]
            out.append(((w + 1) // 2, (h + 1) // 2))
        return out

    def _pool_params(self):
        """Pooling and JOD regression constants of do_pooling_and_jods (fvvdp.py:337-357) for the pooling kernels."""
        return nat.PoolParams(self.beta_sch, self.beta_tch, self.beta_t, self.w_transient, self.jod_a,
                              float(10.0 ** self.log_jod_exp))

    def _temporal_taps(self, fps):
        """(filter length, taps fp32 [2, filter length]) at `fps` frames per second; sets self.filter_len and self.F as the
        reference does.  The taps depend on the frame rate only: evaluated once per rate."""
        self.filter_len = filter_length(fps)
        fkey = (float(fps), self.filter_len, float(self.sustained_sigma), float(self.sustained_beta))
        if fkey not in self._filters:
            F, _ = self.get_temporal_filters(fps)
            self._filters[fkey] = (F, np.ascontiguousarray(F.numpy(), dtype=np.float32))
        self.F, taps = self._filters[fkey]
        return self.filter_len, taps

    def _band_maps(self, n, width, height, n_bands, contrast_planes=None):
        """fvvdp_band_maps of every band for `n` frames or pairs, and the tensors behind them (the caller keeps them alive).
        contrast_planes None: the difference maps D only (heat maps), the list holds one tensor per band.  2 (images) or 4
        (video): all four maps (the backward passes), D, contrast, L_bkg, S per band."""
        maps_arr = (nat.BandMaps * n_bands)()
        keep = []
        for b, (w, h) in enumerate(self._level_sizes(width, height, n_bands)[:n_bands]):
            D = torch.empty((n, 2, h, w), dtype=torch.float32, device=self.device)
            maps_arr[b].d_D = D.data_ptr()
            keep.append(D)
            if contrast_planes is not None:
                Cn = torch.empty((n, contrast_planes, h, w), dtype=torch.float32, device=self.device)
                L = torch.empty((n, h, w), dtype=torch.float32, device=self.device)
                S = torch.empty((n, 2, h, w), dtype=torch.float32, device=self.device)
                maps_arr[b].d_contrast, maps_arr[b].d_lbkg, maps_arr[b].d_S = Cn.data_ptr(), L.data_ptr(), S.data_ptr()
                keep += [Cn, L, S]
        return maps_arr, keep

    def _fov_args(self, ctx, fix, b0, nb, n_bands, width, height):
        """(fixation pointer, geometry pointer, array to keep alive until the launch) for entries [b0, b0 + nb) of the gaze
        list `fix`; three None for a metric that is not foveated."""
        if not self.foveated:
            return None, None, None
        fxa = np.ascontiguousarray(fix[b0:b0 + nb], dtype=np.float32)
        g = None
        if native_geometry(self.display_geometry) is not None:
            g = C.byref(self._geom_struct())
        else:                                # user geometry: maps + gaze view directions (degrees)
            self._set_view_maps(ctx, n_bands, width, height)
            fxa = self._gaze_view_dirs(fxa, width, height)
        return nat.fptr(fxa), g, fxa

    def _set_view_maps(self, ctx, n_bands, width, height):
        """User geometry model: evaluate its pix2view_direction / get_resolution_magnification once per band on the
        band's pixel grid (as the reference does per frame, fvvdp.py:424-437) and hand the maps to the kernels."""
        geom = self.display_geometry
        gstate = tuple(sorted((k, repr(v)) for k, v in vars(geom).items() if isinstance(v, (int, float, str, tuple, list, type(None)))))
        if getattr(ctx, "view_maps", None) is not None and ctx.view_geom is geom and ctx.view_gstate == gstate:
            return
        maps = []
        for b, (w_b, h_b) in enumerate(self._level_sizes(width, height, n_bands)[:n_bands]):
            xv = torch.linspace(0.5, w_b - 0.5, w_b, device=self.device)
            yv = torch.linspace(0.5, h_b - 0.5, h_b, device=self.device)
            xx, yy = torch.meshgrid(xv, yv, indexing='xy')
            vd = self.display_geometry.pix2view_direction(torch.tensor((w_b, h_b)), xx, yy)
            rm = self.display_geometry.get_resolution_magnification(vd)
            if rm.dim() == 0:
                rm = rm.expand(h_b, w_b)
            vx = vd[0].to(torch.float32).contiguous()
            vy = vd[1].to(torch.float32).contiguous()
            rm = rm.to(torch.float32).contiguous()
            maps.append((vx, vy, rm))
            nat.check(nat.lib().fvvdp_ctx_set_view_maps(ctx.handle, b, C.c_void_p(vx.data_ptr()), C.c_void_p(vy.data_ptr()),
                                                        C.c_void_p(rm.data_ptr()), float(rm.min()), float(rm.max())))
        ctx.view_maps = maps          # keep the tensors alive as long as the context
        ctx.view_geom, ctx.view_gstate = geom, gstate     # strong reference: the object's id cannot be recycled

    def _gaze_view_dirs(self, fix_px, width, height):
        """Gaze positions [n,2] in frame pixels -> view directions in degrees through the user's geometry."""
        fx = torch.as_tensor(fix_px[:, 0] + 0.5, device=self.device)
        fy = torch.as_tensor(fix_px[:, 1] + 0.5, device=self.device)
        vd = self.display_geometry.pix2view_direction(torch.tensor((width, height)), fx, fy)
        return np.ascontiguousarray(torch.stack((vd[0], vd[1]), dim=1).to(torch.float32).cpu().numpy())

    def _geom_struct(self):
        d = native_geometry(self.display_geometry)
        if d is None:
            raise RuntimeError("internal: user geometry goes through _set_view_maps")
        g = nat.Geom()
        g.display_size_m[0], g.display_size_m[1] = d["display_size_m"]
        g.distance_m, g.ppd_centre = d["distance_m"], d["ppd_centre"]
        return g

    def _fixation(self, fixation_point, width, height, N):
        if fixation_point is None:
            fp = np.array([width // 2, height // 2], dtype=np.float32)
        elif isinstance(fixation_point, torch.Tensor):
            fp = fixation_point.detach().cpu().numpy().astype(np.float32)
        else:
            fp = np.asarray(fixation_point, dtype=np.float32)
        if fp.ndim == 1:
            fp = np.tile(fp.reshape(1, 2), (N, 1))
        if fp.shape != (N, 2):
            raise RuntimeError("fixation_point must be [x, y] or an [N_frames, 2] array")
        return np.ascontiguousarray(fp, dtype=np.float32)

    def _code_lut(self, photometry, nbits):
        """Luminance of every integer code value through the display model's own `forward` (user photometry
        subclasses work), kept on the device; cached by value, see display_model.code_value_tables."""
        return self._lut_dev.get(photometry, nbits, self.device)

    def _to_unit_float(self, a):
        a = a.to(self.device)
        if a.dtype is torch.float32:
            return a
        if a.dtype is torch.float16 or a.dtype is torch.bfloat16:
            return a.to(torch.float32)          # exact
        if a.dtype is torch.uint8:
            return a.to(torch.float32) / 255
        if a.dtype is torch.int16:
            return (a.to(torch.int32) & 0xFFFF).to(torch.float32) / 65535
        raise RuntimeError("Only uint8, uint16 and float32 is currently supported")

    def _place_sources(self, test, ref, need):
        """Source arrays [1, C, F, H, W] -> (test, ref) on the compute device plus the frame number -> position map (None:
        all frames are there in place).  Arrays that are already resident are used where they lie (no copy).  If one of
        them lives on the host, only the frames in `need` (sorted unique frame numbers) cross PCIe: with frame sharding a
        rank uploads its own frames plus the fl-1 frames of temporal halo, not the clip."""
        dev = self.device
        F = test.shape[2]
        if (test.device == dev and ref.device == dev) or len(need) >= F:
            out, remap = [], None
            for a in (test, ref):
                if a.device != dev:
                    self.last_h2d_bytes += a.numel() * a.element_size()
                out.append(a.to(dev).contiguous())
            return out[0], out[1], remap
        lo, hi = int(need[0]), int(need[-1])
        run = (hi - lo + 1 == len(need))               # one run of frames: a view; else (circular / pingpong history) a gather
        out = []
        for a in (test, ref):
            sub = a[:, :, lo:hi + 1] if run else a.index_select(2, torch.as_tensor(np.asarray(need, dtype=np.int64), device=a.device))
            if a.device != dev:
                self.last_h2d_bytes += sub.numel() * sub.element_size()
            out.append(sub.to(dev).contiguous())
        remap = np.full(F, -1, dtype=np.int32)
        remap[np.asarray(need, dtype=np.int64)] = np.arange(len(need), dtype=np.int32)
        return out[0], out[1], remap

    def _make_feeder(self, vs, width, height, need=None):
        """Returns feed(ctx, idx, taps, fl, n_out, oob, stream): fills pyramid level 0 of slots [0, n_out).
        `need`: sorted unique source frames the call will ask for (all frames when None)."""
        lib = nat.lib()
        HW = width * height
        if type(vs) is fvvdp_video_source_array or isinstance(vs, fvvdp_video_source_array):
            test = vs.test_video
            ref = vs.reference_video
            if test.shape[0] != 1:
                raise RuntimeError("Only batch size 1 is supported (as in the reference's sliding-window code)")
            if ref.dtype != test.dtype:
                # the reference unpacks each array by its own dtype (video_source.py:186-200): bring both to
                # normalised fp32 code values on the device, then the common float path applies
                test, ref = self._to_unit_float(test), self._to_unit_float(ref)
            dtype, nbits = _sample_type(test.dtype)
            C_ch = test.shape[1]
            if need is None:
                need = np.arange(test.shape[2])
            # uint8: 256-entry table through the model's own forward() (exact, lives in LDS).  uint16: the 65536-entry
            # table sits in global memory (6 gathers per pixel: K1 98 vs 37 us/frame at 4K), so stock display models are
            # evaluated in closed form on code/65535 like float input (<= 1e-6 relative); `exact_uint16 = True` on the
            # metric, or a user photometry class, keeps the table.
            use_closed = _is_float_type(dtype) or (dtype == nat.FVVDP_U16 and not getattr(self, "exact_uint16", False))
            desc = native_eotf(vs.dm_photometry) if use_closed else None
            if not _is_float_type(dtype) or desc is not None:
                test_d, ref_d, remap = self._place_sources(test, ref, need)
                N = test_d.shape[2]
                e = nat.Eotf()
                if desc is None:
                    lut = self._code_lut(vs.dm_photometry, nbits)
                    e.kind, e.d_lut = nat.EOTF_LUT, lut.data_ptr()
                    e.L_min, e.L_max = self._lut_dev.table_range(lut)      # lets the pyramid pass drop clamps that cannot bind
                else:
                    e.kind = desc[0]
                    e.Y_peak = desc[1].get("Y_peak", 0.0)
                    e.Y_black = desc[1].get("Y_black", 0.0)
                    e.gamma = desc[1].get("gamma", 1.0)
                    e.L_min = desc[1].get("L_min", 0.0)
                    e.L_max = desc[1].get("L_max", 0.0)
                    # (on the source arrays, not the uploaded subset: a frame-sharded call warns like the unsharded one)
                    if e.kind == nat.EOTF_ABSOLUTE and _is_float_type(dtype) and float(torch.maximum(test.max(), ref.max())) < 1:
                        logging.warning('Pixel values are very low. Perhaps images are not scaled in the absolute units of cd/m^2.')
                w = np.asarray(vs.color_to_luminance, dtype=np.float32)

                def feed(ctx, idx, taps, fl, n_out, oob, stream, slot0=0):
                    if remap is not None:
                        idx = np.ascontiguousarray(remap[idx])
                    nat.check(lib.fvvdp_temporal_channels(
                        ctx.handle, C.c_void_p(test_d.data_ptr()), C.c_void_p(ref_d.data_ptr()), dtype, C_ch,
                        N * HW, HW, C.byref(e), nat.fptr(w), idx.ctypes.data_as(C.POINTER(C.c_int32)),
                        nat.fptr(taps), fl, n_out, slot0, C.c_void_p(oob.data_ptr()), stream))

                upcast = []          # float16 / bfloat16 clips as float32, made on the first luminance() call

                def luminance(frames, out, oob, stream):
                    """fp32 luminance of the source frames `frames` (int32 array) of both clips into out [2, len, H, W]: the
                    values feed's temporal kernel filters (fvvdp_luminance_frames).  That entry point takes uint8, uint16 and
                    float32: a half-precision clip goes in upcast (exact, so the values are still the ones feed filters)."""
                    if remap is not None:
                        frames = remap[frames]
                    frames = np.ascontiguousarray(frames, dtype=np.int32)
                    lt, lr, ldtype = test_d, ref_d, dtype
                    if dtype in (nat.FVVDP_F16, nat.FVVDP_BF16):
                        if not upcast:
                            upcast.extend([test_d.float(), ref_d.float()])
                        lt, lr, ldtype = upcast[0], upcast[1], nat.FVVDP_F32
                    nat.check(lib.fvvdp_luminance_frames(
                        C.c_void_p(lt.data_ptr()), C.c_void_p(lr.data_ptr()), ldtype, C_ch, width, height, N * HW, HW,
                        C.byref(e), nat.fptr(w), frames.ctypes.data_as(C.POINTER(C.c_int32)), len(frames),
                        C.c_void_p(out.data_ptr()), C.c_void_p(oob.data_ptr()), stream))
                feed.luminance = luminance
                return feed
        if (isinstance(vs, fvvdp_video_source_yuv_frames) and native_eotf(vs.dm_photometry) is not None
                and not (hasattr(vs, "_resizing") and vs._resizing())
                and filter_length(max(vs.get_frames_per_second(), 1e-9)) <= 64):   # > 256 fps: generic path
            # raw planar YUV: unpacking, chroma upsampling, colour matrix and display model run in the HIP kernel
            test_d = vs.test_yuv.to(self.device).contiguous()
            ref_d = vs.reference_yuv.to(self.device).contiguous()
            desc = native_eotf(vs.dm_photometry)
            e = nat.Eotf()
            e.kind = desc[0]
            e.Y_peak = desc[1].get("Y_peak", 0.0)
            e.Y_black = desc[1].get("Y_black", 0.0)
            e.gamma = desc[1].get("gamma", 1.0)
            e.L_min = desc[1].get("L_min", 0.0)
            e.L_max = desc[1].get("L_max", 0.0)
            fmt = nat.YuvFormat()
            fmt.bit_depth = vs.bit_depth
            fmt.chroma_420 = 1 if vs.chroma_ss == "420" else 0
            for i, val in enumerate(np.asarray(vs.ycbcr2rgb, dtype=np.float32).reshape(-1)):
                fmt.ycbcr2rgb[i] = float(val)
            w = np.asarray(vs.color_to_luminance, dtype=np.float32)

            def feed_yuv(ctx, idx, taps, fl, n_out, oob, stream, slot0=0):
                if fl > 64:
                    raise RuntimeError("frame rate too high for the YUV path (temporal filter longer than 64 taps)")
                nat.check(lib.fvvdp_temporal_channels_yuv(
                    ctx.handle, C.c_void_p(test_d.data_ptr()), C.c_void_p(ref_d.data_ptr()), C.byref(fmt), vs.frame_elems,
                    C.byref(e), nat.fptr(w), idx.ctypes.data_as(C.POINTER(C.c_int32)), nat.fptr(taps), fl, n_out, slot0,
                    C.c_void_p(oob.data_ptr()), stream))
            return feed_yuv
        # generic sources (user subclasses, custom float photometry): luminance frames come from the source's own
        # get_*_frame (the user's code, run on the device); the kernels take over from the temporal filter on.
        return _PipelinedSourceFeeder(self, vs, width, height)


class _SourceRecyclesBuffers(Exception):
    """Raised by _PipelinedSourceFeeder the moment it sees a source reuse the buffer of a frame that was still in the temporal
    window (see there); _predict_on_device re-runs the batch whose input may have been overwritten."""


class _PipelinedSourceFeeder:
    """Frame supply for sources whose frames only exist behind their own `get_*_frame`.

    The reference fetches synchronously inside its frame loop (pyfvvdp/fvvdp.py:287-288).  Here every source frame is
    still fetched exactly once (on a side stream), nothing waits on the host -- while the kernels of batch b run, the
    Python code of the source already produces batch b+1 -- and nothing is copied: the temporal kernel reads the
    luminance tensors the source returned where they are (fvvdp_temporal_channels_frames; frames of the temporal window
    that were fetched for an earlier batch are simply kept alive).  Sources whose tensors the kernel cannot address
    (too far apart in memory, filters longer than 64 taps) go through one stacking copy per stream and batch instead.

    Contract for user sources: a tensor returned by `get_*_frame` is read in place for up to filter_len - 1 + batch later
    frames, and frames may be asked for again (random access).  A source that decodes into buffers it reuses (`return
    self._buf`) is noticed AFTER the fact -- a fresh frame arrives at the address of a frame still in the window, or the test and
    the reference frame of one fetch share an address.  By then the overwritten frames are gone and the kernels of the previous
    batch, still in flight on the caller's stream, may have read them half-written (the fetches run on a side stream that does
    not wait for those kernels).  So from that moment every frame is copied on arrival -- what the reference does for every
    source (pyfvvdp/fvvdp.py:289-291) --, the overwritten frames are fetched again, and _SourceRecyclesBuffers makes the caller
    evaluate the previous batch again from intact copies (batch k-2 and older had finished before the fetch: back-pressure).
    The fetches run on a side stream that first waits for the caller's current stream, so frames produced asynchronously
    on that stream just before the call (GPU-generated video, non_blocking uploads) are complete when they are read."""

    preferred_batch = 64       # largest batch when the caller did not choose (see batch_schedule)

    @staticmethod
    def batch_schedule(n_out, max_batch):
        """Batch sizes when the caller did not choose: 8, 16, 32, ... up to max_batch.  The kernels cannot start before the
        first batch has been fetched, so the first batch is small; later batches are fetched while the previous one is
        computed, and large batches are cheaper per frame (fewer launches, less of the temporal window converted twice:
        4K x60, resident source: 5.6 ms with batches of 16, 4.7 ms with one batch of 60).  A short tail joins the last batch."""
        sizes, left, b = [], n_out, 8
        while left > 0:
            nb = min(b, max_batch, left)
            if left - nb < max(4, nb // 2):
                nb = left if left <= max_batch else nb
            sizes.append(nb)
            left -= nb
            b *= 2
        return sizes

    def __init__(self, metric, vs, width, height):
        self.m, self.vs, self.W, self.H = metric, vs, width, height
        self.dev = metric.device
        res = getattr(metric, "_feeder_res", None)     # side stream + events live as long as the metric object
        if res is None or res[0] != self.dev:
            res = (self.dev, torch.cuda.Stream(device=self.dev), torch.cuda.Event(), [torch.cuda.Event(), torch.cuda.Event()])
            metric._feeder_res = res
        self.side = res[1]
        self.frames = {}                  # source frame -> (test tensor, reference tensor, their addresses); fp32 luminance on the device
        self.prev_done = None             # kernels of the previous batch have finished reading their frames
        # events are reused (creating one costs as much as ten frame fetches): one for "frames fetched", two alternating
        # ones for "batch finished" (the older one is still being polled when the newer one is recorded)
        self.ev_ready, self.ev_done = res[2], res[3]
        self.n_batches = 0
        self.retired = []                 # tensors of frames that left the window: freed once their last reader has finished
        self.live_ptrs = {}               # address -> source frame, of every tensor in self.frames (aliasing detection)
        self.copy_mode = False            # the source reuses its buffers: clone on arrival
        self.recycled = False             # set by _buffer_reuse: the batch in flight may have read overwritten frames
        self.waited_main = False
        self.eotf = nat.Eotf()
        self.eotf.kind = nat.EOTF_NONE

    def _conform(self, x):
        dev, f32 = self.dev, torch.float32
        if not (type(x) is torch.Tensor and x.dtype is f32 and x.is_cuda and x.device == dev and x.is_contiguous()):
            x = torch.as_tensor(x).to(device=dev, dtype=f32).contiguous()
        if x.numel() != self.H * self.W:
            raise RuntimeError("get_*_frame must return one luminance frame of %dx%d pixels" % (self.W, self.H))
        return x

    def _fetch(self, f):
        """One source frame of both streams (the per-frame host cost of a user source: kept to a few attribute reads)."""
        t = self._conform(self.vs.get_test_frame(f, device=self.dev))
        if self.copy_mode:
            t = t.clone()
        r = self._conform(self.vs.get_reference_frame(f, device=self.dev))
        if self.copy_mode:
            r = r.clone()
        tp, rp = t.data_ptr(), r.data_ptr()
        if not self.copy_mode:
            if tp == rp or tp in self.live_ptrs or rp in self.live_ptrs:
                return self._buffer_reuse(f, t, r)
            self.live_ptrs[tp] = f
            self.live_ptrs[rp] = f
        return (t, r, tp, rp)

    def _buffer_reuse(self, f, t, r):
        """The source handed out an address that a frame still in the temporal window occupies (or one address for the test
        and the reference frame): it decodes into buffers it reuses.  The new frame is intact right now unless its two halves
        share the buffer (then it is fetched again, copying); the held frames at the same addresses are gone (fetched again
        and copied); every other held frame is still intact and is copied before a later fetch can overwrite it."""
        tp, rp = t.data_ptr(), r.data_ptr()
        hit = sorted({self.live_ptrs[p] for p in (tp, rp) if p in self.live_ptrs})
        self.copy_mode = True
        self.live_ptrs = {}
        self.recycled = True                             # __call__ raises once the bookkeeping is consistent again
        if tp == rp:
            t = r = None                                 # the reference fetch overwrote the test frame
        else:
            t, r = t.clone(), r.clone()
        for g in list(self.frames):
            if g not in hit:
                h = self.frames[g]
                tt, rr = h[0].clone(), h[1].clone()
                self.frames[g] = (tt, rr, tt.data_ptr(), rr.data_ptr())
        for g in hit:
            self.frames[g] = self._fetch(g)               # copy mode: cloned on arrival
        if t is None:
            return self._fetch(f)
        return (t, r, t.data_ptr(), r.data_ptr())

    def __call__(self, ctx, idx, taps, fl, n_out, oob, stream):
        uniq = sorted(set(int(f) for f in idx))
        main = torch.cuda.current_stream(self.dev)
        if self.n_batches >= 2:
            # Back-pressure and buffer safety in one: the host waits for the kernels of the batch before the previous one.
            # The GPU still has the previous batch queued (nothing starves), at most ~3 batches of frames are alive however
            # fast the source is, everything retired so far has no reader left, and a source that recycles a buffer of a
            # retired frame writes it after its last reader.
            self.ev_done[self.n_batches & 1].synchronize()
            self.retired.clear()
        with torch.cuda.stream(self.side):
            if not self.waited_main:
                # frames may have been produced asynchronously on the caller's stream just before the call
                self.side.wait_stream(main)
                self.waited_main = True
            fresh = [f for f in uniq if f not in self.frames]
            for f in fresh:
                self.frames[f] = self._fetch(f)
            ready = self.ev_ready
            ready.record(self.side)
        main.wait_event(ready)
        if self.recycled:
            # The frames just overwritten may have been inputs of the previous batch, whose kernels are not known to have
            # finished: hand control back so that batch is evaluated again (every frame held now is a private copy; the
            # copies were made on the side stream, which the caller's stream has just been made to wait for).
            self.recycled = False
            if self.n_batches >= 1:
                raise _SourceRecyclesBuffers()
        pos = {f: k for k, f in enumerate(uniq)}
        ridx = np.asarray([pos[int(f)] for f in idx], dtype=np.int32)
        held = [self.frames[f] for f in uniq]
        tp = (C.c_void_p * len(uniq))(*[h[2] for h in held])
        rp = (C.c_void_p * len(uniq))(*[h[3] for h in held])
        lib = nat.lib()
        rc = lib.fvvdp_temporal_channels_frames(
            ctx.handle, tp, rp, len(uniq), nat.FVVDP_F32, 1, 0, C.byref(self.eotf), None,
            ridx.ctypes.data_as(C.POINTER(C.c_int32)), nat.fptr(taps), fl, n_out, 0, C.c_void_p(oob.data_ptr()), stream)
        if rc == nat.FVVDP_EUNSUPPORTED:          # one array per stream, then the general entry point
            with torch.cuda.stream(self.side):
                bt = torch.stack([h[0].reshape(-1) for h in held])
                br = torch.stack([h[1].reshape(-1) for h in held])
                ready.record(self.side)
            main.wait_event(ready)
            for b in (bt, br):
                b.record_stream(main)
            nat.check(lib.fvvdp_temporal_channels(
                ctx.handle, C.c_void_p(bt.data_ptr()), C.c_void_p(br.data_ptr()), nat.FVVDP_F32, 1, 0, self.H * self.W,
                C.byref(self.eotf), None, ridx.ctypes.data_as(C.POINTER(C.c_int32)), nat.fptr(taps), fl, n_out, 0,
                C.c_void_p(oob.data_ptr()), stream))
        else:
            nat.check(rc)
        # The frames were allocated on the side stream and are read by kernels torch does not know about: they are kept
        # alive here until an event recorded AFTER their last reader has passed (cheaper than record_stream on every
        # tensor and batch: 184 calls on a 60-frame clip); release() covers the tensors still held when the call ends.
        keep = set(uniq)
        for f in [f for f in self.frames if f not in keep]:
            h = self.frames.pop(f)
            self.live_ptrs.pop(h[2], None)
            self.live_ptrs.pop(h[3], None)
            self.retired.append(h)                  # not in this batch's window: last read by the previous batch or earlier
        done = self.ev_done[self.n_batches & 1]
        self.n_batches += 1
        done.record(main)
        self.prev_done = done

    def release(self, synced):
        """End of the predict call.  After a host synchronisation nothing is in flight; otherwise (sync=False) the
        allocator is told that the main stream still reads the frames."""
        if not synced:
            main = torch.cuda.current_stream(self.dev)
            for held in list(self.frames.values()) + self.retired:
                held[0].record_stream(main)
                held[1].record_stream(main)
        self.frames.clear()
        self.retired.clear()
        self.live_ptrs = {}

