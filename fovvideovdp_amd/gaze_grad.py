"""Differentiable many-gaze JOD: fvvdp.jod_gazes and its autograd function (include/fvvdp_hip_gaze_grad.h).

The forward makes the launches of fvvdp.predict_gazes for a device-resident float clip (fvvdp_temporal_channels per frame
batch, fvvdp_bands_forward_gazes, the pooling of fvvdp_bands_forward_gazes_pool on the last batch) with arguments from the
same methods of the metric, so row g is bit-identical to it.  The backward of a loss sum_g w_g JOD_g shares among the gazes
everything that does not depend on the gaze: per backward batch one ingest and one map-writing pyramid pass (on the trace of
gaze 0; only its contrast and L_bkg maps are read), then fvvdp_gaze_grad_frames sums the layer gradients of all gazes and runs
the coarse-to-fine sweep and level 0 once, and after the last batch one fvvdp_video_grad_input applies the transpose of the
temporal filter and the display model's derivative.  Neither pass reads context scratch left by the other, and neither
synchronises with the host.  Setup, buffers and the map-writing pass are grad_passes.py's, as jod_video's."""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .display_model import native_geometry
from .gazes import _gaze_array
from .grad_passes import ClipBuffers, ClipSetup, _ptr, batches, grad_batch_size, workspace_bytes
from .image_grad import place
from .video_grad import GRAD_PLANES, clip_arguments

# Largest group of gazes one gaze_layer_kernel launch takes: 0 = the library's default (FVVDP_GAZE_GROUP_MAX = 8), or 1, 2, 4, 8.
# The gradient does not depend on it, bit for bit; smaller groups only make more launches (tests, A/B runs).
GROUP_MAX = 0


def _csf_tables(metric):
    """The two 32^3 CSF tables and their axes [3, 32] on the metric's device, plus the host copy of the axes: uploaded once per
    metric (and device, and set of tables) and kept.  Both temporal channels' tables must share their axes (the native context
    keeps one set as well): checked here."""
    key = (str(metric.device), tuple(id(l["S_log"]) for l in metric.csf_lut))
    have = metric.__dict__.get("_gaze_grad_tables")
    if have is None or have[0] != key:
        lut = metric.csf_lut
        ax = [np.ascontiguousarray(np.stack([np.asarray(lut[cc][k], dtype=np.float32).reshape(nat.LUT_N)
                                             for k in ("Y_log", "rho_log", "ecc_sqrt")])) for cc in range(2)]
        if not np.array_equal(ax[0], ax[1]):
            raise RuntimeError("jod_gazes: the CSF tables of the two temporal channels must have the same axes")
        axes = ax[1]
        s = [torch.from_numpy(np.ascontiguousarray(lut[cc]["S_log"], dtype=np.float32)).to(metric.device) for cc in range(2)]
        if any(tuple(t.shape) != (nat.LUT_N,) * 3 for t in s):
            raise RuntimeError("jod_gazes: the CSF tables must be %d^3" % nat.LUT_N)
        # the last element keeps the table arrays alive: the key holds their id(), which a freed array's successor could reuse
        have = (key, s[0], s[1], torch.from_numpy(axes).to(metric.device), axes, metric.csf_lut)
        metric._gaze_grad_tables = have
    return have[1:5]


def _forward(metric, t, r, fps, gaze):
    """JOD [G] and Q_per_ch [G, n_bands, 2, N] on the device: the launches of predict_gazes, no flag read back."""
    s = ClipSetup(metric, t, fps, r)
    N, dev, G = s.N, metric.device, gaze.shape[0]
    nq = s.n_bands * 2 * N
    res = torch.zeros(G * nq + 1 + G, dtype=torch.float32, device=dev)      # Q_per_ch | range flag | JOD, as predict_gazes lays it out
    Q = res[:G * nq].view(G, s.n_bands, 2, N)
    oob = res[G * nq:G * nq + 1].view(torch.int32)
    jod = res[G * nq + 1:]
    lib = nat.lib()
    nbytes = workspace_bytes(lib.fvvdp_gaze_workspace, s.W, s.H, s.n_bands, G, min(s.batch, N))
    work = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    geom = metric._geom_struct()
    for b0, nb in batches(N, s.batch):
        s.ingest(lib, t, r, b0, nb, oob)
        common = (s.ctx.handle, nb, G, _ptr(gaze, 8 * b0), 2 * N, _ptr(Q), N, b0, C.byref(geom), _ptr(work), nbytes)
        if b0 + nb == N:
            nat.check(lib.fvvdp_bands_forward_gazes_pool(*common, C.byref(s.pp), _ptr(jod), s.stream))
        else:
            nat.check(lib.fvvdp_bands_forward_gazes(*common, s.stream))
    return jod, Q


def _backward(metric, t, r, fps, gaze, fix0, Q, gamma):
    """sum_g gamma[g] * dJOD_g/dt for the contiguous device clip t [1, C, N, H, W]."""
    s = ClipSetup(metric, t, fps, r)
    N, dev, G = s.N, metric.device, gaze.shape[0]
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, GRAD_PLANES)
    lib = nat.lib()
    buf = ClipBuffers("jod_gazes", metric, s, t, gb, workspace_bytes(lib.fvvdp_gaze_grad_workspace, s.W, s.H, s.n_bands, gb, G))
    lut0, lut1, d_axes, h_axes = _csf_tables(metric)
    prm, geom = s.params(), metric._geom_struct()
    rho = np.ascontiguousarray(s.rho_band, dtype=np.float64)
    gamma = gamma.to(device=dev, dtype=torch.float32).reshape(G).contiguous()
    for b0, nb in batches(N, gb):
        buf.maps_pass(lib, metric, s, t, r, fix0, b0, nb)                      # on the trace of gaze 0: only gaze-invariant maps are read
        nat.check(lib.fvvdp_gaze_grad_frames(s.W, s.H, s.n_bands, nb, G, int(GROUP_MAX), C.byref(prm), C.byref(s.pp),
                                             C.byref(geom), rho.ctypes.data_as(C.POINTER(C.c_double)), _ptr(lut0), _ptr(lut1),
                                             _ptr(d_axes), nat.fptr(h_axes), _ptr(gaze, 8 * b0), 2 * N, _ptr(Q), N, b0,
                                             _ptr(gamma), buf.maps.maps_arr, _ptr(buf.g0), _ptr(buf.work), buf.work_bytes, s.stream))
    return buf.input_grad(lib, s, t)


class JodGazesFunction(torch.autograd.Function):
    """test [1, C, N, H, W] (contiguous float32, float16 or bfloat16 on the metric's device), reference (the same, constant), gaze [G, N, 2] (device)
    -> JOD [G]."""

    @staticmethod
    def forward(ctx, test, reference, metric, fps, gaze, fix0):
        with torch.cuda.device(metric.device):
            jod, Q = _forward(metric, test, reference, fps, gaze)
        ctx.metric, ctx.fps, ctx.fix0 = metric, fps, fix0
        ctx.save_for_backward(test, reference, gaze, Q)
        return jod.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_jod):
        test, reference, gaze, Q = ctx.saved_tensors
        grad = None
        if ctx.needs_input_grad[0]:
            with torch.cuda.device(ctx.metric.device):
                grad = _backward(ctx.metric, test, reference, ctx.fps, gaze, ctx.fix0, Q, grad_jod)
        return grad, None, None, None, None, None


def jod_gazes(metric, test, reference, fixation_points, dim_order="BCFHW", frames_per_second=0):
    """fvvdp.jod_gazes (see there)."""
    if not metric.foveated:
        raise RuntimeError("jod_gazes needs a foveated metric (fvvdp(foveated=True)): without foveation the gaze does not "
                           "enter the result, use jod_video()")
    if metric.do_heatmap:
        raise RuntimeError("jod_gazes makes no heat maps: build the metric without heatmap=")
    if native_geometry(metric.display_geometry) is None:
        raise RuntimeError("jod_gazes covers the stock display geometry; a user display_geometry class takes jod_video(), one "
                           "gaze per call")
    t, r = clip_arguments("jod_gazes", metric, test, reference, dim_order, frames_per_second)
    fix = _gaze_array(metric, fixation_points, t.shape[4], t.shape[3], t.shape[2])
    t, r = place(metric, t, r)
    gaze = torch.from_numpy(fix).to(metric.device)                            # [G, N, 2], uploaded once
    return JodGazesFunction.apply(t, r, metric, float(frames_per_second), gaze, fix[0])
