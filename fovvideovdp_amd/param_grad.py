"""Gradients of the JOD with respect to the model parameters: fvvdp.calibration_jod_images / calibration_jod_video, the
parameter vector behind them and their autograd function (include/fvvdp_hip_params.h).

The twelve parameters of PARAMETER_NAMES enter the metric after the pyramid: six pointwise in the masking model of every band
pixel, six in do_pooling_and_jods.  A call evaluates the metric under a vector `theta` on the metric's ordinary native context,
whose model constants are replaced for the duration of the call (fvvdp_ctx_set_params) and restored in a `finally`: the metric's
attributes are never touched, no context is created.  The forward makes the launches of predict_images / predict with constants
converted from theta exactly as native_params() and _pool_params() convert the attributes, so the JOD is bit-identical to that
of a metric whose attributes hold theta.  When theta needs a gradient the forward also re-runs the pyramid pass with every
band's maps written, per backward batch of frames (grad_passes.grad_batch_size), and fvvdp_param_sums reduces the maps to five
sums per (band, temporal channel, frame); only Q_per_ch and the sums are kept.  backward() is `chain` alone: float64 tensor
operations on [bands, 2, frames] arrays.

Not part of the vector: k_cm and csf_sigma (they select a precomputed CSF table), filter_len (an integer) and the enumerated
model variants.

sustained_sigma and sustained_beta (TEMPORAL_PARAMETER_NAMES) are a vector of their own, `phi`, that calibration_jod_video takes
as temporal=: they enter only through the taps of the temporal filters, which are a per-call argument of the ingest, so the
clip is evaluated under taps made from phi (fvvdp.temporal_filters, the expressions of get_temporal_filters).  When phi needs a
gradient, every backward batch also makes the two level-0 backward passes of jod_video(wrt="both") with gamma = 1 from the same
maps (slope planes on), the luminance of the source frames under the batch's windows (fvvdp_luminance_frames) and the
tap-gradient kernel (fvvdp_tap_grad, include/fvvdp_hip_taps.h); the batches' dJOD/dtaps [2, fl] are added in frame order in
float64 and are all that is kept.  backward() is `tap_chain`: the float64 Jacobian of the taps with respect to phi.
The setups (with theta's constants and phi's taps), both forward loops, the map-writing passes, the buffers with their memory
check and the level-0 backward are grad_passes.py's, shared with the other differentiable entry points; what is here is the
vectors, the two chains, the sums (_Sums) and the tap gradient's own buffers and kernel (_TapGrad)."""
import ctypes as C
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .fvvdp import _image_stack, filter_length, fvvdp as _fvvdp, temporal_filters
from .grad_passes import (ClipBuffers, ImageSetup, Maps, PlanClipSetup, _apply, _ptr, _refuse, batches, forward_clip,
                          forward_images, grad_batch_size, level0_backward, vector_values, work_tensor, workspace,
                          workspace_bytes)
from .video_grad import video_grad_planes
from .video_source import fvvdp_video_source_array

PARAMETER_NAMES = _fvvdp.PARAMETER_NAMES
TEMPORAL_PARAMETER_NAMES = _fvvdp.TEMPORAL_PARAMETER_NAMES
K2 = 0.062170507756932                   # scale of the transient filter (get_temporal_filters)
_IDX = {name: i for i, name in enumerate(PARAMETER_NAMES)}
_POSITIVE = ("beta", "beta_sch", "beta_tch", "beta_t", "mask_p")
LN10 = math.log(10.0)


def parameter_tensor(metric):
    """The metric's current values of PARAMETER_NAMES as a 1-D float64 host tensor."""
    return torch.tensor([float(getattr(metric, name)) for name in PARAMETER_NAMES], dtype=torch.float64)


def set_parameters(metric, theta):
    """Writes a vector laid out as PARAMETER_NAMES into the metric's attributes (what load_config sets); the next call builds
    its native context from them."""
    vals = theta_values(theta)
    for name, v in zip(PARAMETER_NAMES, vals):
        setattr(metric, name, v)
    metric._drop_context()


def theta_values(theta):
    """theta (a 1-D tensor or sequence of len(PARAMETER_NAMES) values) -> list of Python floats; refuses what the metric cannot
    be evaluated under.  A host tensor is read without touching the GPU."""
    vals = vector_values("theta", "PARAMETER_NAMES", theta)
    for name in _POSITIVE:
        if not vals[_IDX[name]] > 0:
            raise RuntimeError("theta: %s must be positive (an exponent of the model), got %g" % (name, vals[_IDX[name]]))
    if vals[_IDX["jod_a"]] == 0:
        raise RuntimeError("theta: jod_a must not be 0 (the JOD would not depend on the images)")
    return vals


def temporal_parameter_tensor(metric):
    """The metric's current values of TEMPORAL_PARAMETER_NAMES as a 1-D float64 host tensor."""
    return torch.tensor([float(getattr(metric, name)) for name in TEMPORAL_PARAMETER_NAMES], dtype=torch.float64)


def set_temporal_parameters(metric, phi):
    """Writes a vector laid out as TEMPORAL_PARAMETER_NAMES into the metric's attributes, as Python floats.  The taps are an
    argument of every call: the native context stays."""
    for name, v in zip(TEMPORAL_PARAMETER_NAMES, phi_values(phi)):
        setattr(metric, name, v)


def phi_values(phi):
    """phi (a 1-D tensor or sequence of the 2 values of TEMPORAL_PARAMETER_NAMES) -> list of Python floats; refuses what no
    temporal filter can be made from.  A host tensor is read without touching the GPU."""
    vals = vector_values("temporal", "TEMPORAL_PARAMETER_NAMES", phi)
    for name, v in zip(TEMPORAL_PARAMETER_NAMES, vals):
        if not v > 0:
            raise RuntimeError("temporal: %s must be positive (a width and a time of the log-Gaussian filter), got %g" % (name, v))
    return vals


def taps_jacobian(fps, fl, sigma, beta):
    """(taps [2, fl], d taps / d(sigma, beta) [2, fl, 2]) in float64, by hand.
    F0 = e / sum e with e_k = exp(-(ln(t_k + 1e-4) - ln beta)^2 / (2 sigma^2)), t = linspace(0, fl / fps, fl);
    F1_k = K2 (F0_{k+1} - F0_k) / dt for k < fl - 1 and F1_{fl-1} = 0, a constant: its derivative is exactly 0.
    With d = ln(t + 1e-4) - ln beta:  dln e / dsigma = d^2 / sigma^3,  dln e / dbeta = d / (sigma^2 beta), and
    dF0_k / dp = F0_k (a_k - sum_j F0_j a_j) for a = dln e / dp."""
    t = torch.linspace(0.0, fl / fps, fl, dtype=torch.float64)
    d = torch.log(t + 1e-4) - math.log(beta)
    e = torch.exp(-d * d / (2.0 * sigma * sigma))
    F0 = e / e.sum()
    a = torch.stack([d * d / sigma ** 3, d / (sigma * sigma * beta)], dim=1)          # [fl, 2]
    dF0 = F0[:, None] * (a - (F0[:, None] * a).sum(0, keepdim=True))
    F = torch.zeros((2, fl), dtype=torch.float64)
    J = torch.zeros((2, fl, 2), dtype=torch.float64)
    F[0], J[0] = F0, dF0
    if fl > 1:
        dt = t[1] - t[0]
        F[1, :-1] = K2 * (F0[1:] - F0[:-1]) / dt
        J[1, :-1] = K2 * (dF0[1:] - dF0[:-1]) / dt
    return F, J


def tap_chain(dtaps, fps, fl, sigma, beta):
    """dJOD/dphi [2] float64 from dJOD/dtaps [2, fl] (any device and float dtype)."""
    _, J = taps_jacobian(fps, fl, sigma, beta)
    return (dtaps.to(device="cpu", dtype=torch.float64)[:, :, None] * J).sum(dim=(0, 1))


def native_params_of(vals):
    """fvvdp_params for the values `vals`: the conversions of fvvdp.native_params (mask_k is the fp32 pow(10, mask_c))."""
    v = dict(zip(PARAMETER_NAMES, vals))
    p = nat.Params()
    p.mask_p = v["mask_p"]
    p.mask_q[0], p.mask_q[1] = v["mask_q_sust"], v["mask_q_trans"]
    p.mask_k = float(torch.pow(torch.tensor(10.0), torch.tensor(v["mask_c"])))
    p.beta = v["beta"]
    p.sens_gain = 10.0 ** (v["sensitivity_correction"] / 20.0)
    p.lbkg_min, p.contrast_max, p.d_max = 0.1, 1000.0, 1e4
    return p


def pool_params_of(vals):
    """fvvdp_pool_params for the values `vals`: the conversions of fvvdp._pool_params."""
    v = dict(zip(PARAMETER_NAMES, vals))
    return nat.PoolParams(v["beta_sch"], v["beta_tch"], v["beta_t"], v["w_transient"], v["jod_a"],
                          float(10.0 ** v["log_jod_exp"]))


# ---- the chain: Q_per_ch and the sums -> dJOD/dtheta ---------------------------------------------------------------------
def _lp(x, p, dim, mean):
    """y = (sum x^p [/ n])^(1/p) along `dim` (kept) for x >= 0, with G = dy/dx and the terms t of dy/dp = sum_dim t.
    dy/dp = y / p sum_i w_i (ln x_i - ln y), w_i = x_i^p / sum x^p: zero entries contribute exact zeros (never 0^(p-1) 0), and a
    norm over one entry is the identity, whose derivative with respect to p is exactly 0."""
    n = x.shape[dim]
    if n == 1:
        return x, torch.ones_like(x), torch.zeros_like(x)
    xp = x.pow(p)
    S = xp.sum(dim, keepdim=True)
    y = (S / n if mean else S).pow(1.0 / p)
    ok = (x > 0) & (y > 0)
    one = torch.ones_like(x)
    sx, sy, sS = torch.where(ok, x, one), torch.where(y > 0, y, torch.ones_like(y)), torch.where(S > 0, S, torch.ones_like(S))
    zero = torch.zeros_like(x)
    G = torch.where(ok, (sx / sy).pow(p - 1.0), zero) / (n if mean else 1)
    t = torch.where(ok, y / p * (xp / sS) * (sx.log() - sy.log()), zero)
    return y, G, t


def chain(Q, sums, npx, vals, n_channels, per_column, with_scale=False):
    """dJOD/dtheta from what the forward kept.
    Q [bands, 2, F] (the forward's Q_per_ch), sums [bands, 2, F, 5] (fvvdp_param_sums), npx [bands] (pixels per band), on one
    device, any float dtype (computed in float64); vals: the parameter values; n_channels: 1 (still images: the transient
    channel does not exist) or 2.  per_column True: the F columns are F still images, each with its own JOD -> [F, 12]; False:
    the F frames of one clip -> [1, 12].  with_scale: also the sum of the absolute per-(band, channel, frame) terms of every
    entry, the yardstick a comparison against finite differences is relative to.
    With m = mean D^beta = Q^beta and n pixels:  dQ/dmask_p = Q/(n m) s1,  dQ/dmask_q = -Q/(n m) s2 (its own channel),
    dQ/dmask_c = -Q/(n m) q ln10 s3,  dQ/dsensitivity_correction = Q/(n m) (p s0 - q s3) ln10/20,
    dQ/dbeta = Q (-ln m / beta^2 + s4 / (n beta m)); everything 0 where Q = 0.  The pooling stage is do_pooling_and_jods
    differentiated by hand (JOD = jod_a Q_all^beta_jod + 10)."""
    v = dict(zip(PARAMETER_NAMES, vals))
    Cn = n_channels
    Q = Q.to(torch.float64)[:, :Cn]
    s = sums.to(torch.float64)[:, :Cn]
    nb, _, F = Q.shape
    n = npx.to(device=Q.device, dtype=torch.float64).view(nb, 1, 1)
    p, beta = v["mask_p"], v["beta"]
    qv = Q.new_empty((1, Cn, 1))
    w = Q.new_ones((1, Cn, 1))
    qv[:, 0] = v["mask_q_sust"]
    if Cn == 2:
        qv[:, 1] = v["mask_q_trans"]
        w[:, 1] = v["w_transient"]
    zero = torch.zeros_like(Q)
    posQ = Q > 0
    sQ = torch.where(posQ, Q, torch.ones_like(Q))
    m = sQ.pow(beta)
    inv = torch.where(posQ, sQ / (n * m), zero)
    s0, s1, s2, s3, s4 = (s[..., j] for j in range(5))
    dQ = {"mask_p": inv * s1,
          "mask_q": -inv * s2,
          "mask_c": -inv * qv * LN10 * s3,
          "sensitivity_correction": inv * (p * s0 - qv * s3) * (LN10 / 20.0),
          "beta": torch.where(posQ, sQ * (-m.log() / beta ** 2 + s4 / (n * beta * m)), zero)}

    X = Q * w
    Qsc, G1, t1 = _lp(X, v["beta_sch"], 0, False)                 # [1, C, F]
    Qtc, G2, t2 = _lp(Qsc, v["beta_tch"], 1, False)               # [1, 1, F]
    if per_column:
        Qall, G3, t3 = Qtc, torch.ones_like(Qtc), torch.zeros_like(Qtc)
    else:
        Qall, G3, t3 = _lp(Qtc, v["beta_t"], 2, True)             # [1, 1, 1]
    bj = 10.0 ** v["log_jod_exp"]
    a = v["jod_a"]
    pos = Qall > 0
    sq = torch.where(pos, Qall, torch.ones_like(Qall))
    Qb = torch.where(pos, sq.pow(bj), torch.zeros_like(Qall))
    dJ = torch.where(pos, a * bj * sq.pow(bj - 1.0), torch.zeros_like(Qall))
    g3 = dJ * G3                                                   # dJOD/dQ_tc [1, 1, F]
    g2 = g3 * G2                                                   # dJOD/dQ_sc [1, C, F]
    g1 = g2 * G1                                                   # dJOD/d(w Q) [bands, C, F]
    gQ = g1 * w
    terms = [None] * len(PARAMETER_NAMES)
    terms[_IDX["mask_p"]] = gQ * dQ["mask_p"]
    tq = gQ * dQ["mask_q"]
    terms[_IDX["mask_q_sust"]] = tq[:, 0:1]
    terms[_IDX["mask_q_trans"]] = tq[:, 1:2] if Cn == 2 else zero[:, 0:1]
    terms[_IDX["mask_c"]] = gQ * dQ["mask_c"]
    terms[_IDX["sensitivity_correction"]] = gQ * dQ["sensitivity_correction"]
    terms[_IDX["beta"]] = gQ * dQ["beta"]
    terms[_IDX["beta_sch"]] = g2 * t1
    terms[_IDX["beta_tch"]] = g3 * t2
    terms[_IDX["beta_t"]] = dJ * t3
    terms[_IDX["w_transient"]] = (g1 * Q)[:, 1:2] if Cn == 2 else zero[:, 0:1]
    terms[_IDX["jod_a"]] = Qb
    terms[_IDX["log_jod_exp"]] = torch.where(pos, a * Qb * sq.log() * (bj * LN10), torch.zeros_like(Qall))

    def total(t):
        return t.sum(dim=(0, 1)).expand(F) if per_column else t.sum().reshape(1)

    J = torch.stack([total(t) for t in terms], dim=1)             # [F or 1, 12]
    if not with_scale:
        return J
    return J, torch.stack([total(t.abs()) for t in terms], dim=1)


# ---- the forward under theta ------------------------------------------------------------------------------------------
class _UnderTheta:
    """The metric's ordinary native context with theta's constants for the length of a `with` block."""

    def __init__(self, metric, ctx, prm):
        self.metric, self.ctx, self.prm = metric, ctx, prm

    def __enter__(self):
        nat.check(nat.lib().fvvdp_ctx_set_params(self.ctx.handle, C.byref(self.prm)))
        return self

    def __exit__(self, *exc):
        own = self.metric.native_params()
        nat.check(nat.lib().fvvdp_ctx_set_params(self.ctx.handle, C.byref(own)))
        return False


class _Sums:
    """Maps, workspace and result of fvvdp_param_sums for backward batches of up to gb slots of a W x H pyramid; `total` slots
    (frames of the clip, or image pairs) in all."""

    def __init__(self, metric, W, H, n_bands, planes, gb, total):
        dev = metric.device
        self.W, self.H, self.n_bands, self.planes, self.gb = W, H, n_bands, planes, gb
        self.maps = Maps(metric, W, H, n_bands, planes, gb)
        self.maps_arr, self.q_scratch = self.maps.maps_arr, self.maps.q_scratch              # (tools read them here)
        self.work_bytes, self.work = workspace(nat.lib().fvvdp_param_sums_workspace, W, H, n_bands, gb, dtype=torch.float64)
        self.batch_sums = torch.empty((n_bands, 2, gb, nat.PARAM_SUMS), dtype=torch.float64, device=dev)
        self.sums = torch.empty((n_bands, 2, total, nat.PARAM_SUMS), dtype=torch.float64, device=dev)
        self.npx = torch.tensor([float(w * h) for w, h in metric._level_sizes(W, H, n_bands)[:n_bands]], dtype=torch.float64)

    def reduce(self, prm, b0, nb, stream):
        """The maps of the nb slots just written -> columns [b0, b0 + nb) of self.sums."""
        out = self.batch_sums.view(-1)[:self.n_bands * 2 * nb * nat.PARAM_SUMS].view(self.n_bands, 2, nb, nat.PARAM_SUMS)
        nat.check(nat.lib().fvvdp_param_sums(self.W, self.H, self.n_bands, nb, self.planes, C.byref(prm), self.maps_arr,
                                             _ptr(out), _ptr(self.work), self.work_bytes, stream))
        self.sums[:, :, b0:b0 + nb] = out

    def drop_maps(self):
        """The maps are transient: only Q and the sums outlive the forward."""
        self.maps = self.maps_arr = self.q_scratch = None


def _images_forward(metric, t, r, fix, vals, want_sums):
    """The launches of fvvdp._predict_image_group (no heat maps, no flags read back) under theta -> (JOD [B], Q [bands, 2, B],
    _Sums or None).  t, r: [B, C, H, W] on any device."""
    if t.dtype != r.dtype:
        t, r = metric._to_unit_float(t), metric._to_unit_float(r)
    s = ImageSetup(metric, t.to(metric.device).contiguous(), r.to(metric.device).contiguous(),
                   prm=native_params_of(vals), pp=pool_params_of(vals))
    sums = None
    with _UnderTheta(metric, s.ctx, s.prm):
        jod, Q = forward_images(s, fix)
        if want_sums:
            gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, 7)
            sums = _Sums(metric, s.W, s.H, s.n_bands, 2, gb, s.B)
            for b0, nb in batches(s.B, gb):
                s.write_maps(sums.maps, fix, b0, nb)
                sums.reduce(s.prm, b0, nb, s.stream)
            sums.drop_maps()
    return jod, Q, sums


class _TapGrad:
    """What the tap gradient of the clip of the setup s holds beside a backward's buffers, in backward batches of up to gb: the
    luminance frames under a batch's windows, workspace and result of fvvdp_tap_grad, and the running dJOD/dtaps [2, fl]
    (float64, added in frame order).  self.buf: the grad_passes.ClipBuffers of the two level-0 backward passes (clip-long
    gradients of both sides, their workspaces, maps and slope planes), whose memory check covers all of this."""

    def __init__(self, metric, s, gb, with_scale=False):
        dev, HW, lib = metric.device, s.H * s.W, nat.lib()
        vb = workspace_bytes(lib.fvvdp_video_grad_workspace, s.W, s.H, s.n_bands, gb)
        rb = workspace_bytes(lib.fvvdp_ref_grad_workspace, s.W, s.H, s.n_bands, gb, 2)
        self.tap_bytes = workspace_bytes(lib.fvvdp_tap_grad_workspace, s.W, s.H, s.fl)
        n_lum = min(s.N, s.fl - 1 + gb)
        lum_bytes = 2 * n_lum * HW * 4
        self.s = s
        self.buf = ClipBuffers("calibration_jod_video", metric, s, None, gb, vb, True, rb, results=False, head=False, maps=False,
                               extra_bytes=self.tap_bytes + lum_bytes, lum_bytes=lum_bytes)
        self.lum = torch.empty((2, n_lum, s.H, s.W), dtype=torch.float32, device=dev)
        self.tap_work = work_tensor(self.tap_bytes, torch.float64)
        self.out = torch.empty((2, s.fl), dtype=torch.float64, device=dev)
        self.dtaps = torch.zeros((2, s.fl), dtype=torch.float64, device=dev)
        self.gamma = torch.ones(1, dtype=torch.float32, device=dev)
        self.scale = torch.zeros((2, s.fl), dtype=torch.float64, device=dev) if with_scale else None

    def batch(self, prm, Q, b0, nb):
        """The maps of output frames [b0, b0 + nb) (slope planes included) -> their share of dJOD/dtaps, added to self.dtaps."""
        s, buf = self.s, self.buf
        W, H, HW, fl = s.W, s.H, s.H * s.W, s.fl
        level0_backward(buf, s, prm, Q, s.N, b0, nb, self.gamma)
        idx = s.widx[b0:b0 + fl - 1 + nb]                  # the batch's window list: fl - 1 + nb source frames, oldest first
        frames = np.unique(idx)
        nu = len(frames)
        pos = np.ascontiguousarray(np.searchsorted(frames, idx), dtype=np.int32)
        lum = self.lum.view(-1)[:2 * nu * HW]
        s.feeder.luminance(frames, lum, buf.oob, s.stream)
        nat.check(nat.lib().fvvdp_tap_grad(W, H, nb, fl, _ptr(buf.g0, b0 * 2 * HW * 4), _ptr(buf.g0_r, b0 * 2 * HW * 4), _ptr(lum),
                                           _ptr(lum, nu * HW * 4), pos.ctypes.data_as(C.POINTER(C.c_int32)), nu, _ptr(self.out),
                                           _ptr(self.tap_work), self.tap_bytes, s.stream))
        self.dtaps += self.out
        if self.scale is not None:
            # the yardstick of the kernel's rounding: sum |g0 Y| per entry, with torch, in float64
            widx = torch.as_tensor(pos.astype(np.int64), device=self.out.device)
            t = torch.arange(nb, device=self.out.device)
            for k in range(fl):
                q = widx[t + fl - 1 - k]
                for g, y in ((buf.g0, self.lum.view(-1)[:nu * HW].view(nu, H, W)),
                             (buf.g0_r, self.lum.view(-1)[nu * HW:2 * nu * HW].view(nu, H, W))):
                    self.scale[:, k] += (g[b0:b0 + nb].abs().double() * y[q].double()[:, None].abs()).sum(dim=(0, 2, 3))


def _video_pass(metric, vs, fixation_point, vals, want_sums, pvals=None, want_taps=False, with_scale=False):
    """The launches of fvvdp._predict_on_device (sync=False, no heat maps) under theta -> (JOD 0-d, Q [bands, 2, N], _Sums or
    None, number of temporal channels, dJOD/dtaps [2, fl] float64 or None).  pvals: the values of TEMPORAL_PARAMETER_NAMES the
    taps are made from (None: the metric's own taps); want_taps: also the gradient of the JOD with respect to the taps."""
    height, width, N = vs.get_video_size()
    fix = metric._fixation(fixation_point, width, height, N) if metric.foveated else None
    pl = metric._clip_plan(vs)
    PlanClipSetup.refuse_user_photometry("calibration_jod_video", pl)
    taps = None
    if pvals is not None:
        if pl.planes != 4:
            raise RuntimeError("calibration_jod_video: temporal= needs a clip of at least 2 frames (a single frame has no "
                               "temporal filter)")
        # the taps under phi: never cached (an optimiser makes a new phi per step), never written to the metric
        taps = np.ascontiguousarray(temporal_filters(vs.get_frames_per_second(), pl.fl, pvals[0], pvals[1]).numpy(), dtype=np.float32)
    s = PlanClipSetup("calibration_jod_video", metric, pl, native_params_of(vals), pool_params_of(vals), taps)
    sums = dtaps = None
    with _UnderTheta(metric, s.ctx, s.prm):
        jod, Q = forward_clip(s, fix)
        if want_taps or want_sums:
            # one ingest and one map-writing pass per backward batch; for the taps with the slope planes on, as
            # jod_video(wrt="both"): theta's sums and the two level-0 backward passes read the same maps
            gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch,
                                 video_grad_planes("both") if want_taps else (9 if s.planes == 4 else 7))
            if want_taps:
                gb = max(1, min(gb, nat.TAPS_MAX_POSITIONS - (s.fl - 1)))
            tg = _TapGrad(metric, s, gb, with_scale) if want_taps else None
            sums = _Sums(metric, s.W, s.H, s.n_bands, s.planes, gb, N)
            if tg:
                tg.buf.use_maps(sums.maps)                 # (made last, as the sums' maps always were: the allocator's order)
            flag = tg.buf.oob if tg else torch.zeros(1, dtype=torch.int32, device=metric.device)
            for b0, nb in batches(N, gb):
                s.write_maps(sums.maps, fix, b0, nb, flag)
                if want_sums:
                    sums.reduce(s.prm, b0, nb, s.stream)
                if tg:
                    tg.batch(s.prm, Q, b0, nb)
            sums.drop_maps()
            if not want_sums:
                sums = None
            if tg:
                dtaps = (tg.dtaps, tg.scale) if with_scale else tg.dtaps
    return jod, Q, sums, s.planes // 2, dtaps


def _video_forward(metric, vs, fixation_point, vals, want_sums):
    """_video_pass under the metric's own temporal filters -> (JOD 0-d, Q [bands, 2, N], _Sums or None, temporal channels)."""
    return _video_pass(metric, vs, fixation_point, vals, want_sums)[:4]


def tap_gradient(metric, test, reference, theta, temporal, dim_order="BCFHW", frames_per_second=0, fixation_point=None,
                 with_scale=False):
    """dJOD/dtaps [2, fl] (float64, on the metric's device) of one clip under theta and phi: what the forward of
    calibration_jod_video keeps when phi requires grad.  For tests and tools.  with_scale: also sum |g0 Y| of every entry, the
    yardstick of the tap-gradient kernel's rounding (include/fvvdp_hip_taps.h), made with torch."""
    vals, pvals = theta_values(theta), phi_values(temporal)
    vs = fvvdp_video_source_array(test, reference, frames_per_second, dim_order=dim_order,
                                  display_photometry=metric.display_photometry, color_space_name=metric.color_space)
    metric._check_device()
    with torch.cuda.device(metric.device):
        return _video_pass(metric, vs, fixation_point, vals, False, pvals, True, with_scale)[4]


class _CalibrationFunction(torch.autograd.Function):
    """theta -> JOD ([B] for images, 0-d for a clip).  `run(want_sums)` makes the forward under theta's values."""

    @staticmethod
    def forward(ctx, theta, metric, run, vals, per_column):
        want = bool(ctx.needs_input_grad[0])
        with torch.cuda.device(metric.device):
            jod, Q, sums, channels = run(want)
        if want:
            ctx.vals, ctx.channels, ctx.per_column, ctx.npx = vals, channels, per_column, sums.npx
            ctx.theta_device, ctx.theta_dtype = theta.device, theta.dtype
            ctx.save_for_backward(Q, sums.sums)
        return jod.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_jod):
        Q, sums = ctx.saved_tensors
        J = chain(Q, sums, ctx.npx, ctx.vals, ctx.channels, ctx.per_column)               # [K, 12] float64
        g = grad_jod.to(device=J.device, dtype=torch.float64).reshape(-1, 1)
        grad = (g * J).sum(0)
        return grad.to(device=ctx.theta_device, dtype=ctx.theta_dtype), None, None, None, None


class _TemporalCalibrationFunction(torch.autograd.Function):
    """(theta, phi) -> the JOD of a clip.  `run(want_sums, want_taps)` makes the forward under their values; dJOD/dtaps does
    not depend on the upstream gradient, so the forward forms it and keeps [2, fl] values."""

    @staticmethod
    def forward(ctx, theta, phi, metric, vals, run, tap_args):
        want_theta, want_phi = bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])
        with torch.cuda.device(metric.device):
            jod, Q, sums, channels, dtaps = run(want_theta, want_phi)
        ctx.want_theta, ctx.want_phi, ctx.tap_args = want_theta, want_phi, tap_args
        ctx.phi_device, ctx.phi_dtype = phi.device, phi.dtype
        keep = []
        if want_theta:
            ctx.vals, ctx.channels, ctx.npx = vals, channels, sums.npx
            ctx.theta_device, ctx.theta_dtype = theta.device, theta.dtype
            keep += [Q, sums.sums]
        if want_phi:
            keep.append(dtaps)
        ctx.save_for_backward(*keep)
        return jod.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_jod):
        saved = list(ctx.saved_tensors)
        g_theta = g_phi = None
        if ctx.want_theta:
            Q, sums = saved[0], saved[1]
            J = chain(Q, sums, ctx.npx, ctx.vals, ctx.channels, False)
            g = grad_jod.to(device=J.device, dtype=torch.float64).reshape(-1, 1)
            g_theta = (g * J).sum(0).to(device=ctx.theta_device, dtype=ctx.theta_dtype)
        if ctx.want_phi:
            J = tap_chain(saved[-1], *ctx.tap_args)                                         # [2] float64, host
            g_phi = (grad_jod.to(device="cpu", dtype=torch.float64).reshape(()) * J).to(device=ctx.phi_device, dtype=ctx.phi_dtype)
        return g_theta, g_phi, None, None, None, None


def calibration_jod_images(metric, test, reference, theta, dim_order="BCHW", fixation_point=None):
    """fvvdp.calibration_jod_images (see there)."""
    vals = theta_values(theta)
    _refuse("calibration_jod_images", "the model parameters", metric, test, reference, "jod_images")
    t, r = _image_stack(test, reference, dim_order)
    metric._check_device()
    fix = metric._fixation(fixation_point, t.shape[3], t.shape[2], t.shape[0]) if metric.foveated else None

    def run(want_sums):
        jod, Q, sums = _images_forward(metric, t, r, fix, vals, want_sums)
        return jod, Q, sums, 1

    return _apply(_CalibrationFunction, metric, theta, run, vals, True)


def calibration_jod_video(metric, test, reference, theta, dim_order="BCFHW", frames_per_second=0, fixation_point=None,
                          temporal=None):
    """fvvdp.calibration_jod_video (see there)."""
    vals = theta_values(theta)
    pvals = None if temporal is None else phi_values(temporal)
    phi_grad = isinstance(temporal, torch.Tensor) and temporal.requires_grad and torch.is_grad_enabled()
    if phi_grad and frames_per_second > 0 and filter_length(frames_per_second) > nat.VIDEO_GRAD_MAX_TAPS:
        raise RuntimeError("calibration_jod_video: frame rate too high for the gradient of the temporal parameters: the temporal "
                           "filter has %d taps, the tap-gradient kernel covers %d (256 frames per second); the forward runs "
                           "with a temporal= that does not require grad"
                           % (filter_length(frames_per_second), nat.VIDEO_GRAD_MAX_TAPS))
    _refuse("calibration_jod_video", "the model parameters", metric, test, reference, "jod_video")
    d = dim_order.upper()
    if "B" in d and len(d) == len(test.shape) and test.shape[d.index("B")] != 1:
        raise RuntimeError("calibration_jod_video takes one clip per call (B must be 1)")
    vs = fvvdp_video_source_array(test, reference, frames_per_second, dim_order=dim_order,
                                  display_photometry=metric.display_photometry, color_space_name=metric.color_space)
    metric._check_device()

    if temporal is None:
        def run(want_sums):
            return _video_forward(metric, vs, fixation_point, vals, want_sums)

        return _apply(_CalibrationFunction, metric, theta, run, vals, False)

    def run_phi(want_sums, want_taps=False):
        return _video_pass(metric, vs, fixation_point, vals, want_sums, pvals, want_taps)

    if not phi_grad:
        run = lambda want_sums: run_phi(want_sums)[:4]                                     # noqa: E731
        return _apply(_CalibrationFunction, metric, theta, run, vals, False)
    fps = float(vs.get_frames_per_second())
    return _TemporalCalibrationFunction.apply(theta, temporal, metric, vals, run_phi,
                                              (fps, filter_length(fps), pvals[0], pvals[1]))
