"""Gradients of the JOD with respect to the model parameters: fvvdp.calibration_jod_images / calibration_jod_video, the
parameter vector behind them and their autograd function (include/fvvdp_hip_params.h).

The twelve parameters of PARAMETER_NAMES enter the metric after the pyramid: six pointwise in the masking model of every band
pixel, six in do_pooling_and_jods.  A call evaluates the metric under a vector `theta` on the metric's ordinary native context,
whose model constants are replaced for the duration of the call (fvvdp_ctx_set_params) and restored in a `finally`: the metric's
attributes are never touched, no context is created.  The forward makes the launches of predict_images / predict with constants
converted from theta exactly as native_params() and _pool_params() convert the attributes, so the JOD is bit-identical to that
of a metric whose attributes hold theta.  When theta needs a gradient the forward also re-runs the pyramid pass with every
band's maps written, per backward batch of frames (image_grad.grad_batch_size), and fvvdp_param_sums reduces the maps to five
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
float64 and are all that is kept.  backward() is `tap_chain`: the float64 Jacobian of the taps with respect to phi."""
import ctypes as C
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .fvvdp import fvvdp as _fvvdp
from .image_grad import grad_batch_size

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
    t = theta.detach() if isinstance(theta, torch.Tensor) else torch.as_tensor(np.asarray(theta, dtype=np.float64))
    if t.dim() != 1 or t.shape[0] != len(PARAMETER_NAMES):
        raise RuntimeError("theta must be a 1-D vector of the %d parameters of PARAMETER_NAMES, got shape %s"
                           % (len(PARAMETER_NAMES), tuple(t.shape)))
    if not t.is_floating_point():
        raise RuntimeError("theta must be a float32 or float64 tensor, got %s" % t.dtype)
    vals = [float(v) for v in t.to(device="cpu", dtype=torch.float64).tolist()]
    bad = [PARAMETER_NAMES[i] for i, v in enumerate(vals) if not math.isfinite(v)]
    if bad:
        raise RuntimeError("theta has non-finite entries: %s" % ", ".join(bad))
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
    t = phi.detach() if isinstance(phi, torch.Tensor) else torch.as_tensor(np.asarray(phi, dtype=np.float64))
    if t.dim() != 1 or t.shape[0] != len(TEMPORAL_PARAMETER_NAMES):
        raise RuntimeError("temporal must be a 1-D vector of the %d parameters of TEMPORAL_PARAMETER_NAMES, got shape %s"
                           % (len(TEMPORAL_PARAMETER_NAMES), tuple(t.shape)))
    if not t.is_floating_point():
        raise RuntimeError("temporal must be a float32 or float64 tensor, got %s" % t.dtype)
    vals = [float(v) for v in t.to(device="cpu", dtype=torch.float64).tolist()]
    bad = [TEMPORAL_PARAMETER_NAMES[i] for i, v in enumerate(vals) if not math.isfinite(v)]
    if bad:
        raise RuntimeError("temporal has non-finite entries: %s" % ", ".join(bad))
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
        self.maps_arr, self._maps = metric._band_maps(gb, W, H, n_bands, contrast_planes=planes)
        nbytes = C.c_size_t(0)
        nat.check(nat.lib().fvvdp_param_sums_workspace(W, H, n_bands, gb, C.byref(nbytes)))
        self.work_bytes = nbytes.value
        self.work = torch.empty((nbytes.value + 7) // 8, dtype=torch.float64, device=dev)
        self.batch_sums = torch.empty((n_bands, 2, gb, nat.PARAM_SUMS), dtype=torch.float64, device=dev)
        self.sums = torch.empty((n_bands, 2, total, nat.PARAM_SUMS), dtype=torch.float64, device=dev)
        self.q_scratch = torch.empty((n_bands, 2, gb), dtype=torch.float32, device=dev)
        self.jod_scratch = torch.empty(gb, dtype=torch.float32, device=dev)
        self.npx = torch.tensor([float(w * h) for w, h in metric._level_sizes(W, H, n_bands)[:n_bands]], dtype=torch.float64)

    def reduce(self, prm, b0, nb, stream):
        """The maps of the nb slots just written -> columns [b0, b0 + nb) of self.sums."""
        out = self.batch_sums.view(-1)[:self.n_bands * 2 * nb * nat.PARAM_SUMS].view(self.n_bands, 2, nb, nat.PARAM_SUMS)
        nat.check(nat.lib().fvvdp_param_sums(self.W, self.H, self.n_bands, nb, self.planes, C.byref(prm), self.maps_arr,
                                             C.c_void_p(out.data_ptr()), C.c_void_p(self.work.data_ptr()), self.work_bytes, stream))
        self.sums[:, :, b0:b0 + nb] = out


def _images_forward(metric, t, r, fix, vals, want_sums):
    """The launches of fvvdp._predict_image_group (no heat maps, no flags read back) under theta -> (JOD [B], Q [bands, 2, B],
    _Sums or None).  t, r: [B, C, H, W] on any device."""
    B, C_ch, height, width = t.shape
    dev = metric.device
    n_bands, rho_band = metric._band_count(width, height)
    if t.dtype != r.dtype:
        t, r = metric._to_unit_float(t), metric._to_unit_float(r)
    td, rd = t.to(dev).contiguous(), r.to(dev).contiguous()
    dtype, e = metric._image_eotf(td.dtype)
    w = metric._rgb2y()
    batch = metric._batch_size(width, height, 2, B)
    ctx = metric._context(width, height, n_bands, 2, batch, rho_band)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    Q = torch.zeros((n_bands, 2, B), dtype=torch.float32, device=dev)
    jod = torch.empty(B, dtype=torch.float32, device=dev)
    prm, pp = native_params_of(vals), pool_params_of(vals)
    lib = nat.lib()
    sums = None

    def ingest(b0, nb):
        tp = (C.c_void_p * nb)(*[td[k].data_ptr() for k in range(b0, b0 + nb)])
        rp = (C.c_void_p * nb)(*[rd[k].data_ptr() for k in range(b0, b0 + nb)])
        nat.check(lib.fvvdp_images_channels(ctx.handle, tp, rp, nb, dtype, C_ch, height * width, C.byref(e), nat.fptr(w), 0,
                                            None, stream))

    with _UnderTheta(metric, ctx, prm):
        for b0 in range(0, B, batch):
            nb = min(batch, B - b0)
            ingest(b0, nb)
            fx, g, _keep = metric._fov_args(ctx, fix, b0, nb, n_bands, width, height)
            nat.check(lib.fvvdp_images_forward_pool(ctx.handle, nb, C.c_void_p(Q.data_ptr()), B, b0, fx, g, None, C.byref(pp),
                                                    C.c_void_p(jod.data_ptr() + 4 * b0), stream))
        if want_sums:
            gb = grad_batch_size(metric, width, height, n_bands, batch, 7)
            sums = _Sums(metric, width, height, n_bands, 2, gb, B)
            for b0 in range(0, B, gb):
                nb = min(gb, B - b0)
                ingest(b0, nb)
                fx, g, _keep = metric._fov_args(ctx, fix, b0, nb, n_bands, width, height)
                nat.check(lib.fvvdp_images_forward_pool(ctx.handle, nb, C.c_void_p(sums.q_scratch.data_ptr()), nb, 0, fx, g,
                                                        sums.maps_arr, C.byref(pp), C.c_void_p(sums.jod_scratch.data_ptr()), stream))
                sums.reduce(prm, b0, nb, stream)
            sums._maps = sums.maps_arr = None            # the maps are transient: only Q and the sums outlive the forward
    return jod, Q, sums


class _TapGrad:
    """Buffers of the tap gradient for a clip of N frames in backward batches of up to gb: the clip-long level-0 gradients of
    both sides, the workspaces of the two level-0 backward passes, the slope planes, the luminance frames under a batch's
    windows, workspace and result of fvvdp_tap_grad, and the running dJOD/dtaps [2, fl] (float64, added in frame order).
    Checked against the free device memory first: a sentence instead of an out-of-memory error."""

    def __init__(self, metric, W, H, n_bands, gb, N, fl, with_scale=False):
        from .image_grad import slope_planes
        dev, HW = metric.device, H * W
        lib = nat.lib()
        vb, rb, tb = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        nat.check(lib.fvvdp_video_grad_workspace(W, H, n_bands, gb, C.byref(vb)))
        nat.check(lib.fvvdp_ref_grad_workspace(W, H, n_bands, gb, 2, C.byref(rb)))
        nat.check(lib.fvvdp_tap_grad_workspace(W, H, fl, C.byref(tb)))
        n_lum = min(N, fl - 1 + gb)
        px = sum(w * h for w, h in metric._level_sizes(W, H, n_bands)[:n_bands])
        lum_bytes = 2 * n_lum * HW * 4
        need = gb * px * 4 * (9 + 2) + vb.value + rb.value + tb.value + 2 * N * HW * 8 + lum_bytes
        free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        if need > free:
            raise RuntimeError("calibration_jod_video: the gradient for the temporal parameters of this clip needs %.1f GB of "
                               "device memory (maps and workspace of %d frames, the clip-long level-0 gradients of both sides "
                               "and %.2f GB of luminance frames under a batch's windows) and %.1f GB are free; set a smaller "
                               "metric.grad_batch or a shorter clip" % (need / 1e9, gb, lum_bytes / 1e9, free / 1e9))
        self.W, self.H, self.n_bands, self.N, self.fl, self.n_lum = W, H, n_bands, N, fl, n_lum
        self.g0 = torch.empty((N, 2, H, W), dtype=torch.float32, device=dev)
        self.g0_r = torch.empty((N, 2, H, W), dtype=torch.float32, device=dev)
        self.work = torch.empty((vb.value + 3) // 4, dtype=torch.float32, device=dev)
        self.work_r = torch.empty((rb.value + 3) // 4, dtype=torch.float32, device=dev)
        self.work_bytes, self.ref_bytes, self.tap_bytes = vb.value, rb.value, tb.value
        self.slopes, self._slopes = slope_planes(metric, gb, W, H, n_bands)
        self.lum = torch.empty((2, n_lum, H, W), dtype=torch.float32, device=dev)
        self.tap_work = torch.empty((tb.value + 7) // 8, dtype=torch.float64, device=dev)
        self.out = torch.empty((2, fl), dtype=torch.float64, device=dev)
        self.dtaps = torch.zeros((2, fl), dtype=torch.float64, device=dev)
        self.gamma = torch.ones(1, dtype=torch.float32, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.scale = torch.zeros((2, fl), dtype=torch.float64, device=dev) if with_scale else None

    def batch(self, feeder, prm, pp, Q, maps_arr, idx, b0, nb, stream):
        """The maps of output frames [b0, b0 + nb) (slope planes included) -> their share of dJOD/dtaps, added to self.dtaps.
        idx: the batch's slice of the window index list (fl - 1 + nb source frames, oldest first)."""
        lib = nat.lib()
        W, H, HW = self.W, self.H, self.H * self.W
        nat.check(lib.fvvdp_video_grad_frames(W, H, self.n_bands, nb, C.byref(prm), C.byref(pp), C.c_void_p(Q.data_ptr()), self.N, b0,
                                              C.c_void_p(self.gamma.data_ptr()), maps_arr, C.c_void_p(self.g0.data_ptr()),
                                              C.c_void_p(self.work.data_ptr()), self.work_bytes, stream))
        nat.check(lib.fvvdp_video_ref_grad_frames(W, H, self.n_bands, nb, C.byref(prm), C.byref(pp), C.c_void_p(Q.data_ptr()), self.N,
                                                  b0, C.c_void_p(self.gamma.data_ptr()), maps_arr, self.slopes,
                                                  C.c_void_p(self.g0_r.data_ptr()), C.c_void_p(self.work_r.data_ptr()),
                                                  self.ref_bytes, stream))
        frames = np.unique(idx)
        nu = len(frames)
        pos = np.ascontiguousarray(np.searchsorted(frames, idx), dtype=np.int32)
        lum = self.lum.view(-1)[:2 * nu * HW]
        feeder.luminance(frames, lum, self.flag, stream)
        nat.check(lib.fvvdp_tap_grad(W, H, nb, self.fl, C.c_void_p(self.g0.data_ptr() + b0 * 2 * HW * 4),
                                     C.c_void_p(self.g0_r.data_ptr() + b0 * 2 * HW * 4), C.c_void_p(lum.data_ptr()),
                                     C.c_void_p(lum.data_ptr() + nu * HW * 4), pos.ctypes.data_as(C.POINTER(C.c_int32)), nu,
                                     C.c_void_p(self.out.data_ptr()), C.c_void_p(self.tap_work.data_ptr()), self.tap_bytes, stream))
        self.dtaps += self.out
        if self.scale is not None:
            # the yardstick of the kernel's rounding: sum |g0 Y| per entry, with torch, in float64
            widx = torch.as_tensor(pos.astype(np.int64), device=self.out.device)
            t = torch.arange(nb, device=self.out.device)
            for k in range(self.fl):
                q = widx[t + self.fl - 1 - k]
                for g, y in ((self.g0, self.lum.view(-1)[:nu * HW].view(nu, H, W)),
                             (self.g0_r, self.lum.view(-1)[nu * HW:2 * nu * HW].view(nu, H, W))):
                    self.scale[:, k] += (g[b0:b0 + nb].abs().double() * y[q].double()[:, None].abs()).sum(dim=(0, 2, 3))


def _video_pass(metric, vs, fixation_point, vals, want_sums, pvals=None, want_taps=False, with_scale=False):
    """The launches of fvvdp._predict_on_device (sync=False, no heat maps) under theta -> (JOD 0-d, Q [bands, 2, N], _Sums or
    None, number of temporal channels, dJOD/dtaps [2, fl] float64 or None).  pvals: the values of TEMPORAL_PARAMETER_NAMES the
    taps are made from (None: the metric's own taps); want_taps: also the gradient of the JOD with respect to the taps."""
    from .fvvdp import _PipelinedSourceFeeder, temporal_filters
    from .video_grad import video_grad_planes
    height, width, N = vs.get_video_size()
    dev = metric.device
    fix = metric._fixation(fixation_point, width, height, N) if metric.foveated else None
    pl = metric._clip_plan(vs)
    if isinstance(pl.feeder, _PipelinedSourceFeeder):
        raise RuntimeError("calibration_jod_video needs a display model with a closed form for float input (sRGB, gamma, PQ, "
                           "linear or absolute); a user photometry class has none")
    n_bands, planes, fl, taps, widx = pl.n_bands, pl.planes, pl.fl, pl.taps, pl.widx
    if pvals is not None:
        if planes != 4:
            raise RuntimeError("calibration_jod_video: temporal= needs a clip of at least 2 frames (a single frame has no "
                               "temporal filter)")
        # the taps under phi: never cached (an optimiser makes a new phi per step), never written to the metric
        taps = np.ascontiguousarray(temporal_filters(vs.get_frames_per_second(), fl, pvals[0], pvals[1]).numpy(), dtype=np.float32)
    ctx = metric._context(width, height, n_bands, planes, pl.batch, pl.rho_band)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    nq = n_bands * 2 * N
    res = torch.zeros(nq + 2, dtype=torch.float32, device=dev)          # Q_per_ch | range flag | JOD, as predict lays it out
    Q = res[:nq].view(n_bands, 2, N)
    oob = res[nq:nq + 1].view(torch.int32)
    prm, pp = native_params_of(vals), pool_params_of(vals)
    lib = nat.lib()
    sums = None
    with _UnderTheta(metric, ctx, prm):
        b0 = 0
        for nb in pl.schedule:
            idx = np.ascontiguousarray(widx[b0:b0 + fl - 1 + nb])
            pl.feeder(ctx, idx, taps, fl, nb, oob, stream)
            fx, g, _keep = metric._fov_args(ctx, fix, b0, nb, n_bands, width, height)
            if b0 + nb == N:
                nat.check(lib.fvvdp_bands_forward_pool(ctx.handle, nb, C.c_void_p(Q.data_ptr()), N, b0, fx, g, None, C.byref(pp),
                                                       C.c_void_p(res[nq + 1:].data_ptr()), stream))
            else:
                nat.check(lib.fvvdp_bands_forward(ctx.handle, nb, C.c_void_p(Q.data_ptr()), N, b0, fx, g, None, stream))
            b0 += nb
        if want_taps:
            # one ingest and one map-writing pass per backward batch (slope planes on, as jod_video(wrt="both")): theta's sums
            # and the two level-0 backward passes read the same maps
            gb = grad_batch_size(metric, width, height, n_bands, pl.batch, video_grad_planes("both"))
            gb = max(1, min(gb, nat.TAPS_MAX_POSITIONS - (fl - 1)))
            tg = _TapGrad(metric, width, height, n_bands, gb, N, fl, with_scale)
            sums = _Sums(metric, width, height, n_bands, planes, gb, N)
            for b0 in range(0, N, gb):
                nb = min(gb, N - b0)
                idx = np.ascontiguousarray(widx[b0:b0 + fl - 1 + nb])
                pl.feeder(ctx, idx, taps, fl, nb, tg.flag, stream)
                fx, g, _keep = metric._fov_args(ctx, fix, b0, nb, n_bands, width, height)
                nat.check(lib.fvvdp_ctx_set_slope_maps(ctx.handle, tg.slopes))
                try:
                    nat.check(lib.fvvdp_bands_forward(ctx.handle, nb, C.c_void_p(sums.q_scratch.data_ptr()), nb, 0, fx, g,
                                                      sums.maps_arr, stream))
                finally:
                    nat.check(lib.fvvdp_ctx_set_slope_maps(ctx.handle, None))
                if want_sums:
                    sums.reduce(prm, b0, nb, stream)
                tg.batch(pl.feeder, prm, pp, Q, sums.maps_arr, idx, b0, nb, stream)
            sums._maps = sums.maps_arr = None
            if not want_sums:
                sums = None
            return res[nq + 1], Q, sums, planes // 2, (tg.dtaps, tg.scale) if with_scale else tg.dtaps
        if want_sums:
            gb = grad_batch_size(metric, width, height, n_bands, pl.batch, 9 if planes == 4 else 7)
            sums = _Sums(metric, width, height, n_bands, planes, gb, N)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            for b0 in range(0, N, gb):
                nb = min(gb, N - b0)
                idx = np.ascontiguousarray(widx[b0:b0 + fl - 1 + nb])
                pl.feeder(ctx, idx, taps, fl, nb, flag, stream)
                fx, g, _keep = metric._fov_args(ctx, fix, b0, nb, n_bands, width, height)
                nat.check(lib.fvvdp_bands_forward(ctx.handle, nb, C.c_void_p(sums.q_scratch.data_ptr()), nb, 0, fx, g,
                                                  sums.maps_arr, stream))
                sums.reduce(prm, b0, nb, stream)
            sums._maps = sums.maps_arr = None
    return res[nq + 1], Q, sums, planes // 2, None


def _video_forward(metric, vs, fixation_point, vals, want_sums):
    """_video_pass under the metric's own temporal filters -> (JOD 0-d, Q [bands, 2, N], _Sums or None, temporal channels)."""
    return _video_pass(metric, vs, fixation_point, vals, want_sums)[:4]


def tap_gradient(metric, test, reference, theta, temporal, dim_order="BCFHW", frames_per_second=0, fixation_point=None,
                 with_scale=False):
    """dJOD/dtaps [2, fl] (float64, on the metric's device) of one clip under theta and phi: what the forward of
    calibration_jod_video keeps when phi requires grad.  For tests and tools.  with_scale: also sum |g0 Y| of every entry, the
    yardstick of the tap-gradient kernel's rounding (include/fvvdp_hip_taps.h), made with torch."""
    from .video_source import fvvdp_video_source_array
    vals, pvals = theta_values(theta), phi_values(temporal)
    vs = fvvdp_video_source_array(test, reference, frames_per_second, dim_order=dim_order,
                                  display_photometry=metric.display_photometry, color_space_name=metric.color_space)
    metric._check_device()
    with torch.cuda.device(metric.device):
        return _video_pass(metric, vs, fixation_point, vals, False, pvals, True, with_scale)[4]


class _CalibrationFunction(torch.autograd.Function):
    """theta -> JOD ([B] for images, 0-d for a clip).  `run(want_sums)` makes the forward under theta's values."""

    @staticmethod
    def forward(ctx, theta, metric, vals, run, per_column):
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


def _refuse(name, metric, test, reference, other):
    for a in (test, reference):
        if isinstance(a, torch.Tensor) and a.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("%s differentiates the JOD with respect to the model parameters only and this test or reference "
                               "requires grad; detach it (gradients for the images or frames: %s)" % (name, other))
    if metric.do_heatmap:
        raise RuntimeError("%s makes no heat maps: build the metric with heatmap=None" % name)


def _apply(metric, theta, vals, run, per_column):
    if isinstance(theta, torch.Tensor) and theta.requires_grad and torch.is_grad_enabled():
        return _CalibrationFunction.apply(theta, metric, vals, run, per_column)
    with torch.cuda.device(metric.device):
        return run(False)[0]


def calibration_jod_images(metric, test, reference, theta, dim_order="BCHW", fixation_point=None):
    """fvvdp.calibration_jod_images (see there)."""
    from .fvvdp import _image_stack
    vals = theta_values(theta)
    _refuse("calibration_jod_images", metric, test, reference, "jod_images")
    t, r = _image_stack(test, reference, dim_order)
    metric._check_device()
    fix = metric._fixation(fixation_point, t.shape[3], t.shape[2], t.shape[0]) if metric.foveated else None

    def run(want_sums):
        jod, Q, sums = _images_forward(metric, t, r, fix, vals, want_sums)
        return jod, Q, sums, 1

    return _apply(metric, theta, vals, run, True)


def calibration_jod_video(metric, test, reference, theta, dim_order="BCFHW", frames_per_second=0, fixation_point=None,
                          temporal=None):
    """fvvdp.calibration_jod_video (see there)."""
    from .fvvdp import filter_length
    from .video_source import fvvdp_video_source_array
    vals = theta_values(theta)
    pvals = None if temporal is None else phi_values(temporal)
    phi_grad = isinstance(temporal, torch.Tensor) and temporal.requires_grad and torch.is_grad_enabled()
    if phi_grad and frames_per_second > 0 and filter_length(frames_per_second) > nat.VIDEO_GRAD_MAX_TAPS:
        raise RuntimeError("calibration_jod_video: frame rate too high for the gradient of the temporal parameters: the temporal "
                           "filter has %d taps, the tap-gradient kernel covers %d (256 frames per second); the forward runs "
                           "with a temporal= that does not require grad"
                           % (filter_length(frames_per_second), nat.VIDEO_GRAD_MAX_TAPS))
    _refuse("calibration_jod_video", metric, test, reference, "jod_video")
    d = dim_order.upper()
    if "B" in d and len(d) == len(test.shape) and test.shape[d.index("B")] != 1:
        raise RuntimeError("calibration_jod_video takes one clip per call (B must be 1)")
    vs = fvvdp_video_source_array(test, reference, frames_per_second, dim_order=dim_order,
                                  display_photometry=metric.display_photometry, color_space_name=metric.color_space)
    metric._check_device()

    if temporal is None:
        def run(want_sums):
            return _video_forward(metric, vs, fixation_point, vals, want_sums)

        return _apply(metric, theta, vals, run, False)

    def run_phi(want_sums, want_taps=False):
        return _video_pass(metric, vs, fixation_point, vals, want_sums, pvals, want_taps)

    if not phi_grad:
        return _apply(metric, theta, vals, lambda want_sums: run_phi(want_sums)[:4], False)
    fps = float(vs.get_frames_per_second())
    return _TemporalCalibrationFunction.apply(theta, temporal, metric, vals, run_phi,
                                              (fps, filter_length(fps), pvals[0], pvals[1]))
