"""Float64 (and, via dtype=, float32) restatement of the resizing ingest and of the resize's adjoint, in plain numpy: the yardstick
of fvvdp_temporal_channels_resized and fvvdp_resize_grad (include/fvvdp_hip_resize.h).  TEST INFRASTRUCTURE: numpy only, no GPU.

Forward, per stream:  resize -> clip to [0, 1] -> display model -> luminance weights -> temporal channels.
Adjoint, per frame:   d_c = gL w_c EOTF'(v_c) where the pre-clip value v_c lies in [0, 1], else 0;  grad_c = Ay^T d_c Ax.

The resize is written as two dense matrices, one per axis (every mode of torch's interpolate without antialiasing is separable).
Tap INDICES, window bounds and interpolation WEIGHTS come from float32 arithmetic exactly as ATen does it (UpSample.h:
area_pixel_compute_scale / _source_index, nearest_neighbor_compute_source_index, guard_index_and_lambda, the cubic coefficients
with A = -0.75; AdaptiveAveragePooling.cpp: start_index / end_index) -- in float64 `nearest` and `area` would pick other pixels
than the kernel at some size pairs.  Only the sums run in `dtype`.  tests/test_resize_cpu.py pins the matrices against
torch.nn.functional.interpolate and the adjoint against torch autograd."""
import copy

import numpy as np

import yuv_channels_ref as yref
from yuv_grad_ref import eotf_args, eotf_grad          # noqa: F401  (eotf_args: for the callers)

orc = yref.orc
F32, F64 = np.float32, np.float64
MODES = ("nearest", "bilinear", "bicubic", "area")


def _cubic(t):
    A = F32(-0.75)
    cc1 = lambda x: ((A + F32(2)) * x - (A + F32(3))) * x * x + F32(1)
    cc2 = lambda x: ((A * x - F32(5) * A) * x + F32(8) * A) * x - F32(4) * A
    return [cc2(t + F32(1)), cc1(t), cc1(F32(1) - t), cc2(F32(2) - t)]


def axis_taps(n_in, n_out, mode):
    """[(source indices [n_out] int64, weights [n_out] float32)] of one axis: one entry per tap, indices and weights computed in
    float32 as ATen computes them.  Equal sizes: the identity, whatever the mode (such a stream is not resampled)."""
    o = np.arange(n_out, dtype=F32)
    if n_in == n_out:
        return [(np.arange(n_out, dtype=np.int64), np.ones(n_out, F32))]
    scale = F32(n_in) / F32(n_out)
    if mode == "nearest":
        return [(np.minimum(np.floor(o * scale).astype(np.int64), n_in - 1), np.ones(n_out, F32))]
    if mode == "bilinear":
        src = np.maximum(scale * (o + F32(0.5)) - F32(0.5), F32(0)).astype(F32)
        i0 = np.minimum(src.astype(np.int64), n_in - 1)
        i1 = i0 + (i0 < n_in - 1)
        l1 = np.clip(src - i0.astype(F32), F32(0), F32(1)).astype(F32)
        return [(i0, (F32(1) - l1).astype(F32)), (i1, l1)]
    if mode == "bicubic":
        src = (scale * (o + F32(0.5)) - F32(0.5)).astype(F32)
        fl = np.floor(src)
        c = _cubic((src - fl).astype(F32))
        return [(np.clip(fl.astype(np.int64) - 1 + k, 0, n_in - 1), c[k].astype(F32)) for k in range(4)]
    if mode == "area":
        oi = np.arange(n_out, dtype=np.int64)
        a0 = np.floor((oi * n_in).astype(F32) / F32(n_out)).astype(np.int64)
        a1 = np.ceil(((oi + 1) * n_in).astype(F32) / F32(n_out)).astype(np.int64)
        taps = []
        for k in range(int((a1 - a0).max())):
            inside = a0 + k < a1
            taps.append((np.where(inside, a0 + k, a0), np.where(inside, F32(1) / (a1 - a0).astype(F32), F32(0)).astype(F32)))
        return taps
    raise RuntimeError("Unknown resize method '%s'" % mode)


def axis_matrix(n_in, n_out, mode, dtype=F64, absolute=False):
    """A [n_out, n_in] in `dtype`: A[o, i] = the sum of the weights of target o's taps that read source i (taps the index clamp
    folds onto one border sample add up).  absolute: the sum of their absolute values."""
    A = np.zeros((n_out, n_in), dtype=dtype)
    rows = np.arange(n_out)
    for idx, w in axis_taps(n_in, n_out, mode):
        np.add.at(A, (rows, idx), np.abs(w).astype(dtype) if absolute else w.astype(dtype))
    return A


def axis_support(n_in, n_out, mode):
    """Boolean [n_out, n_in]: which source samples a target reads at all (a tap with weight 0 still reads)."""
    S = np.zeros((n_out, n_in), dtype=bool)
    for idx, _ in axis_taps(n_in, n_out, mode):
        S[np.arange(n_out), idx] = True
    return S


def unit(x, dtype=F64):
    """Samples as values: float32 as they are, uint8 codes / 255."""
    x = np.asarray(x)
    return x.astype(dtype) / dtype(255) if x.dtype == np.uint8 else x.astype(dtype)


def resize(x, size, mode, dtype=F64, absolute=False):
    """x [..., h, w] (values) -> [..., Ho, Wo] before the clip; size = (Wo, Ho)."""
    Wo, Ho = size
    h, w = x.shape[-2:]
    Ay, Ax = axis_matrix(h, Ho, mode, dtype, absolute), axis_matrix(w, Wo, mode, dtype, absolute)
    return np.matmul(np.matmul(Ay, np.asarray(x, dtype=dtype)), Ax.T).astype(dtype)


def luminance(frame, size, mode, photometry, rgb2y, dtype=F64):
    """One frame [C, h, w] of samples -> the luminance frame [Ho, Wo] the ingest pushes into its ring."""
    F = dtype
    v = np.clip(resize(unit(frame, F), size, mode, F), F(0), F(1)).astype(F)
    L, oob = photometry.forward(v[None, :, None])                          # [1, C, 1, Ho, Wo], as frame_luminance
    assert not oob
    if v.shape[0] == 3:
        L = L[:, 0:1] * F(rgb2y[0]) + L[:, 1:2] * F(rgb2y[1]) + L[:, 2:3] * F(rgb2y[2])
    return L[0, 0, 0].astype(F)


def resized_temporal_channels(test, ref, size, mode, photometry, rgb2y, taps32, idx, dtype=F64):
    """yuv_channels_ref.yuv_temporal_channels for clips [C, N, h, w] with sizes of their own: (R, S), R [N, 4, Ho, Wo] in the plane
    order of level 0 and the per-pixel error scale S = sum_k |tap_k| L[window slot k]."""
    F = dtype
    ph = copy.copy(photometry)
    ph.dtype = F
    taps = np.asarray(taps32, dtype=np.float32).astype(F)
    N, fl = idx.shape
    lum = [{}, {}]

    def L(s, f):
        if f not in lum[s]:
            lum[s][f] = luminance((test, ref)[s][:, f], size, mode, ph, rgb2y, F)
        return lum[s][f]
    Wo, Ho = size
    R = np.zeros((N, 4, Ho, Wo), dtype=F)
    S = np.zeros((N, 4, Ho, Wo), dtype=F)
    a = np.abs(taps)
    for ff in range(N):
        win = [np.stack([L(s, int(j)) for j in idx[ff]], 0) for s in range(2)]
        R[ff] = orc.temporal_channels(win[0], win[1], taps, F)
        S[ff] = orc.temporal_channels(win[0], win[1], a, F)
    return R, S


def clip_adjoint(G, frame, size, mode, dtype=F64, absolute=False):
    """The adjoint of resize-then-clip alone: G [C, Ho, Wo], the gradient of every clipped target value, -> [C, h, w].  The clip is
    open on the closed range [0, 1], as torch.clamp's backward.  absolute: the same sums over the absolute values of their terms."""
    F = dtype
    x = np.asarray(frame, dtype=F)
    h, w = x.shape[-2:]
    Wo, Ho = size
    v = resize(x, size, mode, F)
    d = np.where((v >= 0) & (v <= 1), np.asarray(G, dtype=F), F(0)).astype(F)
    if absolute:
        d = np.abs(d)
    Ay, Ax = axis_matrix(h, Ho, mode, F, absolute), axis_matrix(w, Wo, mode, F, absolute)
    return np.matmul(np.matmul(Ay.T, d), Ax).astype(F)


def resize_adjoint(gL, frame, size, mode, rgb2y, kind, dtype=F64, absolute=False, **eotf):
    """The gradient [C, h, w] of one float frame [C, h, w] for the luminance gradient gL [Ho, Wo].  absolute: the same sums over the
    absolute values of their terms, clip applied -- the scale of the rounding error of any evaluation order."""
    F = dtype
    x = np.asarray(frame, dtype=F)
    v = resize(x, size, mode, F)
    wgt = np.asarray(rgb2y, dtype=np.float32).astype(F) if x.shape[0] == 3 else np.ones(1, dtype=F)
    G = np.asarray(gL, dtype=F)[None] * wgt[:, None, None] * eotf_grad(np.clip(v, 0, 1), kind, F, **eotf)
    return clip_adjoint(G, x, size, mode, F, absolute)


def margin(x, size, mode):
    """Per target sample [..., Ho, Wo]: is the float64 pre-clip value in the zone where float32 and float64 could clip differently --
    within 1e-4 of 0 or of 1 without being beyond it by more than 1e-2."""
    v = resize(unit(x), size, mode)
    return ((v >= -1e-2) & (v <= 1e-4)) | ((v >= 1 - 1e-4) & (v <= 1 + 1e-2))
