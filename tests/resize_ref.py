"""Float64 (and, via dtype=, float32) restatement of the resizing ingest and of the resize's adjoint, in plain numpy: the yardstick
of fvvdp_temporal_channels_resized and fvvdp_resize_grad (include/fvvdp_hip_resize.h).  TEST INFRASTRUCTURE: numpy only, no GPU.

Forward, per stream:  resize -> clip to [0, 1] -> display model -> luminance weights -> temporal channels.
Adjoint, per frame:   d_c = gL w_c EOTF'(v_c) where the pre-clip value v_c lies in [0, 1], else 0;  grad_c = Ay^T d_c Ax.

The resize is written as two matrices, one per axis (every mode of torch's interpolate without antialiasing is separable): dense
ones at the small sizes, the same taps applied one by one where a dense matrix would be large (DENSE_MAX).  Tap INDICES and
interpolation WEIGHTS of `nearest`, `bilinear` and `bicubic` come from float32 arithmetic exactly as ATen does it (UpSample.h:
area_pixel_compute_scale / _source_index, nearest_neighbor_compute_source_index, guard_index_and_lambda, the cubic coefficients
with A = -0.75) -- in float64 `nearest` would pick other pixels than the kernel at some size pairs.  The windows of `area` are
ATen's INTEGERS (AdaptiveAveragePooling.cpp: start_index = (o * in) / out, end_index = 1 + ((o + 1) * in - 1) / out): floor and
ceil of a float32 quotient give the same windows only while o * in stays below 2^24.  Only the sums run in `dtype`.
tests/test_resize_cpu.py pins the matrices against torch.nn.functional.interpolate, up to 32768 samples per axis, and the adjoint
against torch autograd."""
import copy
import functools

import numpy as np

import yuv_channels_ref as yref
from yuv_grad_ref import eotf_args, eotf_grad          # noqa: F401  (eotf_args: for the callers)

orc = yref.orc
F32, F64 = np.float32, np.float64
MODES = ("nearest", "bilinear", "bicubic", "area")
DENSE_MAX = 1 << 20          # entries of a dense axis matrix; beyond, resize and its adjoint apply the taps one by one


def _cubic(t):
    A = F32(-0.75)
    cc1 = lambda x: ((A + F32(2)) * x - (A + F32(3))) * x * x + F32(1)
    cc2 = lambda x: ((A * x - F32(5) * A) * x + F32(8) * A) * x - F32(4) * A
    return [cc2(t + F32(1)), cc1(t), cc1(F32(1) - t), cc2(F32(2) - t)]


@functools.lru_cache(maxsize=64)
def axis_taps(n_in, n_out, mode):
    """[(source indices [n_out] int64, weights [n_out] float32)] of one axis: one entry per tap, indices and weights computed as ATen
    computes them (float32; the windows of `area` in integers).  Equal sizes: the identity, whatever the mode (such a stream is not
    resampled).  The arrays are shared between the callers: read only."""
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
        a0 = (oi * n_in) // n_out
        a1 = 1 + ((oi + 1) * n_in - 1) // n_out
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


def _dense(h, w, size):
    return h * size[1] <= DENSE_MAX and w * size[0] <= DENSE_MAX


def axis_apply(x, axis, n_out, mode, dtype=F64, absolute=False, support=False):
    """axis_matrix(...) applied along `axis` of x without building it: the sum over the taps, in their order.  support: axis_support
    in the matrix's place (every sample a target reads counts once, whatever its weight)."""
    xm = np.moveaxis(np.asarray(x, dtype=dtype), axis, 0)
    out = np.zeros((n_out,) + xm.shape[1:], dtype=dtype)
    seen = []
    for idx, w in axis_taps(xm.shape[0], n_out, mode):
        wt = (np.abs(w) if absolute else w).astype(dtype)
        if support:
            wt = (~np.any([idx == j for j in seen], axis=0) if seen else np.ones(n_out, bool)).astype(dtype)
            seen.append(idx)
        out += wt.reshape((-1,) + (1,) * (xm.ndim - 1)) * xm[idx]
    return np.moveaxis(out, 0, axis)


def axis_apply_T(d, axis, n_in, mode, dtype=F64, absolute=False):
    """The transpose of axis_matrix(...) applied along `axis` of d [.., n_out, ..] -> [.., n_in, ..]."""
    dm = np.moveaxis(np.asarray(d, dtype=dtype), axis, 0)
    out = np.zeros((n_in,) + dm.shape[1:], dtype=dtype)
    for idx, w in axis_taps(n_in, dm.shape[0], mode):
        wt = (np.abs(w) if absolute else w).astype(dtype)
        np.add.at(out, idx, wt.reshape((-1,) + (1,) * (dm.ndim - 1)) * dm)
    return np.moveaxis(out, 0, axis)


def reaches(bad, source, mode):
    """bad: boolean [..., Ho, Wo] -> boolean [..., h, w]: the source samples some marked target sample reads (a tap with weight 0
    still reads); source = (w, h)."""
    w, h = source
    Ho, Wo = bad.shape[-2:]
    if _dense(h, w, (Wo, Ho)):
        Sy, Sx = axis_support(h, Ho, mode).astype(np.float64), axis_support(w, Wo, mode).astype(np.float64)
        return np.matmul(np.matmul(Sy.T, bad.astype(np.float64)), Sx) > 0
    hit = np.asarray(bad, dtype=bool)
    for axis, n_in, n_out in ((-2, h, Ho), (-1, w, Wo)):
        dm = np.moveaxis(hit, axis, 0)
        out = np.zeros((n_in,) + dm.shape[1:], dtype=bool)
        for idx, _ in axis_taps(n_in, n_out, mode):
            np.logical_or.at(out, idx, dm)
        hit = np.moveaxis(out, 0, axis)
    return hit


def resize(x, size, mode, dtype=F64, absolute=False):
    """x [..., h, w] (values) -> [..., Ho, Wo] before the clip; size = (Wo, Ho)."""
    Wo, Ho = size
    h, w = x.shape[-2:]
    if not _dense(h, w, size):
        return axis_apply(axis_apply(x, -2, Ho, mode, dtype, absolute), -1, Wo, mode, dtype, absolute).astype(dtype)
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
    if not _dense(h, w, size):
        return axis_apply_T(axis_apply_T(d, -2, h, mode, F, absolute), -1, w, mode, F, absolute).astype(F)
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
