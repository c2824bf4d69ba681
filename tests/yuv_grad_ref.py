"""Float64 (and, via dtype=, float32) restatement of the adjoint of the raw-YUV unpack, in plain numpy: the yardstick of
fvvdp_yuv_grad_planes (include/fvvdp_hip_yuv_grad.h).  TEST INFRASTRUCTURE: numpy only, no GPU.  Its forward is
yuv_channels_ref.yuv_rgb (which takes fractional codes as they are); tests/test_yuv_grad_cpu.py pins the chroma transpose by
<A x, y> = <x, A^T y> and the whole adjoint against torch autograd of the product's unpack arithmetic.

Per frame, with gL the gradient of the frame's luminance:
    d_c = gL w_c EOTF'(rgb_c) (0 where rgb_c is clipped);  dYf = sum_c M[c,0] d_c, du = sum_c M[c,1] d_c, dv = sum_c M[c,2] d_c
    dY = wy dYf, dU = wc Up^T(du), dV = wc Up^T(dv), each 0 where its clamp binds (torch.clamp's backward: open on the closed range)
"""
import numpy as np

import yuv_channels_ref as yref

F64 = np.float64
EOTF_SRGB, EOTF_GAMMA, EOTF_PQ, EOTF_LINEAR, EOTF_ABSOLUTE = 1, 2, 3, 4, 5         # FVVDP_EOTF_*
PQ_N, PQ_M = 0.15930175781250000, 78.843750000000000
PQ_C1, PQ_C2, PQ_C3 = 0.83593750000000000, 18.851562500000000, 18.687500000000000


def axis(n_out, n_in, F):
    """Lower source index, upper source index and weight of the upper one for every destination sample (upsample_x2's rule)."""
    src = np.maximum((np.arange(n_out, dtype=F) + F(0.5)) * F(0.5) - F(0.5), F(0))
    i0 = src.astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (src - i0.astype(F)).astype(F)


def upsample_t(g, uvh, uvw, dtype=F64):
    """The transpose of yuv_channels_ref.upsample_x2: g [P, H, W] -> [P, uvh, uvw]."""
    F = dtype
    g = np.asarray(g, dtype=F)
    P, H, W = g.shape
    y0, y1, fy = axis(H, uvh, F)
    x0, x1, fx = axis(W, uvw, F)
    rows = np.zeros((P, uvh, W), dtype=F)
    np.add.at(rows, (slice(None), y0), (F(1) - fy)[None, :, None] * g)
    np.add.at(rows, (slice(None), y1), fy[None, :, None] * g)
    out = np.zeros((P, uvh, uvw), dtype=F)
    np.add.at(out, (slice(None), slice(None), x0), (F(1) - fx)[None, None, :] * rows)
    np.add.at(out, (slice(None), slice(None), x1), fx[None, None, :] * rows)
    return out


def pre_clip_rgb(Y, U, V, bit_depth, chroma_ss, M, dtype=F64):
    """(rgb [H, W, 3] before its clip to [0, 1], luma clamp open [H, W], chroma clamp open [2, uvh, uvw]) of one frame of sample
    planes; the arithmetic of yuv_channels_ref.yuv_rgb."""
    F = dtype
    H, W = Y.shape
    sc = 2 ** (bit_depth - 8)
    yl = F(1 / (sc * 219)) * np.asarray(Y).astype(F) - F(16 / 219)
    cl = F(1 / (sc * 224)) * np.stack((np.asarray(U), np.asarray(V))).astype(F) - F(128 / 224)
    Yf = np.clip(yl, 0, 1).astype(F)
    uv = np.clip(cl, F(-0.5), F(0.5)).astype(F)
    if chroma_ss == "420":
        uv = yref.upsample_x2(uv, H, W, F)
    Yuv = np.stack((Yf, uv[0], uv[1]), axis=-1)
    rgb = (Yuv @ np.asarray(M, dtype=F).T).astype(F)
    return rgb, (yl >= 0) & (yl <= 1), (cl >= F(-0.5)) & (cl <= F(0.5))


def eotf_grad(V, kind, dtype=F64, Y_peak=0.0, Y_black=0.0, gamma=2.2, L_min=0.0, L_max=0.0):
    """dL/dV of the display model at the clipped-to-[0, 1] sample V, in `dtype`; zero outside the closed ranges of the model's own
    clamps (video_grad_input_ref.eotf_grad for any dtype and without its float32 view of the sample)."""
    F = dtype
    V = np.asarray(V, dtype=F)
    scale = F(F(Y_peak) - F(Y_black))
    with np.errstate(all="ignore"):
        if kind == EOTF_SRGB:
            hi = F(2.4 / 1.055) * np.power((V + F(0.055)) / F(1.055), F(1.4))
            return (scale * np.where(V > F(0.04045), hi, F(1 / 12.92))).astype(F)
        if kind == EOTF_GAMMA:
            return np.where(V > 0, scale * F(gamma) * np.power(V, F(gamma) - F(1)), F(0)).astype(F)
        if kind == EOTF_PQ:
            t = np.power(V, F(1 / PQ_M))
            den = F(PQ_C2) - F(PQ_C3) * t
            r = np.maximum(t - F(PQ_C1), F(0)) / den
            L = F(10000) * np.power(r, F(1 / PQ_N))
            d = L / (F(PQ_N) * r) * (F(PQ_C2 - PQ_C3 * PQ_C1) / (den * den)) * (t / (F(PQ_M) * V))
            return np.where((V > 0) & (r > 0) & (L >= F(0.005)) & (L <= F(Y_peak)), d, F(0)).astype(F)
        if kind == EOTF_LINEAR:
            return np.where((V >= F(0.005)) & (V <= F(Y_peak)), F(1), F(0)).astype(F)
        if kind == EOTF_ABSOLUTE:
            return np.where((V >= F(L_min)) & (V <= F(L_max)), F(1), F(0)).astype(F)
    raise ValueError("no closed form for display model kind %r" % (kind,))


def unpack_adjoint(gL, Y, U, V, bit_depth, chroma_ss, M, rgb2y, kind, dtype=F64, absolute=False, **eotf):
    """(dY [H, W], dU, dV [uvh, uvw]) of one frame in `dtype`.  absolute: the same sums over the absolute values of their terms,
    clamps applied -- the scale of the rounding error of any evaluation order."""
    F = dtype
    rgb, y_open, c_open = pre_clip_rgb(Y, U, V, bit_depth, chroma_ss, M, F)
    inside = (rgb >= 0) & (rgb <= 1)
    w = np.asarray(rgb2y, dtype=np.float32).astype(F)
    d = np.where(inside, np.asarray(gL, dtype=F)[..., None] * w * eotf_grad(np.clip(rgb, 0, 1), kind, F, **eotf), F(0)).astype(F)
    Mf = np.asarray(M, dtype=F)
    if absolute:
        d, Mf = np.abs(d), np.abs(Mf)
    dYuv = (d @ Mf).astype(F)                                   # [H, W, 3]: sum_c M[c, k] d_c
    sc = 2 ** (bit_depth - 8)
    dY = np.where(y_open, F(1 / (sc * 219)) * dYuv[..., 0], F(0)).astype(F)
    duv = np.ascontiguousarray(dYuv[..., 1:].transpose(2, 0, 1))
    if chroma_ss == "420":
        duv = upsample_t(duv, U.shape[0], U.shape[1], F)
    dC = np.where(c_open, F(1 / (sc * 224)) * duv, F(0)).astype(F)
    return dY, dC[0], dC[1]


def rgb_margin(Y, U, V, bit_depth, chroma_ss, M):
    """Per luma pixel, the smallest distance of a float64 pre-clip RGB value from 0, from 1 and from the sRGB toe (0.04045)."""
    rgb, _, _ = pre_clip_rgb(Y, U, V, bit_depth, chroma_ss, M, F64)
    return np.minimum(np.minimum(np.abs(rgb), np.abs(rgb - 1.0)), np.abs(rgb - 0.04045)).min(axis=-1)


def eotf_args(photometry):
    """(kind, keyword arguments of eotf_grad) of an oracle photometry object (yuv_channels_ref.photometry_for)."""
    if isinstance(photometry, yref.AbsolutePhotometry):
        return EOTF_ABSOLUTE, dict(L_min=photometry.L_min, L_max=photometry.L_max)
    kind = {"sRGB": EOTF_SRGB, "gamma": EOTF_GAMMA, "PQ": EOTF_PQ, "linear": EOTF_LINEAR}[photometry.EOTF]
    return kind, dict(Y_peak=np.float32(photometry.Y_peak), Y_black=np.float32(photometry.get_black_level()),
                      gamma=np.float32(photometry.gamma))
