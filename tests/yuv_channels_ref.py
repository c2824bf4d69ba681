"""Float64 yardstick for the raw-YUV ingest kernels (temporal_yuv_vec_kernel, temporal_yuv_kernel, yuv_luminance_frames_kernel):
planar limited-range YUV codes -> RGB -> display model -> luminance -> temporal channels, written out plainly in numpy from the
reference's unpack (pyfvvdp/video_source_file.py:219-276, as documented in oracle/fvvdp_oracle.py::yuv_unpack) with an arbitrary
3x3 colour matrix.  With dtype=np.float32 the same function reproduces the reference's float32 chain bit for bit, which gives every
test case its own baseline error.  TEST INFRASTRUCTURE: numpy only, no GPU; tests/test_yuv_ref_cpu.py pins it against the oracle and
the product's torch unpack.

Also here, because the CPU tests and the GPU tests must share them: the random clips (`yuv_clip`), the comparison (`channel_error`,
`error_bound`, `assert_channels_close`) and the display models of the test matrix (`photometry_for`).
"""
import copy

import numpy as np

from oracle import fvvdp_oracle as orc

F64 = np.float64


# ---- the unpack ----------------------------------------------------------------------------------------------------------
def upsample_x2(uv, H, W, F):
    """torch.nn.functional.interpolate(uv, scale_factor=2, mode='bilinear', align_corners=False) for uv [2,uvh,uvw]:
    source coordinate (dst + 0.5) / 2 - 0.5 clamped at 0, upper neighbour clamped to the last row / column."""
    uvh, uvw = uv.shape[1:]

    def axis(n_out, n_in):
        src = np.maximum((np.arange(n_out, dtype=F) + F(0.5)) * F(0.5) - F(0.5), F(0))
        i0 = src.astype(np.int64)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, (src - i0.astype(F)).astype(F)
    y0, y1, fy = axis(H, uvh)
    x0, x1, fx = axis(W, uvw)
    fy, fx = fy[None, :, None], fx[None, None, :]
    top = (F(1) - fx) * uv[:, y0][:, :, x0] + fx * uv[:, y0][:, :, x1]
    bot = (F(1) - fx) * uv[:, y1][:, :, x0] + fx * uv[:, y1][:, :, x1]
    return ((F(1) - fy) * top + fy * bot).astype(F)


def yuv_rgb(frame, W, H, bit_depth, chroma_ss, matrix3x3, dtype=F64, upsample=upsample_x2):
    """One planar frame of codes (1-D: Y plane, U plane, V plane; any integer dtype, the VALUES are the codes) -> display-encoded
    RGB [H,W,3] in [0,1]."""
    F = dtype
    ypx = W * H
    uvh, uvw = (H // 2, W // 2) if chroma_ss == "420" else (H, W)
    x = np.asarray(frame).astype(F)                                                    # code -> float
    sc = 2 ** (bit_depth - 8)
    Y = np.clip(F(1 / (sc * 219)) * x[:ypx] - F(16 / 219), 0, 1).reshape(H, W).astype(F)                      # limited-range luma, clamp
    uv = np.clip(F(1 / (sc * 224)) * x[ypx:] - F(128 / 224), F(-0.5), F(0.5)).reshape(2, uvh, uvw).astype(F)    # chroma, clamp
    if chroma_ss == "420":
        uv = upsample(uv, H, W, F)
    Yuv = np.stack((Y, uv[0], uv[1]), axis=-1)
    M = np.asarray(matrix3x3, dtype=F)        # (the kernels receive nine float32 numbers: their tests pass the rounded matrix)
    return np.clip((Yuv @ M.T).astype(F), 0, 1).astype(F)


def _luminance(frame, W, H, bit_depth, chroma_ss, matrix3x3, photometry, rgb2y, F, upsample):
    rgb = yuv_rgb(frame, W, H, bit_depth, chroma_ss, matrix3x3, F, upsample)
    L, oob = photometry.forward(rgb.transpose(2, 0, 1)[None, :, None])                # [1,3,1,H,W], as frame_luminance
    assert not oob                                                                     # RGB is clipped before the display model
    L = L[:, 0:1] * F(rgb2y[0]) + L[:, 1:2] * F(rgb2y[1]) + L[:, 2:3] * F(rgb2y[2])
    return L[0, 0, 0].astype(F)


def yuv_temporal_channels(test_yuv, ref_yuv, W, H, bit_depth, chroma_ss, matrix3x3, photometry, rgb2y, taps32, idx, dtype=F64,
                          upsample=upsample_x2):
    """Temporal channels of a raw-YUV clip pair.  test_yuv / ref_yuv: [N, frame_elems] codes; photometry: an oracle Photometry (or
    AbsolutePhotometry); taps32: float32 [2, fl] (oracle.temporal_filters); idx: [N, fl] from window_frame_indices.
    Returns (R, S): R [N,4,H,W] in the plane order of level 0 (sustained test, sustained reference, transient test, transient
    reference) and the per-pixel error scale S [N,4,H,W] = sum_k |taps[cc][k]| * L_s[window slot k] (the transient taps sum to
    about 0, so |R| is no usable scale), both in `dtype`."""
    F = dtype
    ph = copy.copy(photometry)
    ph.dtype = F
    taps = np.asarray(taps32, dtype=np.float32).astype(F)
    N, fl = idx.shape
    assert taps.shape == (2, fl)
    lum = [{}, {}]

    def L(s, f):
        if f not in lum[s]:
            lum[s][f] = _luminance((test_yuv, ref_yuv)[s][f], W, H, bit_depth, chroma_ss, matrix3x3, ph, rgb2y, F, upsample)
        return lum[s][f]
    R = np.zeros((N, 4, H, W), dtype=F)
    S = np.zeros((N, 4, H, W), dtype=F)
    a = np.abs(taps)
    for ff in range(N):
        win = [np.stack([L(s, int(j)) for j in idx[ff]], 0) for s in range(2)]        # oldest first
        R[ff] = orc.temporal_channels(win[0], win[1], taps, F)
        S[ff] = orc.temporal_channels(win[0], win[1], a, F)
    return R, S


class AbsolutePhotometry:
    """fvvdp_display_photo_absolute (pyfvvdp/fvvdp_display_model.py:203-212): the content is cd/m^2 already, clamped to the display's range."""

    def __init__(self, L_max=10000, L_min=0.005, dtype=np.float32):
        self.L_max, self.L_min, self.dtype = L_max, L_min, dtype

    def forward(self, V):
        F = self.dtype
        return np.clip(np.asarray(V, dtype=F), F(self.L_min), F(self.L_max)).astype(F), False


# ---- the comparison ------------------------------------------------------------------------------------------------------
def channel_error(R, R64, S64):
    """max |R - R64| / S over every frame, plane and pixel."""
    assert R.shape == R64.shape == S64.shape, (R.shape, R64.shape, S64.shape)
    assert np.all(S64 > 0)
    return float(np.max(np.abs(np.asarray(R, F64) - R64) / S64))


def error_bound(e_ref):
    """4 x the error of the reference's own float32 chain on the same inputs (hardware log2 / exp2, fused multiply-adds and another
    summation order are what the kernels legitimately do differently), floored at 4 float32 ulp of the scale so that the clamp-only
    display models, whose float32 chain is a couple of ulp off, do not demand bit equality."""
    return 4.0 * max(e_ref, 4.0 * 2.0 ** -24)


def assert_channels_close(R, R32, R64, S64, label=""):
    """The check of the GPU tests: R (kernel output) against the float64 reference, bounded by the float32 chain's own error.
    Returns (error, e_ref)."""
    e_ref = channel_error(R32, R64, S64)
    err = channel_error(R, R64, S64)
    assert np.isfinite(np.asarray(R)).all(), label
    assert err <= error_bound(e_ref), "%s: max |R - R64| / S = %.3g > bound %.3g (e_ref %.3g)" % (label, err, error_bound(e_ref), e_ref)
    return err, e_ref


# ---- inputs --------------------------------------------------------------------------------------------------------------
# no zero and no one among the nine entries, rows summing to about 1 in luma: every product of the nine-term form is visible
DENSE_MATRIX = [[0.93, 0.21, 1.37], [1.06, -0.41, -0.66], [0.98, 1.69, 0.17]]


def yuv_clip(N, H, W, bit_depth, chroma_ss, seed):
    """(test, ref) codes [N, frame_elems], uint8 (8 bit) or uint16.  Every frame of every stream is drawn independently.  Frames cycle
    through three kinds:
      0  uniform random codes over the whole code range (illegal codes included: both clamps bind), pixel row 1 all 0, row 2 all max;
      1  bright only: Y in [100,235]*sc, chroma in [118,138]*sc (RGB stays above the sRGB toe);
      2  bright left of an odd column near 5W/8, random right of it."""
    rng = np.random.default_rng(seed)
    sc, top = 1 << (bit_depth - 8), (1 << bit_depth) - 1
    c420 = chroma_ss == "420"
    uvh, uvw = (H // 2, W // 2) if c420 else (H, W)
    split = ((5 * W) // 8) | 1
    csplit = (split + 1) // 2 if c420 else split

    def rand(h, w):
        return rng.integers(0, top + 1, (h, w))

    def bright(h, w, lo, hi):
        return rng.integers(lo * sc, hi * sc + 1, (h, w))
    out = []
    for s in range(2):
        frames = []
        for f in range(N):
            kind = f % 3
            if kind == 0:
                Y, U, V = rand(H, W), rand(uvh, uvw), rand(uvh, uvw)
                Y[1], Y[2] = 0, top
                for C in (U, V):
                    if c420:
                        C[0], C[1] = 0, top
                    else:
                        C[1], C[2] = 0, top
            else:
                Y, U, V = bright(H, W, 100, 235), bright(uvh, uvw, 118, 138), bright(uvh, uvw, 118, 138)
                if kind == 2:
                    Y[:, split:] = rand(H, W - split)
                    U[:, csplit:] = rand(uvh, uvw - csplit)
                    V[:, csplit:] = rand(uvh, uvw - csplit)
            frames.append(np.concatenate([Y.ravel(), U.ravel(), V.ravel()]))
        out.append(np.stack(frames).astype(np.uint8 if bit_depth == 8 else np.uint16))
    return out[0], out[1]


def photometry_for(model, dtype=np.float32):
    """The display models of the test matrix as oracle photometry objects (the product side is built by the GPU test)."""
    if model == "gamma2.4":
        return orc.Photometry(200, contrast=1000, EOTF="gamma", gamma=2.4, E_ambient=250, k_refl=0.005, dtype=dtype)
    if model == "absolute":
        return AbsolutePhotometry(10000, 0.005, dtype)
    return orc.Photometry.load(model, dtype=dtype)


MATRICES = {"bt709": [[1, 0, 1.402], [1, -0.344136, -0.714136], [1, 1.772, 0]],
            "bt2020nc": [[1, 0, 1.47460], [1, -0.16455, -0.57135], [1, 1.88140, 0]],
            "dense": DENSE_MATRIX}
_REFS = {}


def case_reference(H, W, bit_depth, chroma_ss, model, fps, matrix="bt709", padding="replicate", N=None, taps=None):
    """Clip and references of one test case, computed once per process and left unchanged: dict(test, ref [N, frame_elems] codes, N,
    fl, M (the colour matrix rounded to float32, as the kernels receive it), photometry, rgb2y, taps, idx, R64, S64, R32,
    bright_rgb_min (the smallest RGB value of the bright-only frames, both streams)).  N defaults to ring length + 3, so that each of
    the ring's straight-line FIR variants produces a live frame.  `taps`: the float32 taps handed to the code under test (the metric
    evaluates its filters with torch, whose exp / log differ from numpy's in the last bits; the taps are not the kernels' work);
    default: the oracle's."""
    fl = orc.filter_len(fps)
    taps = orc.temporal_filters(fps) if taps is None else np.ascontiguousarray(taps, dtype=np.float32)
    if N is None:
        N = (8 if fl <= 8 else 16 if fl <= 16 else 32 if fl <= 32 else 64) + 3
    key = (H, W, bit_depth, chroma_ss, model, fps, matrix, padding, N, taps.tobytes())
    if key in _REFS:
        return _REFS[key]
    seed = [H, W, bit_depth, int(chroma_ss), int(fps), N]
    test, ref = yuv_clip(N, H, W, bit_depth, chroma_ss, seed)
    M = np.asarray(MATRICES[matrix], dtype=np.float32)
    ph = photometry_for(model)
    rgb2y = orc.load_defaults()["color_spaces.json"]["BT.2020" if matrix == "bt2020nc" else "sRGB"]["RGB2Y"]
    idx = orc.window_frame_indices(N, fl, padding)
    args = (test, ref, W, H, bit_depth, chroma_ss, M, ph, rgb2y, taps, idx)
    R64, S64 = yuv_temporal_channels(*args, dtype=F64)
    R32, _ = yuv_temporal_channels(*args, dtype=np.float32)
    bright = min(float(yuv_rgb(s[f], W, H, bit_depth, chroma_ss, M, F64).min()) for s in (test, ref) for f in range(1, N, 3))
    for a in (test, ref, R64, S64, R32):
        a.setflags(write=False)
    c = dict(test=test, ref=ref, N=N, fl=fl, M=M, photometry=ph, rgb2y=rgb2y, taps=taps, idx=idx, R64=R64, S64=S64, R32=R32,
             bright_rgb_min=bright, args=args)
    _REFS[key] = c
    return c
