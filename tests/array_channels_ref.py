"""Float64 yardstick for the array-source ingest kernels (temporal_vec_kernel, temporal_vec_half_kernel, temporal_ring_kernel,
temporal_ring_half_kernel, temporal_generic_kernel, luminance_frames_kernel): uint8 / uint16 / float32 / float16 / bfloat16 samples,
C = 1 or 3 -> display model -> luminance -> temporal channels, built from the oracle's frame_luminance and temporal_channels in a
chosen precision.  With dtype=np.float32 it IS the reference's float32 chain, bit for bit, which gives every test case its own baseline
error.  TEST INFRASTRUCTURE: numpy (torch only to hold half-precision clips, which numpy cannot: bfloat16), no GPU;
tests/test_array_ref_cpu.py pins it against the oracle and the reference's golden vectors.

The comparison (`channel_error`, `error_bound`, `assert_channels_close`) and the display models (`photometry_for`, `AbsolutePhotometry`)
are those of the YUV yardstick, tests/yuv_channels_ref.py.  Also here, because the CPU tests and the GPU tests must share them: the
random clips (`array_clip`) and the per-process cache of a case's clip and references (`case_reference`).
"""
import copy

import numpy as np

from oracle import fvvdp_oracle as orc
from yuv_channels_ref import AbsolutePhotometry, assert_channels_close, channel_error, error_bound, photometry_for  # noqa: F401

F64 = np.float64
INT_TOP = {"uint8": 255, "uint16": 65535}
FLOAT_DTYPES = ("float32", "float16", "bfloat16")
DTYPES = ("uint8", "uint16") + FLOAT_DTYPES
MODELS = ["standard_fhd", "standard_hdr_pq", "gamma2.4", "standard_hdr_linear", "absolute"]
PEAK = {"standard_hdr_linear": 1500.0, "absolute": 10000.0}     # models whose float content is cd/m^2: peak of the display
TOE = 0.04045                                                   # sRGB: samples at or below it take the linear segment


def as_float_numpy(clip):
    """A clip as numpy: uint8 / uint16 / float32 arrays as they are, half-precision torch tensors upcast to float32 (exact)."""
    if isinstance(clip, np.ndarray):
        return clip
    import torch
    assert clip.dtype in (torch.float16, torch.bfloat16), clip.dtype
    return clip.to(torch.float32).numpy()


def array_temporal_channels(test, ref, photometry, rgb2y, taps32, idx, dtype=F64):
    """Temporal channels of an array clip pair.  test / ref: [1,C,N,H,W] (numpy uint8 / uint16 / float32, or torch float16 /
    bfloat16); photometry: an oracle Photometry (or AbsolutePhotometry); taps32: float32 [2, fl]; idx: [N, fl] from
    window_frame_indices, or None for a still image (N = 1: the two luminance planes themselves, S = R).
    Returns (R, S): R [N,4,H,W] ([1,2,H,W] for a still image) in the plane order of level 0 (sustained test, sustained reference,
    transient test, transient reference) and the per-pixel error scale S = sum_k |taps[cc][k]| * L_s[window slot k], both in `dtype`."""
    F = dtype
    ph = copy.copy(photometry)
    ph.dtype = F
    clips = (as_float_numpy(test), as_float_numpy(ref))
    lum = [{}, {}]

    def L(s, f):
        if f not in lum[s]:
            lum[s][f] = orc.frame_luminance(clips[s], f, ph, rgb2y, F)[0]
        return lum[s][f]
    if idx is None:
        R = np.stack([L(0, 0), L(1, 0)])[None].astype(F)
        return R, R.copy()
    taps = np.asarray(taps32, dtype=np.float32).astype(F)
    N, fl = idx.shape
    assert taps.shape == (2, fl)
    H, W = clips[0].shape[-2:]
    R = np.zeros((N, 4, H, W), dtype=F)
    S = np.zeros((N, 4, H, W), dtype=F)
    a = np.abs(taps)
    for ff in range(N):
        win = [np.stack([L(s, int(j)) for j in idx[ff]], 0) for s in range(2)]        # oldest first
        R[ff] = orc.temporal_channels(win[0], win[1], taps, F)
        S[ff] = orc.temporal_channels(win[0], win[1], a, F)
    return R, S


def array_out_of_range(test, ref, photometry, idx):
    """The reference's out-of-range flag: some frame the windows use holds a sample outside [0,1] behind a display model that clips."""
    clips = (as_float_numpy(test), as_float_numpy(ref))
    ph = copy.copy(photometry)
    ph.dtype = np.float32
    frames = [0] if idx is None else sorted(set(int(j) for j in np.asarray(idx).ravel()))
    return any(bool(ph.forward(orc.frame_to_unit(c, f, np.float32))[1]) for c in clips for f in frames)


# ---- inputs --------------------------------------------------------------------------------------------------------------
def array_clip(N, H, W, C, dtype, model, seed, outlier=None):
    """(test, ref) [1,C,N,H,W]: numpy uint8 / uint16 / float32, torch float16 / bfloat16.  Every frame of every stream is drawn
    independently.  Frames cycle through three kinds:
      0  random over the whole range.  Integer types: every code, pixel row 1 all 0, row 2 all max.  Float types: [0,1] with row 1
         exactly 0.0 and row 2 exactly 1.0 (float16: every third sample of row 0 subnormal); behind the linear and the absolute
         model 0.001 ... 1.2 x peak, log-uniform, row 1 all 0.001 and row 2 all 1.2 x peak, so that both clamps bind;
      1  bright only: no sample below 0.2 of the range (none in the sRGB toe);
      2  bright left of an odd column near 5W/8, dark right of it (at or below the toe threshold 0.04045).
    `outlier` ("above" / "below", float32 only): [0,1] content behind every model, and the last channel of the last pixel of the last frame of the reference stream becomes
    1 + 2^-23 / -1e-6."""
    assert H >= 3 and dtype in DTYPES
    rng = np.random.default_rng(seed)
    split = ((5 * W) // 8) | 1
    wide = dtype in FLOAT_DTYPES and model in PEAK and outlier is None      # (an outlier clip is [0,1] content behind every model)
    out = []
    for s in range(2):
        frames = []
        for f in range(N):
            kind = f % 3
            if dtype in INT_TOP:
                top = INT_TOP[dtype]
                if kind == 0:
                    a = rng.integers(0, top + 1, (C, H, W))
                    a[:, 1], a[:, 2] = 0, top
                else:
                    a = rng.integers(top // 5, top + 1, (C, H, W))
                    if kind == 2:
                        a[:, :, split:] = rng.integers(0, int(TOE * top) + 1, (C, H, W - split))
            elif wide:
                peak = PEAK[model]
                if kind == 0:
                    a = np.exp(rng.uniform(np.log(0.001), np.log(1.2 * peak), (C, H, W)))
                    a[:, 1], a[:, 2] = 0.001, 1.2 * peak
                else:
                    a = rng.uniform(0.2 * peak, peak, (C, H, W))
                    if kind == 2:
                        a[:, :, split:] = rng.uniform(0.001, 0.04, (C, H, W - split))
            else:
                if kind == 0:
                    a = rng.uniform(0.0, 1.0, (C, H, W))
                    if dtype == "float16":
                        a[:, 0, ::3] = rng.integers(1, 1024, a[:, 0, ::3].shape) * 2.0 ** -24
                    a[:, 1], a[:, 2] = 0.0, 1.0
                else:
                    a = rng.uniform(0.2, 1.0, (C, H, W))
                    if kind == 2:
                        a[:, :, split:] = rng.uniform(0.0, 0.04, (C, H, W - split))      # (0.04: still under the toe after rounding to bfloat16)
            frames.append(a)
        clip = np.stack(frames, 1)[None]                       # [1,C,N,H,W]
        if dtype in INT_TOP:
            clip = clip.astype(np.uint8 if dtype == "uint8" else np.uint16)
        else:
            clip = clip.astype(np.float32)
            if outlier is not None and s == 1:
                assert dtype == "float32"
                clip[0, C - 1, N - 1, H - 1, W - 1] = {"above": np.float32(1) + np.float32(2.0 ** -23), "below": np.float32(-1e-6)}[outlier]
            if dtype != "float32":
                import torch
                clip = torch.from_numpy(clip).to(torch.float16 if dtype == "float16" else torch.bfloat16)
        out.append(clip)
    return out[0], out[1]


def ring_length(fl):
    return 8 if fl <= 8 else 16 if fl <= 16 else 32 if fl <= 32 else 64


_REFS = {}


def case_reference(H, W, C, dtype, model, fps, padding="replicate", N=None, taps=None, outlier=None):
    """Clip and references of one test case, computed once per process and left unchanged: dict(test, ref [1,C,N,H,W], N, fl,
    photometry, rgb2y, taps, idx, R64, S64, R32, oob (the reference's out-of-range flag), bright_min (the smallest sample of the
    bright-only frames as a fraction of the range, both streams), args).  fps = 0: a still image (N = 1, idx None, two planes).
    N defaults to ring length + 3, so that each straight-line step of a register ring produces a live frame.  `taps`: the float32 taps
    handed to the code under test (the metric's, evaluated with torch); default: the oracle's.  A uint16 clip has ONE reference
    (code / 65535 through forward()), whether the product reads a code-value table or evaluates the closed form."""
    still = not fps
    if still:
        fl, N, taps, idx = 1, 1, np.ones((2, 1), dtype=np.float32), None
    else:
        fl = orc.filter_len(fps)
        taps = orc.temporal_filters(fps) if taps is None else np.ascontiguousarray(taps, dtype=np.float32)
        if N is None:
            N = ring_length(fl) + 3
    key = (H, W, C, dtype, model, fps, padding, N, taps.tobytes(), outlier)
    if key in _REFS:
        return _REFS[key]
    seed = [H, W, C, DTYPES.index(dtype), MODELS.index(model), int(fps), N]
    test, ref = array_clip(N, H, W, C, dtype, model, seed, outlier)
    ph = photometry_for(model)
    rgb2y = orc.load_defaults()["color_spaces.json"]["sRGB"]["RGB2Y"]
    if not still:
        idx = orc.window_frame_indices(N, fl, padding)
    args = (test, ref, ph, rgb2y, taps, idx)
    R64, S64 = array_temporal_channels(*args, dtype=F64)
    R32, _ = array_temporal_channels(*args, dtype=np.float32)
    t, r = as_float_numpy(test), as_float_numpy(ref)
    unit = INT_TOP.get(dtype, PEAK[model] if (model in PEAK and outlier is None) else 1.0)
    b = [s[:, :, 1::3].copy() for s in (t, r)]
    if outlier is not None and (N - 1) % 3 == 1:
        b[1][0, C - 1, -1, -1, -1] = 1.0                      # (the planted sample is not the content)
    bright = min(float(s.min()) for s in b) / unit if N > 1 else None
    for a in (t, r, R64, S64, R32):
        a.setflags(write=False)
    c = dict(test=test, ref=ref, N=N, fl=fl, photometry=ph, rgb2y=rgb2y, taps=taps, idx=idx, R64=R64, S64=S64, R32=R32,
             oob=array_out_of_range(test, ref, ph, idx), bright_min=bright, args=args)
    _REFS[key] = c
    return c
