"""GPU: the array-source ingest kernels (temporal_vec_kernel, temporal_vec_half_kernel, temporal_ring_kernel,
temporal_ring_half_kernel, temporal_generic_kernel, luminance_frames_kernel), pixel by pixel, against a float64 statement of the
reference's chain (tests/array_channels_ref.py, pinned without a GPU by tests/test_array_ref_cpu.py).

Every case runs predict (sync=False, then fvvdp.finish) -- or, where the case needs a layout or a clip length predict cannot produce,
the C ABI through tests/lowlevel.py --, reads level 0 of the context and compares EVERY pixel of every frame and plane.  It also asserts
the exact list of FVVDP_DEBUG_VARIANT lines of temporal_channels_core (which kernel served every launch, with which ring, sample type,
channel count and display model), and that the out-of-range flag and warning equal the reference's.

The kernels index pixels flat, so only H*W matters; the frames are the smallest that hit every seam:
  vector kernel (a wave's block is 64*PX pixels, PX = 4 / 2 / 2 / 1 for the 8 / 16 / 32 / 64-slot ring, four waves per workgroup at 8)
    8x8 (64)      one partly filled wave, lanes clamped to HW - PX       8x32 (256)    exactly one block of the 8-slot ring
    4x65 (260)    one full block plus one live lane                      4x257 (1028)  a second workgroup, three waves return early
    12x171 (2052) two workgroups plus one lane                           10x77 (770)   even, no multiple of 4: vector at 16 / 32 / 64
  per-pixel ring (256 threads x PX = 4 / 4 / 2): 7x9 (63), 33x31 (1023), 25x41 (1025), 9x57 (513)
(770 and 513 pixels are 2x385 and 3x171 factored again, as 10x77 and 9x57: the library takes no frame with a side under 4.)  Frames
with a side of exactly 4 -- one band over a 2-row base level -- go through predict like the rest; test_predict_on_four_row_frames_vs_oracle
holds what predict returns there against the oracle.
uint8 is one kernel instantiation per (ring length, C), whatever the display model: the table's contents are data.  All five tables
run at FL 8 with C = 3; every other (FL, C) gets one model in rotation.  That reduction is deliberate (241 cases as it is).
The clips (array_channels_ref.array_clip) cycle through random samples over the whole range with a row of the smallest and a row of
the largest value, bright-only frames and frames bright on the left and dark (sRGB toe) on the right; N = ring length + 3 frames.

Tolerance (yuv_channels_ref.error_bound, unchanged): max |R_gpu - R64| / S <= 4 * max(e_ref, 4 * 2^-24), S = sum_k |tap_k| * L_k,
e_ref the same error of the reference's own float32 chain on the same clip, computed at run time.

The ticketed uint8 path of the 16-slot ring engages only when the grid exceeds twice the resident capacity: out of reach at these
sizes (test_ticketed_temporal_kernel_changes_no_bits covers it at full size); every line here must say `tickets 0`.

Measured on MI355X, worst case per display model over the four kernel families (error / S; e_ref of that case; share of the bound):
sRGB 6.3e-7 (3.6e-7, 0.45), PQ 3.3e-5 (3.4e-5, 0.24), gamma 2.4 6.8e-7 (3.4e-7, 0.49), linear 3.4e-7 (4.1e-7, 0.21), absolute 3.8e-7
(2.9e-7, 0.32); no kernel defect found, the tolerance is the YUV file's, unchanged.  The whole file (241 cases, three four-row oracle checks, the
coverage test): 245 tests in 5.7 s.  predict on the four-row frames: JOD equal to the oracle's to the printed six digits, Q_per_ch within 2.1e-6.  A single
pixel off by 1e-4 of S is seen behind every model but PQ (bound 1.2e-4 ... 1.6e-4 there).  The full table is in DESIGN.md, "Array
ingest, per pixel".
"""
import ctypes as C
import logging
import re

import numpy as np
import pytest
import torch

import array_channels_ref as aref

pytestmark = pytest.mark.gpu

VARIANT_RE = re.compile(r"array ingest: (vector|per-pixel|generic|luminance), FL (\d+), fl (\d+), dtype (\d), C (\d), eotf kind (\d), "
                        r"n_out (\d+), t0 (\d+), tickets (\d)")
MODELS = aref.MODELS
SRGB, PQ, GAMMA, LINEAR, ABSOLUTE = "standard_fhd", "standard_hdr_pq", "gamma2.4", "standard_hdr_linear", "absolute"
EOTF_KIND = {SRGB: 1, GAMMA: 2, PQ: 3, LINEAR: 4, ABSOLUTE: 5}          # FVVDP_EOTF_*; 0: code-value table, 6: none (luminance frames)
DT = {"uint8": 0, "uint16": 1, "float32": 2, "float16": 3, "bfloat16": 4}                      # FVVDP_U8 ...
T_MAX_IDX = 320                                                          # window index entries of one launch (temporal_kernels.hpp)
SZ_VEC = [(8, 8), (8, 32), (4, 65), (4, 257), (12, 171), (10, 77)]
SZ_VEC4 = SZ_VEC[:5]                                                     # H*W a multiple of 4: vector at every ring length
SZ_RING = [(7, 9), (33, 31), (25, 41), (9, 57)]
FPS_OF_FL = {8: 30, 16: 60, 32: 120, 64: 240}


def _case(family, path, H, W, C_ch, dtype, model, fps, exact16=False, scalar=False, padding="replicate", N=None, layout=None,
          outlier=None):
    """layout: None (predict, or the C ABI on contiguous tensors where predict cannot: see _driver), "offset" (C ABI, both source
    pointers one element past an aligned address), "stride" (C ABI, frames H*W + 1 elements apart), "frames4" / "frames1" (per-frame
    pointers at shuffled addresses, every distance a multiple of 4 elements / an odd distance)."""
    ident = "%s-%s-%dx%d-C%d-%s%s-%s-%gfps" % (family, path, H, W, C_ch, dtype, "-table" if exact16 else "", model, fps)
    ident += "".join("-" + s for s in (("scalar",) if scalar else ()) + ((padding,) if padding != "replicate" else ()) +
                     (("N%d" % N,) if N else ()) + ((layout,) if layout else ()) + ((outlier,) if outlier else ()))
    return pytest.param(dict(family=family, path=path, H=H, W=W, C=C_ch, dtype=dtype, model=model, fps=fps, exact16=exact16,
                             scalar=scalar, padding=padding, N=N, layout=layout, outlier=outlier), id=ident)


def _kinds(dtype):
    """(display model, table?) pairs a sample type meets: uint8 the table only, uint16 the table and every closed form, floats the
    closed forms."""
    if dtype == "uint8":
        return [(m, False) for m in MODELS]
    if dtype == "uint16":
        return [(m, False) for m in MODELS] + [(SRGB, True)]
    return [(m, False) for m in MODELS]


def _vector_cases():
    """A: every (ring length, sample type, channel count, display model) of the vector kernels: sizes rotate through them."""
    out, i = [], 0
    for FL in (8, 16, 32):
        sizes = SZ_VEC4 if FL == 8 else SZ_VEC
        for dtype in aref.DTYPES:
            for C_ch in (1, 3):
                kinds = _kinds(dtype)
                if dtype == "uint8" and not (FL == 8 and C_ch == 3):
                    kinds = [kinds[(FL // 8 + C_ch) % 5]]        # uint8 is one instantiation per (FL, C): all five tables at FL 8, C 3, else one
                for model, table in kinds:
                    H, W = sizes[i % len(sizes)]
                    i += 1
                    out.append(_case("A", "vector", H, W, C_ch, dtype, model, FPS_OF_FL[FL], exact16=table))
    # 64-slot ring: uint8, and 16-bit / float RGB behind sRGB and PQ
    for j, (dtype, C_ch, model) in enumerate([("uint8", 1, SRGB), ("uint8", 3, PQ)] +
                                             [(d, 3, m) for d in aref.DTYPES[1:] for m in (SRGB, PQ)]):
        H, W = SZ_VEC[j % 6]
        out.append(_case("A", "vector", H, W, C_ch, dtype, model, 240))
    return out


def _short_filter_cases():
    """B: filters shorter than their ring (25: 7 in 8, 50: 13 in 16, 90: 23 in 32, 144: 36 in 64; 60, 120 and 240 fps are family A)."""
    return [_case("B", "vector", 4, 65, 3, "uint8", SRGB, 25), _case("B", "vector", 8, 8, 1, "float32", PQ, 25),
            _case("B", "per-pixel", 25, 41, 3, "float16", GAMMA, 25),
            _case("B", "vector", 12, 171, 3, "uint16", PQ, 50), _case("B", "vector", 10, 77, 3, "bfloat16", SRGB, 50),
            _case("B", "per-pixel", 7, 9, 1, "uint8", SRGB, 50),
            _case("B", "vector", 8, 32, 1, "uint8", GAMMA, 90), _case("B", "vector", 4, 257, 3, "float16", SRGB, 90),
            _case("B", "per-pixel", 33, 31, 3, "uint16", LINEAR, 90),
            _case("B", "vector", 10, 77, 3, "uint8", SRGB, 144), _case("B", "vector", 7, 9, 3, "float32", PQ, 144),
            _case("B", "vector", 8, 8, 3, "float16", SRGB, 144), _case("B", "vector", 25, 41, 3, "uint16", SRGB, 144)]


def _ring_cases():
    """C: the per-pixel ring, every (ring length, sample type) with C = 3 through an odd frame size and with C = 1 through one of:
    FVVDP_TEMPORAL_SCALAR=1, a source pointer offset by one element, a frame stride that is no multiple of PX, 770 pixels at FL 8."""
    out, i = [], 0
    for FL in (8, 16, 32):
        for dtype in aref.DTYPES:
            model, table = _kinds(dtype)[i % len(_kinds(dtype))]
            H, W = SZ_RING[i % 4]
            out.append(_case("C", "per-pixel", H, W, 3, dtype, model, FPS_OF_FL[FL], exact16=table))
            model = MODELS[(i + 2) % 5]
            how = i % 4 if FL == 8 else i % 3
            if how == 0:
                out.append(_case("C", "per-pixel", *SZ_VEC4[i % 5], 1, dtype, model, FPS_OF_FL[FL], scalar=True))
            elif how == 1:
                out.append(_case("C", "per-pixel", 8, 32, 1, dtype, model, FPS_OF_FL[FL], layout="offset"))
            elif how == 2:
                out.append(_case("C", "per-pixel", 12, 171, 1, dtype, model, FPS_OF_FL[FL], layout="stride"))
            else:
                out.append(_case("C", "per-pixel", 10, 77, 1, dtype, model, 30))
            i += 1
    return out


CASES = _vector_cases() + _short_filter_cases() + _ring_cases() + [
    # D: 144 / 240 fps outside k1_ring64_ok: luminance frames first, then the 64-slot ring on them (float32, C 1, no display model)
    _case("D", "two-pass", 8, 32, 3, "uint16", GAMMA, 240), _case("D", "two-pass", 7, 9, 3, "uint16", SRGB, 144, exact16=True),
    _case("D", "two-pass", 4, 65, 3, "float32", LINEAR, 144), _case("D", "two-pass", 12, 171, 3, "bfloat16", ABSOLUTE, 240),
    _case("D", "two-pass", 33, 31, 3, "float16", GAMMA, 144), _case("D", "two-pass", 10, 77, 1, "float32", SRGB, 240),
    _case("D", "two-pass", 25, 41, 1, "uint16", PQ, 240), _case("D", "two-pass", 4, 257, 1, "float16", SRGB, 144),
    _case("D", "two-pass", 9, 57, 1, "bfloat16", PQ, 144), _case("D", "two-pass", 8, 8, 1, "float16", PQ, 240),
    # E: the generic kernel.  Still images (planes == 2) for every sample type at 63 and 1028 pixels ...
    _case("E", "generic", 7, 9, 3, "uint8", SRGB, 0), _case("E", "generic", 4, 257, 1, "uint8", PQ, 0),
    _case("E", "generic", 7, 9, 1, "uint16", PQ, 0), _case("E", "generic", 4, 257, 3, "uint16", SRGB, 0, exact16=True),
    _case("E", "generic", 7, 9, 3, "float32", PQ, 0), _case("E", "generic", 4, 257, 1, "float32", LINEAR, 0),
    _case("E", "generic", 7, 9, 1, "float16", SRGB, 0), _case("E", "generic", 4, 257, 3, "float16", GAMMA, 0),
    _case("E", "generic", 7, 9, 3, "bfloat16", ABSOLUTE, 0), _case("E", "generic", 4, 257, 1, "bfloat16", SRGB, 0),
    # ... 300 fps (75 taps, tables through device memory) and 240 fps under FVVDP_TEMPORAL_SCALAR=1
    _case("E", "generic", 7, 9, 3, "uint8", SRGB, 300, N=6), _case("E", "generic", 4, 65, 1, "float32", PQ, 300, N=6),
    _case("E", "generic", 8, 8, 3, "uint8", SRGB, 240, scalar=True, N=5), _case("E", "generic", 7, 9, 3, "float16", PQ, 240, scalar=True, N=5),
    # F: clips longer than one launch's index list: 313 + 7 frames at 30 fps, 257 + 5 at 240 fps
    _case("F", "vector", 8, 8, 3, "uint8", SRGB, 30, N=320), _case("F", "vector", 4, 65, 1, "uint8", PQ, 30, N=320),
    _case("F", "vector", 8, 8, 1, "float32", PQ, 30, N=320), _case("F", "vector", 4, 65, 3, "float32", SRGB, 30, N=320),
    _case("F", "vector", 8, 8, 1, "uint8", SRGB, 240, N=262), _case("F", "vector", 4, 65, 3, "uint8", PQ, 240, N=262),
    _case("F", "vector", 8, 8, 3, "float32", SRGB, 240, N=262), _case("F", "vector", 4, 65, 3, "float32", PQ, 240, N=262),
    # G: the other temporal paddings at the shortest and the longest ring ...
    _case("G", "vector", 8, 32, 3, "uint8", SRGB, 30, padding="circular"), _case("G", "vector", 12, 171, 3, "float32", PQ, 30, padding="pingpong"),
    _case("G", "vector", 4, 65, 3, "uint8", SRGB, 240, padding="pingpong"), _case("G", "vector", 10, 77, 3, "bfloat16", PQ, 240, padding="circular"),
    _case("G", "two-pass", 8, 8, 1, "float32", GAMMA, 144, padding="circular"),
    # ... and float clips whose ONLY sample outside [0,1] is one channel of the last pixel of the last reference frame: 1 + 2^-23 or
    # -1e-6.  Behind a model that clips the flag fires, behind the linear and the absolute model it does not.  (Every other float
    # case holds exact 0.0 and 1.0 and nothing outside: no flag.)
    _case("G", "vector", 8, 8, 3, "float32", SRGB, 30, outlier="above"), _case("G", "vector", 12, 171, 3, "float32", SRGB, 60, outlier="below"),
    _case("G", "vector", 4, 65, 1, "float32", PQ, 120, outlier="above"), _case("G", "vector", 8, 32, 3, "float32", PQ, 240, outlier="below"),
    _case("G", "per-pixel", 7, 9, 3, "float32", GAMMA, 30, outlier="above"), _case("G", "two-pass", 25, 41, 1, "float32", GAMMA, 144, outlier="below"),
    _case("G", "generic", 7, 9, 3, "float32", SRGB, 0, outlier="above"),
    _case("G", "vector", 8, 8, 3, "float32", LINEAR, 30, outlier="above"), _case("G", "vector", 8, 32, 1, "float32", LINEAR, 60, outlier="below"),
    _case("G", "vector", 4, 65, 3, "float32", ABSOLUTE, 30, outlier="below"), _case("G", "per-pixel", 33, 31, 1, "float32", ABSOLUTE, 60, outlier="above"),
    # H: per-frame source pointers (fvvdp_temporal_channels_frames), test and reference frames at differently shuffled addresses
    _case("H", "vector", 8, 32, 3, "uint8", SRGB, 60, layout="frames4"), _case("H", "per-pixel", 8, 32, 3, "uint8", SRGB, 60, layout="frames1"),
    _case("H", "vector", 4, 65, 1, "float32", PQ, 30, layout="frames4"), _case("H", "per-pixel", 4, 65, 1, "float32", PQ, 30, layout="frames1"),
]


def _ring64_ok(dt, C_ch, kind):                                          # k1_ring64_ok (temporal_launch.hpp)
    return dt == 0 or (C_ch == 3 and kind in (1, 3)) or (dt == 2 and C_ch == 1 and kind == 6)


def _kind(c):
    return 0 if (c["dtype"] == "uint8" or c["exact16"]) else EOTF_KIND[c["model"]]


def _frames(c):
    if not c["fps"]:
        return 1, 1
    fl = aref.orc.filter_len(c["fps"])
    return fl, (c["N"] or aref.ring_length(fl) + 3)


def _expected_variants(c):
    """The FVVDP_DEBUG_VARIANT lines of the case, from the dispatch rules of temporal_channels_core restated: (kernel, FL, fl, dtype, C,
    eotf kind, n_out, t0, tickets)."""
    fl, N = _frames(c)
    dt, C_ch, kind, HW = DT[c["dtype"]], c["C"], _kind(c), c["H"] * c["W"]
    if not c["fps"] or fl > 64 or (fl > 32 and c["scalar"]):
        return [("generic", 0, fl, dt, C_ch, kind, N, 0, 0)]
    pre = []
    if fl > 32 and not _ring64_ok(dt, C_ch, kind):
        assert fl - 1 + N <= T_MAX_IDX
        pre = [("luminance", 0, fl, dt, C_ch, kind, N, 0, 0)]           # (every padding here uses all N frames, or all but frame 0)
        if c["padding"] == "circular":
            pre = [("luminance", 0, fl, dt, C_ch, kind, N - 1, 0, 0)]   # circular: frame 0 is in no window
        dt, C_ch, kind = 2, 1, 6
    FL = aref.ring_length(fl)
    PX = {8: 4, 16: 2, 32: 2, 64: 1}[FL]
    aligned = c["layout"] not in ("offset", "stride", "frames1") or PX == 1
    vec = (not c["scalar"]) and HW % PX == 0 and aligned
    max_out = T_MAX_IDX - (FL - 1)
    return pre + [("vector" if vec else "per-pixel", FL, fl, dt, C_ch, kind, min(max_out, N - t0), t0, 0) for t0 in range(0, N, max_out)]


def _path(lines):
    return "two-pass" if lines[0][0] == "luminance" else lines[0][0]


def _driver(c):
    """"predict" wherever predict can produce the launch; the C ABI for the layouts and for the 240 fps clip longer than predict's
    batch of 128 frames."""
    if c["layout"] or (c["N"] or 0) > 128 and c["fps"] > 128:
        return "abi"
    return "predict"


_METRICS = {}


def _metric(c, batch):
    import fovvideovdp_amd as fv
    key = (c["model"], c["padding"], c["exact16"], batch)
    if key not in _METRICS:
        if c["model"] == GAMMA:
            ph = fv.fvvdp_display_photo_eotf(200, contrast=1000, EOTF="gamma", gamma=2.4, E_ambient=250, k_refl=0.005)
        elif c["model"] == ABSOLUTE:
            ph = fv.fvvdp_display_photo_absolute(10000, 0.005)
        else:
            ph = fv.fvvdp_display_photometry.load(c["model"])
        m = fv.fvvdp(display_name="standard_fhd", display_photometry=ph, temp_padding=c["padding"], batch_frames=batch)
        if c["exact16"]:
            m.exact_uint16 = True
        _METRICS[key] = m
    m = _METRICS[key]
    m._drop_context()                       # (the library reads its switches when a context is created)
    return m


def _tensor(a):
    """A clip of the reference as a torch tensor of the product's sample type (uint16 travels as int16 bits)."""
    if isinstance(a, torch.Tensor):
        return a.clone()
    a = a.copy()
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def _eotf(m, c, keep):
    """fvvdp_eotf of the case, as fvvdp._make_feeder fills it."""
    from fovvideovdp_amd import _native as nat
    from fovvideovdp_amd.display_model import native_eotf
    e = nat.Eotf()
    if _kind(c) == 0:
        lut = m._code_lut(m.display_photometry, 8 if c["dtype"] == "uint8" else 16)
        keep.append(lut)
        e.kind, e.d_lut = nat.EOTF_LUT, lut.data_ptr()
        e.L_min, e.L_max = m._lut_dev.table_range(lut)
    else:
        kind, d = native_eotf(m.display_photometry)
        e.kind, e.Y_peak, e.Y_black, e.gamma = kind, d.get("Y_peak", 0.0), d.get("Y_black", 0.0), d.get("gamma", 1.0)
        e.L_min, e.L_max = d.get("L_min", 0.0), d.get("L_max", 0.0)
    assert e.kind == _kind(c)
    return e


def _place(t, c, which):
    """Device copy of clip t [1,C,N,H,W] in the layout of the case: (tensor that owns the memory, address of sample 0, chan_stride,
    frame_stride in elements; per-frame addresses for the frames layouts)."""
    Cc, N, HW = c["C"], t.shape[2], c["H"] * c["W"]
    flat = t.reshape(Cc, N, HW).cuda()
    es = flat.element_size()
    lay = c["layout"]
    if lay is None:
        return flat, flat.data_ptr(), N * HW, HW, None
    if lay == "offset":
        buf = torch.zeros(flat.numel() + 16, dtype=flat.dtype, device="cuda")
        buf[1:1 + flat.numel()] = flat.reshape(-1)
        assert buf.data_ptr() % 16 == 0
        return buf, buf.data_ptr() + es, N * HW, HW, None
    if lay == "stride":
        buf = torch.zeros((Cc, N, HW + 1), dtype=flat.dtype, device="cuda")
        buf[:, :, :HW] = flat
        return buf, buf.data_ptr(), N * (HW + 1), HW + 1, None
    # per-frame pointers: frame f of this stream lives in slot perm[f]; a slot holds the C planes of one frame, chan_stride HW apart
    pad = 8 if lay == "frames4" else 7
    slot = Cc * HW + pad
    perm = np.random.default_rng([which, N]).permutation(N)
    buf = torch.zeros(N * slot + 16, dtype=flat.dtype, device="cuda")
    for f in range(N):
        buf[perm[f] * slot:perm[f] * slot + Cc * HW] = flat[:, f].reshape(-1)
    assert buf.data_ptr() % 16 == 0 and (slot % 4 == 0) == (lay == "frames4")
    return buf, None, HW, None, [buf.data_ptr() + int(perm[f]) * slot * es for f in range(N)]


def _run_abi(m, c, r, taps):
    """The temporal pass alone through the C ABI: level 0 [N,P,H,W] and the out-of-range flag."""
    from fovvideovdp_amd import _native as nat
    from lowlevel import Pipeline
    H, W, N, fl = c["H"], c["W"], r["N"], r["fl"]
    keep = []
    e = _eotf(m, c, keep)
    idx = np.zeros(1, np.int32) if r["idx"] is None else np.concatenate([r["idx"][0], r["idx"][1:, -1]]).astype(np.int32)
    assert len(idx) == fl - 1 + N
    bt, pt, cs, fs, ft = _place(_tensor(r["test"]), c, 0)
    br, pr, _, _, fr = _place(_tensor(r["ref"]), c, 1)
    oob = torch.zeros(1, dtype=torch.int32, device="cuda")
    pipe = Pipeline(m, W, H, 2 if r["idx"] is None else 4, N)
    try:
        w = nat.fptr(np.ascontiguousarray(m._rgb2y(), dtype=np.float32)) if c["C"] == 3 else None
        tp = np.ascontiguousarray(taps, dtype=np.float32)
        if ft is None:
            nat.check(pipe.lib.fvvdp_temporal_channels(pipe.handle, C.c_void_p(pt), C.c_void_p(pr), DT[c["dtype"]], c["C"], cs, fs,
                                                       C.byref(e), w, idx.ctypes.data_as(C.POINTER(C.c_int32)), nat.fptr(tp), fl, N, 0,
                                                       C.c_void_p(oob.data_ptr()), pipe.stream()))
        else:
            assert ft != fr and [a - ft[0] for a in ft] != [a - fr[0] for a in fr]       # the two streams' index lists differ
            nat.check(pipe.lib.fvvdp_temporal_channels_frames(pipe.handle, (C.c_void_p * N)(*ft), (C.c_void_p * N)(*fr), N, DT[c["dtype"]],
                                                              c["C"], cs, C.byref(e), w, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                                              nat.fptr(tp), fl, N, 0, C.c_void_p(oob.data_ptr()), pipe.stream()))
        R = pipe.export_level(0, N).cpu().numpy()
        flag = int(oob.cpu()[0])
    finally:
        pipe.close()
    del bt, br, keep
    return R, flag


def _run_predict(m, c, r, caplog):
    """predict(sync=False) + finish: level 0, the flag in stats['range_flag'] and whether the warning was logged."""
    import fovvideovdp_amd as fv
    from fovvideovdp_amd import _native as nat
    H, W, N = c["H"], c["W"], r["N"]
    t, rf = _tensor(r["test"]), _tensor(r["ref"])
    with caplog.at_level(logging.WARNING):
        if r["idx"] is None:
            order = "HWC" if c["C"] == 3 else "HW"
            t, rf = (x[0, :, 0].permute(1, 2, 0).contiguous() if c["C"] == 3 else x[0, 0, 0].contiguous() for x in (t, rf))
            q, st = m.predict(t, rf, dim_order=order, sync=False)
        else:
            q, st = m.predict(t, rf, dim_order="BCFHW", frames_per_second=c["fps"], sync=False)
        flag = int(st["range_flag"].cpu()[0])
        fv.fvvdp.finish(st)
    P = 2 if r["idx"] is None else 4
    out = torch.empty((N, P, H, W), dtype=torch.float32, device="cuda")
    nat.check(nat.lib().fvvdp_export_level(m._ctx.handle, 0, N, C.c_void_p(out.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    R = out.cpu().numpy()
    assert np.isfinite(float(q)) and np.isfinite(st["Q_per_ch"]).all()
    warned = any("outside the valid range" in rec.message for rec in caplog.records)
    assert warned == (flag != 0)
    return R, flag


@pytest.mark.parametrize("c", CASES)
def test_array_ingest_per_pixel(c, monkeypatch, capfd, caplog):
    monkeypatch.delenv("FVVDP_TEMPORAL_SCALAR", raising=False)
    monkeypatch.delenv("FVVDP_K1_TICKET", raising=False)
    if c["scalar"]:
        monkeypatch.setenv("FVVDP_TEMPORAL_SCALAR", "1")
    monkeypatch.setenv("FVVDP_DEBUG_VARIANT", "1")
    fl, N = _frames(c)
    drv = _driver(c)
    m = _metric(c, N if (drv == "predict" and N > 128) else None)
    taps = m._temporal_taps(c["fps"])[1] if c["fps"] else None
    r = aref.case_reference(c["H"], c["W"], c["C"], c["dtype"], c["model"], c["fps"], c["padding"], N=c["N"], taps=taps,
                            outlier=c["outlier"])
    assert (r["N"], r["fl"]) == (N, fl)
    if c["dtype"] == "uint16":
        assert (r["test"] >= 32768).any() and (r["ref"] >= 32768).any()       # negative as int16: a sign extension would show
    if N >= 2:
        assert r["bright_min"] > 0.05                                          # the bright frames never need the sRGB toe
    if c["outlier"]:
        assert r["oob"] == (c["model"] in (SRGB, PQ, GAMMA))
    elif c["dtype"] in aref.FLOAT_DTYPES and c["model"] in (SRGB, PQ, GAMMA):
        t = aref.as_float_numpy(r["test"])
        assert t.min() == 0.0 and t.max() == 1.0 or N == 1                     # exact 0.0 and 1.0, nothing outside
        assert not r["oob"]
    want = _expected_variants(c)
    assert _path(want) == c["path"], (want, c["path"])                         # the case list says what each case is for
    capfd.readouterr()
    caplog.clear()
    if drv == "abi":
        R, flag = _run_abi(m, c, r, taps if taps is not None else np.ones((2, 1), np.float32))
    else:
        R, flag = _run_predict(m, c, r, caplog)
    m._drop_context()
    ran = [(g[0],) + tuple(int(x) for x in g[1:]) for g in VARIANT_RE.findall(capfd.readouterr().err)]
    assert ran == want, (ran, want)
    assert all(x[8] == 0 for x in ran)
    assert (flag != 0) == r["oob"], (flag, r["oob"])
    e_ref = aref.channel_error(r["R32"], r["R64"], r["S64"])
    err = aref.channel_error(R, r["R64"], r["S64"])
    print("\narray-pixels %s %s %s FL %d C %d %s: err %.3g e_ref %.3g bound %.3g" % (
        c["family"], c["model"], c["path"], want[-1][1], c["C"], c["dtype"] + ("-table" if c["exact16"] else ""), err, e_ref,
        aref.error_bound(e_ref)))
    if err > aref.error_bound(e_ref):
        d = np.abs(R.astype(np.float64) - r["R64"]) / r["S64"]
        print("array-pixels worst (frame, plane, y, x):", np.unravel_index(int(np.argmax(d)), d.shape))
    aref.assert_channels_close(R, r["R32"], r["R64"], r["S64"], label=str(c))


@pytest.mark.parametrize("N,H,W,fps", [(11, 4, 65, 30), (1, 4, 257, 0), (11, 4, 257, 30)])
def test_predict_on_four_row_frames_vs_oracle(N, H, W, fps):
    """The 260- and 1028-pixel frames above have 4 rows, the smallest side the library takes: one band over a 2-row base level, a
    height no other test gives the pyramid pass.  What predict returns there, on the smooth synthetic pair, against the oracle: JOD
    within the project's bound of 1e-3, Q_per_ch within the 4e-3 the suite applies to its other tiny frames (36x64)."""
    import fovvideovdp_amd as fv
    from fovvideovdp_amd.synth import synth_video_pair
    test, ref = synth_video_pair(N, H, W)
    m = fv.fvvdp(display_name="standard_fhd")
    o = aref.orc.Oracle("standard_fhd")
    if fps:
        q, st = m.predict(test, ref, frames_per_second=fps)
        oq, ost = o.predict(test.numpy(), ref.numpy(), frames_per_second=fps)
    else:
        t, r = (x[0, :, 0].permute(1, 2, 0).contiguous() for x in (test, ref))
        q, st = m.predict(t, r, dim_order="HWC")
        oq, ost = o.predict(t.numpy(), r.numpy(), dim_order="HWC")
    Q, oQ = np.asarray(st["Q_per_ch"], np.float64), np.asarray(ost["Q_per_ch"], np.float64)
    assert Q.shape == oQ.shape
    rel = float(np.max(np.abs(Q - oQ) / (np.abs(oQ) + 1e-3 * np.max(np.abs(oQ)))))
    print("\narray-pixels four rows %dx%dx%d: JOD %.6f oracle %.6f, Q_per_ch rel %.3g" % (N, H, W, float(q), float(oq), rel))
    assert abs(float(q) - float(oq)) < 1e-3
    assert rel < 4e-3


def test_cases_cover_every_instantiation_axis():
    """Each case asserts its own variant lines, so the list itself shows what was covered."""
    cs = [p.values[0] for p in CASES]
    lines = [x for c in cs for x in _expected_variants(c)]
    vec = {x[1:6] for x in lines if x[0] == "vector"}                          # (FL, fl, dtype, C, kind)
    want = set()
    for FL in (8, 16, 32):
        for C_ch in (1, 3):
            want.add((FL, 0, C_ch, 0))                                         # uint8: the table
            want |= {(FL, 1, C_ch, k) for k in range(6)}                       # uint16: the table and every closed form
            want |= {(FL, d, C_ch, k) for d in (2, 3, 4) for k in range(1, 6)}
    want |= {(64, 0, 1, 0), (64, 0, 3, 0), (64, 2, 1, 6)} | {(64, d, 3, k) for d in (1, 2, 3, 4) for k in (1, 3)}
    have = {(x[0], x[2], x[3], x[4]) for x in vec}
    assert have >= want, sorted(want - have)
    assert {(64, d, C_ch, k) for (FL, d, C_ch, k) in have if FL == 64} == {x for x in want if x[0] == 64}     # what the host allows
    ring = {(x[1], x[3], x[4]) for x in lines if x[0] == "per-pixel"}
    assert ring == {(FL, d, C_ch) for FL in (8, 16, 32) for d in range(5) for C_ch in (1, 3)}
    assert {fl for (_, fl, _, _, _) in vec} >= {7, 8, 13, 15, 23, 30, 36, 60}   # filters shorter than their ring
    gen = [(c, x) for c in cs for x in _expected_variants(c) if x[0] == "generic"]
    assert {x[3] for c, x in gen if not c["fps"]} == set(range(5)) and {c["H"] * c["W"] for c, x in gen if not c["fps"]} == {63, 1028}
    assert {x[2] for c, x in gen if c["fps"]} == {60, 75}                       # planes == 4
    assert {x[3] for x in lines if x[0] == "luminance"} == {1, 2, 3, 4}         # (uint8 always has the 64-slot ring)
    assert {c["H"] * c["W"] for c in cs if _path(_expected_variants(c)) == "vector"} >= {64, 256, 260, 1028, 2052, 770}
    assert {c["H"] * c["W"] for c in cs if _path(_expected_variants(c)) == "per-pixel"} >= {63, 1023, 1025, 513, 770}
    assert {(c["H"], c["W"]) for c in cs} >= set(SZ_VEC) | set(SZ_RING)
    assert max(c["H"] * c["W"] for c in cs) <= 2052
    split = [c for c in cs if len([x for x in _expected_variants(c) if x[0] != "luminance"]) == 2]
    assert {(c["fps"], c["N"], c["H"] * c["W"], c["dtype"]) for c in split} == {(f, n, s, d) for (f, n) in ((30, 320), (240, 262))
                                                                               for s in (64, 260) for d in ("uint8", "float32")}
    assert {c["layout"] for c in cs} == {None, "offset", "stride", "frames4", "frames1"}
    assert {c["padding"] for c in cs} == {"replicate", "circular", "pingpong"}
