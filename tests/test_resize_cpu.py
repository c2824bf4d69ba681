"""Mixed-resolution clips without a GPU: the header and its binding, the argument checks of its two entry points, every refusal of
fvvdp.predict_resized / fvvdp.jod_video_resized that comes before any device work, the numpy restatement (tests/resize_ref.py)
against torch.nn.functional.interpolate, against the inner-product identity and against torch autograd, the margin of the case
inputs, the code objects of the new kernels, and the goldens."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_cases as rc                    # noqa: E402
import resize_ref as rref                    # noqa: E402

U24 = 2.0 ** -24
WEIGHT_ULPS = 4              # see test_axis_matrices_are_torchs
NEW_KERNELS = ["void resized_ring_kernel<%d, %d, %d>" % (fl, 2 if fl <= 16 and m <= 1 else 1, m) for fl in (8, 16, 32) for m in range(4)] + \
    ["void resize_adjoint_d_kernel<%d>" % m for m in range(5)] + ["void resize_adjoint_gather_kernel<%d>" % m for m in range(5)]
PAIRS = [(s, t) for s in rc.SOURCES for t in rc.TARGETS]
# One axis (n_in, n_out), both directions: index times size goes beyond 2^24, where the floor and ceil of a float32 quotient leave
# ATen's integer `area` windows (at 5805 -> 2903 the last float32 window would end at n_in + 1), up to the largest size the entry
# points take
LARGE_AXES = [p for a, b in ((4100, 4099), (4320, 4319), (7680, 4097), (5805, 2903), (8192, 8191), (32768, 30000), (32768, 32767))
              for p in ((a, b), (b, a))]
COMB = 16                    # see comb_matrix: above twice the widest support of LARGE_AXES (four taps; `area` windows of at most 3)


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def test_resize_header_is_exported_and_bound():
    nat.build()
    names = declared("fvvdp_hip_resize.h")
    assert names == ["fvvdp_resize_grad", "fvvdp_temporal_channels_resized"]
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert sorted(nat.RESIZE_SYMBOLS) == names
    lib = nat.lib()
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    assert not hasattr(L, "fvvdp_ctx_ingest_begin")                            # the context's side of the ingest stays internal
    txt = open(os.path.join(ROOT, "include", "fvvdp_hip_resize.h")).read()
    assert int(re.search(r"#define FVVDP_RESIZE_MAX_TAPS (\d+)", txt).group(1)) == nat.RESIZE_MAX_TAPS
    assert ctypes.sizeof(nat.ResizeStream) == 40
    assert nat.resize_grad_table_bytes(60, 34) == 768 and nat.resize_grad_table_bytes(1920, 1080) == 24064
    assert callable(fv.fvvdp.predict_resized) and callable(fv.fvvdp.jod_video_resized)
    # the unit is built without contraction of multiplies and adds
    src = open(os.path.join(ROOT, "fovvideovdp_amd", "_native.py")).read()
    assert re.search(r'"resize_launch\.hip"\), \["-ffp-contract=off"\]', src)


def test_argument_checks_need_no_device():
    lib = nat.lib()
    p = ctypes.c_void_p
    i32p = ctypes.POINTER(ctypes.c_int32)
    e = nat.Eotf()
    w = np.ones(3, np.float32)
    Wo, Ho, N = 120, 68, 5

    def stream(data=256, dtype=nat.FVVDP_F32, C=3, width=60, height=34, fs=None, ps=None):
        hw = width * height
        return nat.ResizeStream(data, dtype, C, width, height, hw if fs is None else fs, N * hw if ps is None else ps)

    # the adjoint
    def adj(gL=256, t=None, g=512, mode=1, kind=nat.EOTF_SRGB, width=Wo, height=Ho, n=N, work=1024, bytes_=1 << 30):
        e.kind = kind
        return lib.fvvdp_resize_grad(width, height, n, p(gL), ctypes.byref(t or stream()), p(g), mode, ctypes.byref(e), nat.fptr(w),
                                     p(work), bytes_, None)

    assert lib.fvvdp_resize_grad(Wo, Ho, N, None, None, None, 1, None, None, None, 0, None) == -1 and b"null" in lib.fvvdp_last_error()
    assert adj(width=0) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert adj(n=0) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert adj(mode=4) == -1 and b"unknown resize mode" in lib.fvvdp_last_error()
    assert adj(mode=-1) == -1 and b"unknown resize mode" in lib.fvvdp_last_error()
    assert adj(kind=nat.EOTF_LUT) == -1 and b"closed-form" in lib.fvvdp_last_error()
    assert adj(kind=nat.EOTF_NONE) == -1 and b"closed-form" in lib.fvvdp_last_error()
    assert adj(t=stream(data=0)) == -1 and b"null data pointer (test)" in lib.fvvdp_last_error()
    assert adj(t=stream(dtype=nat.FVVDP_U8)) == -1 and b"the test must be float32 (" in lib.fvvdp_last_error()
    assert adj(t=stream(dtype=nat.FVVDP_F16)) == -1 and b"the test must be float32 (" in lib.fvvdp_last_error()
    assert adj(t=stream(data=258)) == -1 and b"aligned to 4 bytes (test)" in lib.fvvdp_last_error()
    assert adj(t=stream(C=2)) == -1 and b"1 or 3 colour channels" in lib.fvvdp_last_error()
    assert adj(t=stream(width=0)) == -1 and b"bad frame size" in lib.fvvdp_last_error()
    assert adj(t=stream(ps=60 * 34 - 1)) == -1 and b"plane_stride" in lib.fvvdp_last_error()
    assert adj(t=stream(fs=60 * 34 - 1)) == -1 and b"frame_stride" in lib.fvvdp_last_error()
    assert adj(gL=258) == -1 and b"aligned to 4 bytes" in lib.fvvdp_last_error()
    assert adj(g=514) == -1 and b"aligned to 4 bytes" in lib.fvvdp_last_error()
    assert adj(work=1025) == -1 and b"256-byte aligned" in lib.fvvdp_last_error()
    one = nat.resize_grad_table_bytes(60, 34) + 4 * 3 * Wo * Ho
    assert adj(bytes_=one - 1) == -1 and b"needed for one frame" in lib.fvvdp_last_error()
    # 1 .. 32768 per axis, stream and target alike, in the words of fvvdp_yuv_frame_resized: the index arithmetic runs in 32 bits
    out_of_range = b"frame size out of range (1..32768 per axis)"
    assert adj(t=stream(width=32769, height=1)) == -1 and out_of_range + b": 32769x1 (test)" in lib.fvvdp_last_error()
    assert adj(t=stream(width=1, height=32769)) == -1 and out_of_range + b": 1x32769 (test)" in lib.fvvdp_last_error()
    assert adj(t=stream(width=65536, height=32768)) == -1 and out_of_range in lib.fvvdp_last_error()
    assert adj(width=32769) == -1 and out_of_range + b": 32769x68 (target)" in lib.fvvdp_last_error()
    assert adj(height=1 << 30) == -1 and out_of_range in lib.fvvdp_last_error()
    # the largest sizes pass this check: the call is refused by a later one
    assert adj(t=stream(width=32768, height=2), bytes_=1) == -1 and b"needed for one frame" in lib.fvvdp_last_error()
    assert adj(width=32768, height=32768, bytes_=1) == -1 and b"needed for one frame" in lib.fvvdp_last_error()

    # the ingest: everything that is checked before the context is looked at (a context needs a device)
    taps = np.ones((2, 40), np.float32)
    idx = np.zeros(64, np.int32)

    def ing(ctx=256, t=None, r=None, mode=1, kind=nat.EOTF_SRGB, fl=8):
        e.kind = kind
        return lib.fvvdp_temporal_channels_resized(p(ctx), ctypes.byref(t or stream()), ctypes.byref(r or stream(dtype=nat.FVVDP_U8)), mode,
                                                   ctypes.byref(e), nat.fptr(w), idx.ctypes.data_as(i32p), nat.fptr(taps), fl, 4, 0, None)

    assert ing(ctx=None) == -1 and b"null" in lib.fvvdp_last_error()
    assert ing(mode=7) == -1 and b"unknown resize mode" in lib.fvvdp_last_error()
    assert ing(fl=0) == -1 and b"filter length" in lib.fvvdp_last_error()
    assert ing(fl=33) == nat.FVVDP_EUNSUPPORTED and b"up to 32 taps" in lib.fvvdp_last_error()
    assert ing(kind=nat.EOTF_LUT) == -1 and b"closed-form" in lib.fvvdp_last_error()
    assert ing(kind=nat.EOTF_NONE) == -1 and b"closed-form" in lib.fvvdp_last_error()
    assert ing(t=stream(data=0)) == -1 and b"null data pointer (test)" in lib.fvvdp_last_error()
    assert ing(r=stream(dtype=nat.FVVDP_U16)) == -1 and b"the reference must be float32 or uint8" in lib.fvvdp_last_error()
    assert ing(r=stream(data=258)) == -1 and b"aligned to 4 bytes (reference)" in lib.fvvdp_last_error()
    assert ing(r=stream(C=1)) == -1 and b"differ in their channel counts (3 and 1)" in lib.fvvdp_last_error()
    assert ing(t=stream(height=-3)) == -1 and b"bad frame size" in lib.fvvdp_last_error()
    assert ing(t=stream(width=1, height=32769)) == -1 and out_of_range + b": 1x32769 (test)" in lib.fvvdp_last_error()
    assert ing(r=stream(dtype=nat.FVVDP_U8, width=40000, height=2)) == -1 and out_of_range + b": 40000x2 (reference)" in lib.fvvdp_last_error()
    assert ing(t=stream(width=32768, height=2), r=stream(C=1)) == -1 and b"channel counts" in lib.fvvdp_last_error()


def test_refusals_without_device():
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    t, r = torch.rand(1, 3, 4, 17, 30), torch.rand(1, 3, 4, 34, 60)
    for call, name in ((m.predict_resized, "predict_resized"), (m.jod_video_resized, "jod_video_resized")):
        kw = dict(resize_resolution=(60, 34), frames_per_second=30)
        with pytest.raises(RuntimeError, match="Unknown resize method 'lanczos'"):
            call(t, r, full_screen_resize="lanczos", **kw)
        with pytest.raises(RuntimeError, match="Unknown resize method 'None'"):
            call(t, r, full_screen_resize=None, **kw)
        for bad in (torch.float16, torch.bfloat16, torch.float64, torch.int16):
            with pytest.raises(RuntimeError, match="the test is .*Half-precision, float64 and uint16 samples are not supported"):
                call(t.to(bad), r, **kw)
            with pytest.raises(RuntimeError, match="the reference is .*Half-precision, float64 and uint16 samples are not supported"):
                call(t, r.to(bad), **kw)
        with pytest.raises(RuntimeError, match="the reference is uint16"):
            call(t, (r.numpy() * 65535).astype(np.uint16), **kw)
        with pytest.raises(RuntimeError, match="differ in their frame counts \\(4 and 3\\)"):
            call(t, r[:, :, :3], **kw)
        with pytest.raises(RuntimeError, match="differ in their channel counts \\(3 and 1\\)"):
            call(t, r[:, :1], **kw)
        with pytest.raises(RuntimeError, match="either 1 or 3 colour channels"):
            call(t[:, :2], r[:, :2], **kw)
        with pytest.raises(RuntimeError, match="frame rate too high: its temporal filter has 33 taps"):
            call(t, r, resize_resolution=(60, 34), frames_per_second=130)
        with pytest.raises(RuntimeError, match="frames_per_second"):
            call(t, r, resize_resolution=(60, 34), frames_per_second=0)
        with pytest.raises(RuntimeError, match="at least 2 frames"):
            call(t[:, :, :1], r[:, :, :1], **kw)
        with pytest.raises(RuntimeError, match="at least 2 frames"):                  # single images: no F axis at all
            call(t[0, :, 0], r[0, :, 0], dim_order="CHW", **kw)
        with pytest.raises(RuntimeError, match="one clip per call"):
            call(torch.rand(2, 3, 4, 17, 30), torch.rand(2, 3, 4, 34, 60), **kw)
        with pytest.raises(RuntimeError, match="exactly as many dimensions"):
            call(t, r, dim_order="CFHW", **kw)
        with pytest.raises(RuntimeError, match="bad resize_resolution"):
            call(t, r, resize_resolution=(0, 34), frames_per_second=30)
        # everything accepted: the first device work is refused on a CPU metric (the default target is the display's resolution)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(t, r, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(t, (r * 255).to(torch.uint8), full_screen_resize="area", frames_per_second=120)
        with pytest.raises(RuntimeError, match="no CPU fallback"):                    # both at the target size: predict / jod_video
            call(r, r.clone(), **kw)
    with pytest.raises(RuntimeError, match="gradients with respect to the reference are not supported"):
        m.jod_video_resized(t, r.clone().requires_grad_(True), resize_resolution=(60, 34))
    with pytest.raises(RuntimeError, match="the test is uint8"):                       # a differentiated test is float32
        m.jod_video_resized((t * 255).to(torch.uint8), r, resize_resolution=(60, 34))
    with pytest.raises(RuntimeError, match="forward-only"):
        m.predict_resized(t.clone().requires_grad_(True), r, resize_resolution=(60, 34))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                         # predict_resized takes a uint8 test
        m.predict_resized((t * 255).to(torch.uint8), r, resize_resolution=(60, 34))


def test_refuses_user_photometry():
    class MyDisplay(fv.fvvdp_display_photometry):
        def forward(self, V):
            return 100.0 * V + 0.5

        def get_peak_luminance(self):
            return 100.5

        def get_black_level(self):
            return 0.5

    m = fv.fvvdp(display_name="standard_4k", display_photometry=MyDisplay(), device="cpu", quiet=True)
    for call in (m.predict_resized, m.jod_video_resized):
        with pytest.raises(RuntimeError, match="needs a display model with a closed form"):
            call(torch.rand(3, 4, 17, 30), torch.rand(3, 4, 34, 60), resize_resolution=(60, 34), dim_order="CFHW")


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def _interp(x, size, mode):
    return torch.nn.functional.interpolate(x, size=(size[1], size[0]), mode=mode)


@pytest.mark.parametrize("mode", rref.MODES)
def test_axis_matrices_are_torchs(mode):
    """One axis at a time: torch resizes the identity matrix along its rows only (the other axis keeps its size, so its weights are
    exactly 0 and 1), which lays torch's own index sets and weights out as a matrix.  The index sets must be equal.  The weights are
    float32 on both sides, but torch's CPU build contracts the coordinate scale * (o + 0.5) - 0.5 into one fused multiply-subtract
    where the restatement (and the kernels, built with -ffp-contract=off) round the product first: the coordinate is below n_in, so
    the two differ by up to 2^-24 n_in, and a weight -- whose slope in the coordinate is at most 1.5, in the cubic -- by 1.5 times
    that.  WEIGHT_ULPS = 4 per unit of n_in leaves room for the weight's own roundings."""
    for n_in, n_out in sorted({(s[k], t[k]) for s, t in PAIRS for k in range(2)}):
        want = _interp(torch.eye(n_in)[None, None], (n_in, n_out), mode)[0, 0].numpy()
        A = rref.axis_matrix(n_in, n_out, mode, np.float32)
        S = rref.axis_support(n_in, n_out, mode)
        if mode in ("nearest", "area"):                 # nothing to contract: the same pixels with the same weights, bit for bit
            assert np.array_equal(A, want) and np.array_equal(A != 0, S), (mode, n_in, n_out)
        # torch reads no sample the restatement does not read, and the other way round: a tap that only one side gives a weight
        # other than zero (a coordinate that is an integer on one side and 1e-8 off on the other) has a weight inside the bound
        assert not ((want != 0) & ~S).any() and not ((A != 0) & ~S).any(), (mode, n_in, n_out)
        assert np.abs(A - want).max() <= WEIGHT_ULPS * U24 * n_in, (mode, n_in, n_out)
        if mode != "bicubic":
            assert (A >= 0).all()
        # every mode reproduces a constant (a cubic coefficient has intermediates of up to 8 |A| = 6 and four roundings)
        assert np.abs(A.sum(axis=1) - 1).max() <= (4 * 4 * 6 if mode == "bicubic" else 8) * U24


def comb_matrix(n_in, n_out, mode, along):
    """torch's one-axis matrix [n_out, n_in] of a long axis, folded: torch resizes COMB combs -- comb k has a one at every index that
    is k modulo COMB -- along axis `along` (-2: rows, -1: columns) while the other axis keeps its size.  A target's taps span fewer
    than COMB samples, so entry [o, k] is the weight torch gives the one sample of o's support that is k modulo COMB."""
    comb = (np.arange(n_in)[:, None] % COMB == np.arange(COMB)[None]).astype(np.float32)
    if along == -2:
        return _interp(torch.from_numpy(comb)[None, None], (COMB, n_out), mode)[0, 0].numpy()
    return _interp(torch.from_numpy(comb.T.copy())[None, None], (n_out, COMB), mode)[0, 0].numpy().T


@pytest.mark.parametrize("mode", rref.MODES)
def test_axis_matrices_are_torchs_at_long_axes(mode):
    """test_axis_matrices_are_torchs for LARGE_AXES, from the per-tap index arrays of axis_taps folded as comb_matrix folds torch's
    (a dense 30000 x 32768 matrix is out of reach).  The same assertions: equal supports in every mode; `nearest` and `area` bit for
    bit; the weights of the other two within WEIGHT_ULPS 2^-24 n_in, the bound derived there from the fused multiply-subtract of
    torch's coordinate (not from any kernel).  Measured against torch on the CPU, largest at 5805 -> 2903: bilinear 2.4e-4, bicubic
    3.0e-4 (bound 1.4e-3) -- half a unit in the last place of a coordinate above 4096; at 32768 -> 30000 8.6e-6 (bound 7.8e-3)."""
    worst = {}
    for n_in, n_out in LARGE_AXES:
        taps = rref.axis_taps(n_in, n_out, mode)
        every = np.stack([idx for idx, _ in taps])
        assert int((every.max(axis=0) - every.min(axis=0)).max()) < COMB // 2
        rows = np.arange(n_out)
        A = np.zeros((n_out, COMB), np.float32)
        S = np.zeros((n_out, COMB), bool)
        for idx, w in taps:
            assert idx.min() >= 0 and idx.max() <= n_in - 1
            np.add.at(A, (rows, idx % COMB), w)
            S[rows, idx % COMB] = True
        for along in (-2, -1):
            want = comb_matrix(n_in, n_out, mode, along)
            if mode in ("nearest", "area"):
                assert np.array_equal(A, want) and np.array_equal(A != 0, S), (mode, n_in, n_out, along)
            assert not ((want != 0) & ~S).any() and not ((A != 0) & ~S).any(), (mode, n_in, n_out, along)
            d = float(np.abs(A - want).max())
            worst[(n_in, n_out)] = max(worst.get((n_in, n_out), 0.0), d)
            assert d <= WEIGHT_ULPS * U24 * n_in, (mode, n_in, n_out, along, d)
        if mode != "bicubic":
            assert (A >= 0).all()
        assert np.abs(A.astype(np.float64).sum(axis=1) - 1).max() <= (4 * 4 * 6 if mode == "bicubic" else 8) * U24
    print("\n%s: max |weight - torch's| per pair %s" % (mode, {k: "%.3g" % v for k, v in worst.items()}))


@pytest.mark.parametrize("mode", rref.MODES)
def test_resize_is_torchs_interpolate_at_long_axes(mode):
    """test_resize_is_torchs_interpolate with LARGE_AXES as the height and as the width of skinny images (the other axis 3 -> 5), and
    its bound.  At 32768 -> 30000 the float32 windows of `area` differ from torch by 0.28 on 16 rows of such an image."""
    rng = np.random.default_rng(11)
    for n_in, n_out in LARGE_AXES:
        for source, target in (((3, n_in), (5, n_out)), ((n_in, 3), (n_out, 5))):
            x = rng.uniform(-0.25, 1.25, (3, 1, source[1], source[0])).astype(np.float32)
            want = _interp(torch.from_numpy(x).permute(1, 0, 2, 3), target, mode).permute(1, 0, 2, 3).numpy()
            got = rref.resize(x.astype(np.float64), target, mode)
            scale = rref.resize(np.abs(x).astype(np.float64), target, mode, absolute=True)
            # the largest number of samples a target reads and the sum of |x| over them, per axis as axis_support has them
            T = int(rref.axis_apply(np.ones(source[1]), 0, target[1], mode, support=True).max()) * \
                int(rref.axis_apply(np.ones(source[0]), 0, target[0], mode, support=True).max())
            taps = rref.axis_apply(rref.axis_apply(np.abs(x), -2, target[1], mode, support=True), -1, target[0], mode, support=True)
            assert want.shape == got.shape
            d = np.abs(got - want)
            assert (d <= (T + 4) * U24 * scale + WEIGHT_ULPS * U24 * sum(source) * taps).all(), (mode, source, target, float(d.max()))
            assert (np.abs(rref.resize(x, target, mode, np.float32) - got) <= (T + 4) * U24 * scale).all()


@pytest.mark.parametrize("n_in,n_out", [(5805, 2903), (7680, 4097)])
def test_oracle_area_is_torchs_at_long_axes(n_in, n_out):
    """oracle.torch_interpolate(mode="area"), the yardstick of fvvdp_yuv_frame_resized, against torch itself on skinny frames whose
    long axis takes index times size beyond 2^24, in both orientations.  The same windows, so the two differ by the order of their
    float32 sums alone: within the 8e-6 the g17 tests of the resize give `area` (measured: 0 -- both add a window of at most six samples row by row)."""
    orc = rref.orc
    rng = np.random.default_rng(n_in)
    worst = 0.0
    for h, w, Ho, Wo in ((n_in, 6, n_out, 8), (6, n_in, 8, n_out)):
        x = rng.uniform(-0.25, 1.25, (3, h, w)).astype(np.float32)
        want = torch.nn.functional.interpolate(torch.from_numpy(x)[None], size=(Ho, Wo), mode="area")[0].numpy()
        got = orc.torch_interpolate(x, Ho, Wo, "area")
        assert got.shape == want.shape and got.dtype == np.float32
        worst = max(worst, float(np.abs(got - want).max()))
    print("\noracle area %d -> %d: max |oracle - torch| %.3g" % (n_in, n_out, worst))
    assert worst <= 8e-6


@pytest.mark.parametrize("mode", rref.MODES)
def test_resize_is_torchs_interpolate(mode):
    """Both axes, float32 torch against the float64 sums of the restatement.  torch adds the T = ty * tx products of a target sample
    in float32: (T + 4) 2^-24 sum |w| |x| bounds its rounding (T - 1 additions, one rounding per product, and for `area` the final
    division; the restatement's weights 1 / ny and 1 / nx are two more).  On top comes the difference of the weights themselves
    (test_axis_matrices_are_torchs): WEIGHT_ULPS 2^-24 (h + w) per tap, times the sum of |x| over the taps."""
    rng = np.random.default_rng(7)
    for source, target in PAIRS:
        x = rng.uniform(-0.25, 1.25, (3, 2, source[1], source[0])).astype(np.float32)
        want = _interp(torch.from_numpy(x).permute(1, 0, 2, 3), target, mode).permute(1, 0, 2, 3).numpy()
        got = rref.resize(x.astype(np.float64), target, mode)
        scale = rref.resize(np.abs(x).astype(np.float64), target, mode, absolute=True)
        T = int((rref.axis_matrix(source[1], target[1], mode) != 0).sum(axis=1).max()) * \
            int((rref.axis_matrix(source[0], target[0], mode) != 0).sum(axis=1).max())
        Sy, Sx = (rref.axis_support(source[k], target[k], mode).astype(np.float64) for k in (1, 0))
        taps = np.matmul(np.matmul(Sy, np.abs(x).astype(np.float64)), Sx.T)
        assert want.shape == got.shape
        assert (np.abs(got - want) <= (T + 4) * U24 * scale + WEIGHT_ULPS * U24 * sum(source) * taps).all(), (mode, source, target)
        # float32 sums of the restatement stay within the same bound of its float64 sums
        assert (np.abs(rref.resize(x, target, mode, np.float32) - got) <= (T + 4) * U24 * scale).all()


@pytest.mark.parametrize("mode", rref.MODES)
def test_adjoint_satisfies_the_inner_product_identity(mode):
    """<A x, y> = <x, A^T y> with the whole restated adjoint: a linear display model inside its clip has derivative 1, samples in
    [0.3, 0.7] stay clear of every clip, and weights of one leave A^T y."""
    for source, target in PAIRS:
        rng = np.random.default_rng(source[0] * target[0])
        x = rng.uniform(0.3, 0.7, (3, source[1], source[0]))
        y = rng.standard_normal((target[1], target[0]))
        lhs = float((rref.resize(x, target, mode) * y[None]).sum())
        adj = rref.resize_adjoint(y, x, target, mode, np.ones(3), rref.eotf_args(rref.yref.orc.Photometry(1000, EOTF="linear"))[0],
                                  Y_peak=1000.0)
        rhs = float((x * adj).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (mode, source, target)


@pytest.mark.parametrize("mode", rref.MODES)
def test_adjoint_is_torchs_autograd(mode):
    """interpolate(x).clip(0, 1) under torch autograd in float32 against the float64 adjoint.  A source sample sums T terms, T the
    number of target samples that reach it: (T + 4) 2^-24 sum |w| |G| plus the difference of the weights, as above.  Exact zeros where nothing arrives (every target
    sample that reaches the source sample clipped, or none reaching it at all), on both sides."""
    zeros = 0
    for source, target in PAIRS:
        c = dict(C=3, source=source, target=target, mode=mode)
        x, _ = rc.draw_clip([3, *source, *target], 3, 2, source, target, mode)
        rng = np.random.default_rng(source[1] * target[0])
        G = (rng.uniform(0.25, 2.0, (3, 2, target[1], target[0])) * rng.choice([-1.0, 1.0], (3, 2, target[1], target[0]))).astype(np.float32)
        xt = torch.from_numpy(x.copy()).requires_grad_(True)
        (_interp(xt.permute(1, 0, 2, 3), target, mode).clip(0, 1).permute(1, 0, 2, 3) * torch.from_numpy(G)).sum().backward()
        want = xt.grad.numpy()
        Ty = int((rref.axis_matrix(source[1], target[1], mode) != 0).sum(axis=0).max())
        Tx = int((rref.axis_matrix(source[0], target[0], mode) != 0).sum(axis=0).max())
        Sy, Sx = (rref.axis_support(source[k], target[k], mode).astype(np.float64) for k in (1, 0))
        for f in range(2):
            got = rref.clip_adjoint(G[:, f], x[:, f], target, mode)
            scale = rref.clip_adjoint(G[:, f], x[:, f], target, mode, absolute=True)
            v = rref.resize(x[:, f].astype(np.float64), target, mode)
            taps = np.matmul(np.matmul(Sy.T, np.abs(G[:, f]) * ((v >= 0) & (v <= 1))), Sx)
            assert (np.abs(got - want[:, f]) <= (Ty * Tx + 4) * U24 * scale + WEIGHT_ULPS * U24 * sum(source) * taps).all(), c
            assert (want[:, f][scale == 0] == 0).all() and (got[scale == 0] == 0).all()
            zeros += int((scale == 0).sum())
    assert zeros > 0


def test_case_inputs_keep_their_margin():
    """No float64 pre-clip value of a case lies where float32 and float64 could clip differently, the clip does bind, and bicubic
    cases overshoot on both sides."""
    for c in rc.rotation():
        test, ref = rc.rotation_inputs(c)
        again, _ = rc.rotation_inputs(c)
        assert test.dtype == np.float32 and str(ref.dtype) == c["ref_dtype"] and again is test
        assert test.shape[2:] == c["source"][::-1] and ref.shape[2:] == (c["ref_source"] or c["target"])[::-1]
        for x, src in ((test, c["source"]), (ref, c["ref_source"])):
            if src is None:
                continue
            assert not rref.margin(x, c["target"], c["mode"]).any(), rc.case_id(c)
        v = rref.resize(test.astype(np.float64), c["target"], c["mode"])
        print("%s: %d of %d target values below 0, %d above 1" % (rc.case_id(c), int((v < 0).sum()), v.size, int((v > 1).sum())))
        if c["source"] != (7, 5) or c["mode"] == "bicubic":           # (factor 17: see the module text of resize_cases.py)
            assert (v < -1e-2).any() and (v > 1 + 1e-2).any(), rc.case_id(c)
    for name in rc.CASES:
        N, C, source, target, mode = rc.CASES[name][:5]
        test, ref = rc.case_inputs(name)
        assert test.shape == (C, N, source[1], source[0]) and ref.shape == (C, N, target[1], target[0])
        assert not rref.margin(test, target, mode).any()
        v = rref.resize(test.astype(np.float64), target, mode)
        assert (v < 0).any() and (v > 1).any(), name


def test_rotation_covers_the_matrix():
    R = rc.rotation()
    assert {(c["mode"], c["fps"]) for c in R} == {(m, f) for m in rref.MODES for f in rc.FPS}
    assert {c["C"] for c in R} == {1, 3} and {c["source"] for c in R} == set(rc.SOURCES) and {c["target"] for c in R} == set(rc.TARGETS)
    assert {c["ref_dtype"] for c in R} == {"float32", "uint8"} and {c["display"] for c in R} == set(rc.DISPLAYS)
    assert {c["padding"] for c in R} == set(rc.PADDINGS)
    assert any(c["ref_source"] is None for c in R) and any(c["ref_source"] not in (None, c["source"]) for c in R)


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_goldens_load(name):
    N, C, source, target = rc.CASES[name][:4]
    path = os.path.join(rc.GOLDEN, rc.FILES[name])
    largest_g24 = max(os.path.getsize(os.path.join(rc.GOLDEN, f)) for f in os.listdir(rc.GOLDEN) if f.startswith("g24_"))
    assert os.path.getsize(path) <= largest_g24
    jod, g = rc.load_golden(name)
    assert g.shape == (C, N, source[1], source[0]) and np.isfinite(g).all() and 0 < jod < 10 and g.any()
    assert set(np.load(path).files) == {name + "_jod", name + "_grad"}              # outputs only


def test_new_kernels_do_not_spill():
    import codeobj
    nat.build()
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    names = list(md)
    nice = codeobj.demangle(names)
    found = {k: 0 for k in NEW_KERNELS}
    for mname, n in zip(names, nice):
        base = n.split("(")[0]
        if base in found:
            found[base] += 1
            x = md[mname]
            # no scratch memory: nothing private, no vector register spilled.  The ring kernels of `area` -- a divergent loop over the
            # window inside the unrolled frame loop -- may park scalar registers in the lanes of a vector register (the 16-slot one
            # does, two of them), which costs no memory access; every other kernel keeps its scalars where they are
            assert (x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0), n
            if not (base.startswith("void resized_ring_kernel<") and base.endswith(", 3>")):
                assert x["sgpr_spill_count"] == 0, n
    assert found == {k: 1 for k in found}
    # none of the names the other tests count by substring
    for n in NEW_KERNELS:
        assert not any(s in n for s in ("temporal_vec_kernel<", "band2_kernel<", "band_kernel<", "temporal_ring_kernel<",
                                        "temporal_yuv_kernel<", "temporal_yuv_vec_kernel<", "video_input_kernel<",
                                        "yuvplanes_ring_kernel<", "video_lum_input_kernel<"))
