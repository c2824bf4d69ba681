"""fvvdp_video_grad_input alone, through the C ABI, against the float64 reference of tests/video_grad_input_ref.py: every
output sample of every (ring size FL, pixels per lane PX) instantiation of video_input_kernel, at filter lengths on both sides
of each ring size, clip lengths on both sides of the filter length, all three paddings, frame sizes that exercise the tail of
each variant, and strided / offset layouts whose gaps must survive.  Then the display model's derivative in isolation."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd.fvvdp import filter_length, window_frame_indices
from fovvideovdp_amd.video_grad import _fold_arrays, fold_list

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_grad_input_ref as vref          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24                              # unit roundoff of fp32
SENTINEL = 0x7FC12345                       # a quiet NaN with a payload: what the gaps and guards hold
GUARD = 64                                  # floats of sentinel behind every buffer the kernel writes
RGB2Y = np.array([0.2126, 0.7152, 0.0722], np.float32)
_metric = []


def metric():
    if not _metric:
        _metric.append(fv.fvvdp(display_name="standard_4k", quiet=True, device=DEV))
    return _metric[0]


def eotf_struct(kind, Y_peak=0.0, Y_black=0.0, gamma=2.2, L_min=0.0, L_max=0.0):
    return nat.Eotf(kind, Y_peak, Y_black, gamma, L_min, L_max, None)


def expected_variant(fl, HW, C_ch, chan_stride, frame_stride, offset):
    """(FL, PX) by the rule of include/fvvdp_hip_video_grad.h: the ring is fl rounded up to 8 / 16 / 32 / 64 slots; 4 pixels
    per lane up to 16 taps and 2 above when the frame size and the strides are multiples of that and the pointers aligned to
    it, 1 otherwise.  (The buffers of this file come from the caching allocator, aligned far beyond 16 bytes.)"""
    FL = 8 if fl <= 8 else 16 if fl <= 16 else 32 if fl <= 32 else 64
    pxv = 4 if FL <= 16 else 2
    vec = HW % pxv == 0 and frame_stride % pxv == 0 and (C_ch == 1 or chan_stride % pxv == 0) and offset % pxv == 0
    return FL, pxv if vec else 1


def layout_strides(layout, C_ch, N, HW):
    """(chan_stride, frame_stride, offset of the base pointer in floats)."""
    if layout == "fchw":
        return HW, C_ch * HW, 0
    gap = {"cfhw": 0, "off1": 0, "gap1": 1, "gap4": 4}[layout]
    return N * (HW + gap), HW + gap, 1 if layout == "off1" else 0


def run_input(W, H, N, fl, padding, taps, g0, test, eotf, layout):
    """The entry point on g0 [N, 2, HW] and test [C, N, HW] (numpy fp32) laid out as `layout` -> grad [C, N, HW] (numpy fp32).
    Everything between and behind the samples of d_grad and behind d_head holds a sentinel that must survive bit for bit."""
    HW, C_ch = W * H, test.shape[0]
    cs, fs, off = layout_strides(layout, C_ch, N, HW)
    span = off + (C_ch - 1) * cs + (N - 1) * fs + HW
    hb = np.empty(span + GUARD, np.float32)
    hb.view(np.uint32)[:] = SENTINEL
    payload = np.zeros(span + GUARD, bool)
    for c in range(C_ch):
        for f in range(N):
            o = off + c * cs + f * fs
            hb[o:o + HW] = test[c, f]
            payload[o:o + HW] = True
    tbuf = torch.from_numpy(hb).to(DEV)
    gbuf = torch.full((span + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    head = torch.full((fl * HW + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    g0d = torch.from_numpy(np.ascontiguousarray(g0, dtype=np.float32)).to(DEV)
    idx = window_frame_indices(N, fl, padding)
    ff, fp = _fold_arrays(fold_list(idx, fl, N))
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    assert taps.shape == (2, fl) and g0d.shape == (N, 2, HW)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    i32p = C.POINTER(C.c_int32)
    nat.check(nat.lib().fvvdp_video_grad_input(
        W, H, N, C.c_void_p(g0d.data_ptr()), ff.ctypes.data_as(i32p), fp.ctypes.data_as(i32p), nat.fptr(taps), fl,
        C.c_void_p(tbuf.data_ptr() + 4 * off), C.c_void_p(gbuf.data_ptr() + 4 * off), C_ch, cs, fs, C.byref(eotf), nat.fptr(RGB2Y),
        C.c_void_p(head.data_ptr()), fl * HW * 4, stream))
    out = gbuf.cpu().numpy()
    assert (out[~payload] == SENTINEL).all(), "the kernel wrote outside the samples of d_grad (%s)" % layout
    assert (head[fl * HW:].cpu().numpy() == SENTINEL).all(), "the kernel wrote behind the side buffer"
    got = np.empty((C_ch, N, HW), np.float32)
    outf = out.view(np.float32)
    for c in range(C_ch):
        for f in range(N):
            o = off + c * cs + f * fs
            got[c, f] = outf[o:o + HW]
    return got, idx


# ---- structure: the transpose, with a display derivative of exactly 1 (or 0 outside the range) ------------------------------
FILTER_LENGTHS = (1, 6, 8, 9, 15, 16, 17, 30, 32, 33, 36, 60, 64)
LONG_N = 41                                 # "a few dozen" frames for the short filters


def frame_counts(fl):
    if fl <= 6:                             # N >= 2 (window_frame_indices' circular head is empty for N = 1)
        return [fl + 1, 2 * fl + 3, LONG_N]
    return [2, fl - 1, fl, fl + 1, 2 * fl + 3] + ([LONG_N] if fl <= 9 else [])


def shapes(FL):
    """(W, H) per kind; pxv is the vector width of this ring size."""
    pxv = 4 if FL <= 16 else 2
    return [("odd", 5, 3),                      # H*W odd and below one workgroup: PX 1 everywhere
            ("mod2", 2, 129),                   # H*W % 4 == 2: PX 1 up to 16 taps, PX 2 above
            ("mod0", 4, 5),                     # H*W % 4 == 0, a fraction of a workgroup
            ("full", 16, 16 * pxv),             # H*W == 256 PX: the vector variant's one workgroup exactly full
            ("full+", 257, pxv),                # 256 PX + PX: one lane in the second workgroup
            ("sfull+", 257, 1),                 # 256 + 1, odd: the same for the scalar variant
            ("ragged0", 121, 68),               # several workgroups and a ragged last one, H*W % 4 == 0
            ("ragged1", 121, 67),               # ... H*W odd
            ("ragged2", 122, 69)]               # ... H*W % 4 == 2


LAYOUTS = ("cfhw", "gap1", "fchw", "gap4", "off1", "cfhw", "gap4")


def structure_cases():
    """One case per (filter length, frame count, padding); frame size, channels, layout and taps rotate so that every choice
    meets every padding and ring size somewhere (test_cases_reach_every_instantiation checks the variants)."""
    out, j = [], 0
    for fl in FILTER_LENGTHS:
        FL = expected_variant(fl, 4, 1, 0, 4, 0)[0]
        for N in frame_counts(fl):
            for p, padding in enumerate(("replicate", "circular", "pingpong")):
                kind, W, H = shapes(FL)[(j + 4 * p) % 9]
                layout = LAYOUTS[(j + 3 * p) % 7]
                C_ch = 3 if layout == "fchw" or (j + p) % 3 == 0 else 1
                tk = "rand" if ((j + p) % 2 == 0 or fl == 1) else "real"      # the metric's filters need two taps: fl = 1 is random only
                cs, fs, off = layout_strides(layout, C_ch, N, W * H)
                FLx, PX = expected_variant(fl, W * H, C_ch, cs, fs, off)
                cid = "fl%d-N%d-%s-%s-%s%dx%d-C%d-%s-FL%dxPX%d" % (fl, N, padding, tk, kind, W, H, C_ch, layout, FLx, PX)
                out.append(pytest.param(fl, N, padding, tk, W, H, C_ch, layout, 3 * j + p, (FLx, PX), id=cid))
            j += 1
    return out


STRUCTURE = structure_cases()
INSTANTIATIONS = {(8, 4), (8, 1), (16, 4), (16, 1), (32, 2), (32, 1), (64, 2), (64, 1)}


def test_cases_reach_every_instantiation():
    """Every (FL, PX) the library instantiates (tests/test_video_grad_cpu.py lists them from the code object) is selected by
    several structure cases, each with every padding."""
    seen = {}
    for p in STRUCTURE:
        seen.setdefault(p.values[-1], set()).add(p.values[2])
    assert set(seen) == INSTANTIATIONS
    assert all(len(v) == 3 for v in seen.values()), seen


def real_taps(fl):
    fps = 4 * fl - 2
    assert filter_length(fps) == fl
    n, taps = metric()._temporal_taps(fps)
    assert n == fl and taps.shape == (2, fl)
    return taps


def structure_inputs(fl, N, tk, HW, C_ch, seed):
    rng = np.random.default_rng(7000 + seed)
    # random taps of mixed sign: the metric's decay, and a wrong slot at the far end of the ring would hide under the bound
    taps = rng.standard_normal((2, fl)).astype(np.float32) if tk == "rand" else real_taps(fl)
    g0 = rng.standard_normal((N, 2, HW)).astype(np.float32)
    test = rng.uniform(1.0, 70.0, (C_ch, N, HW)).astype(np.float32)
    out = rng.random(test.shape) < 0.1                     # a tenth of the samples outside the display's range: exact zeros
    test[out] = np.where(rng.random(int(out.sum())) < 0.5, np.float32(1e-3), np.float32(500.0))
    test[0, N - 1, HW // 2] = np.float32(500.0)             # at least one, whatever the size
    if seed % 2:
        return taps, g0, test, nat.EOTF_LINEAR, dict(Y_peak=100.0, Y_black=0.1)
    return taps, g0, test, nat.EOTF_ABSOLUTE, dict(L_min=0.5, L_max=80.0)


@pytest.mark.parametrize("fl,N,padding,tk,W,H,C_ch,layout,seed,variant", STRUCTURE)
def test_transpose_per_sample(fl, N, padding, tk, W, H, C_ch, layout, seed, variant):
    """Each output is one chain of at most 3 fl + 4 fp32 additions (2 fl fused multiply-adds per list position, up to fl head
    positions and the streaming term per frame) of terms tap * g0, then two multiplications, so
        |got - ref| <= (3 fl + 6) 2^-24 w_c S,     S = the same sum over |tap * g0| in float64
    (first order; at fl = 64 the second-order term is 1e-5 of it, and 3 fl + 6 leaves two roundings spare).  DERIVED, not
    measured (on MI355X the worst case of this file reaches 0.27 of it).  Where the reference is an exact zero (S = 0: a sample outside the display's range, or a frame no window shows)
    the bound is zero as well."""
    HW = W * H
    taps, g0, test, kind, prm = structure_inputs(fl, N, tk, HW, C_ch, seed)
    got, idx = run_input(W, H, N, fl, padding, taps, g0, test, eotf_struct(kind, **prm), layout)
    wts = RGB2Y if C_ch == 3 else np.ones(1, np.float32)
    ref, S = vref.grad_input(idx, taps, g0, test, wts, kind, **prm)
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    bound = (3 * fl + 6) * U * S
    zero = S == 0
    print("worst |got - ref| / bound %.3f; exact zeros %d of %d" % (float((err[~zero] / bound[~zero]).max()), int(zero.sum()), zero.size))
    assert (got[zero] == 0).all()
    bad = np.argwhere(err > bound)
    assert bad.size == 0, "(channel, frame, pixel) of the first misses: %s" % bad[:8].tolist()
    assert zero.any() and not zero.all()
    if padding == "circular" and N > fl + 1:            # no window shows frame 0
        assert zero[:, 0].all() and (got[:, 0] == 0).all()
    if padding == "pingpong" and 2 < N < fl:            # the head folds many positions onto one frame
        assert max(len(p) for p in fold_list(idx, fl, N)) >= 2
    # the scalar variant of the same ring adds the same terms in the same order: bit-identical
    if variant[1] > 1:
        assert layout != "off1"
        got1, _ = run_input(W, H, N, fl, padding, taps, g0, test, eotf_struct(kind, **prm), "off1" if layout == "cfhw" else "gap1")
        assert np.array_equal(got1.view(np.uint32), got.view(np.uint32))


# ---- the display model's derivative: fl = 1, taps [[1], [0]], replicate: dLum[j] = g0[j][0] exactly --------------------------
# worst |got - ref| / |ref| against the float64 closed form, over C = 1 and C = 3: 3x the value MEASURED on MI355X
# (sRGB 4.2e-7, gamma 2.2 2.5e-7, gamma 1.8 2.3e-7, PQ at a peak of 1500 cd/m^2 2.2e-5, PQ at 400 cd/m^2 1.8e-5; powf is in
# the chain, so no bound follows from the project's own code)
DERIV_TOL = {"srgb": 1.3e-6, "gamma2.2": 7.5e-7, "gamma1.8": 6.8e-7, "pq1500": 6.5e-5, "pq400": 5.4e-5}
# A PQ sample is left out when its float64 luminance lies within this relative distance of a clamp (0.005 cd/m^2, the peak):
# there fp32 and fp64 may fall on different sides.  fp32 carries L to about 1e-5: r = (t - c1) / den loses up to t / (t - c1)
# = 8x at 0.005 cd/m^2, the power 1 / n multiplies by 6.3, on a few ulp of powf (6e-8 each); the margin is ten times that.
PQ_MARGIN = 1e-4
MAX_EXCLUDED = 0.01
# The linear branch of sRGB (V = 0 and the knee V = 0.04045 themselves): Y_peak - Y_black, 1 / 12.92, w_c and three products,
# six roundings.  DERIVED.
LINEAR_BRANCH_TOL = 6 * U
# a result below the smallest normal fp32 may lose bits or be flushed (gamma next to V = 0)
FP32_TINY = 2.0 ** -126


def around(x):
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]


def unit_range_samples(extra):
    v = [np.linspace(0.0, 1.0, 4001, dtype=np.float64).astype(np.float32), around(0.0), around(1.0), [np.float32(-0.0)],
         np.float32([-1e-30, -1e-3, -0.5, -3.0, 1.001, 1.5, 7.0, 1e30]), np.asarray(extra, np.float32)]
    return np.concatenate([np.asarray(a, np.float32).ravel() for a in v])


def pq_samples(peak):
    d = np.array([-1e-1, -1e-2, -1e-3, -3e-4, 3e-4, 1e-3, 1e-2, 1e-1])
    near = np.concatenate([vref.pq_inverse(0.005 * (1 + d)), vref.pq_inverse(peak * (1 + d))])
    return unit_range_samples(near)


DERIV_CASES = {
    "srgb": (nat.EOTF_SRGB, dict(Y_peak=200.0, Y_black=0.2), lambda: unit_range_samples(around(0.04045))),
    "gamma2.2": (nat.EOTF_GAMMA, dict(Y_peak=300.0, Y_black=0.375, gamma=2.2), lambda: unit_range_samples([])),
    "gamma1.8": (nat.EOTF_GAMMA, dict(Y_peak=300.0, Y_black=0.375, gamma=1.8), lambda: unit_range_samples([])),
    "pq1500": (nat.EOTF_PQ, dict(Y_peak=1500.0, Y_black=0.0175), lambda: pq_samples(1500.0)),      # standard_hdr_pq
    "pq400": (nat.EOTF_PQ, dict(Y_peak=400.0, Y_black=0.0175), lambda: pq_samples(400.0)),
    "linear": (nat.EOTF_LINEAR, dict(Y_peak=1500.0, Y_black=0.0175), lambda: np.concatenate([
        np.linspace(0.0, 1600.0, 4001).astype(np.float32), around(0.005), around(1500.0), np.float32([-2.0, -0.0, 1e-3, 1e4])])),
    "absolute": (nat.EOTF_ABSOLUTE, dict(L_min=0.005, L_max=10000.0), lambda: np.concatenate([
        np.linspace(0.0, 10100.0, 4001).astype(np.float32), around(0.005), around(10000.0), np.float32([-2.0, -0.0, 1e-3, 2e4])])),
}


@pytest.mark.parametrize("C_ch", [1, 3])
@pytest.mark.parametrize("name", sorted(DERIV_CASES))
def test_display_derivative(name, C_ch):
    kind, prm, make = DERIV_CASES[name]
    V = make()
    V = np.concatenate([V, np.full((-len(V)) % 2, 0.5, np.float32)])        # two frames
    HW = len(V) // 2
    rng = np.random.default_rng(len(name) + C_ch)
    test = np.stack([np.roll(V, 17 * c) for c in range(C_ch)]).reshape(C_ch, 2, HW)
    g0 = (rng.uniform(0.5, 2.0, (2, 2, HW)) * rng.choice([-1.0, 1.0], (2, 2, HW))).astype(np.float32)
    taps = np.array([[1.0], [0.0]], np.float32)
    got, idx = run_input(HW, 1, 2, 1, "replicate", taps, g0, test, eotf_struct(kind, **prm), "cfhw")
    wts = RGB2Y if C_ch == 3 else np.ones(1, np.float32)
    ref, S = vref.grad_input(idx, taps, g0, test, wts, kind, **prm)
    assert np.array_equal(vref.dlum(idx, taps, g0), g0[:, 0].astype(np.float64))       # the transpose is the identity here
    got64 = got.astype(np.float64)
    assert np.isfinite(got).all()
    excluded = np.zeros(test.shape, bool)
    if kind == nat.EOTF_PQ:
        L = vref.pq_luminance(test)
        excluded = (np.abs(L / 0.005 - 1) < PQ_MARGIN) | (np.abs(L / prm["Y_peak"] - 1) < PQ_MARGIN)
    share = float(excluded.mean())
    zero = (ref == 0) & ~excluded
    live = (ref != 0) & ~excluded
    assert share <= MAX_EXCLUDED and zero.sum() >= 10 and live.sum() >= 1000
    # where the model clamps: exact zeros
    assert (got[zero] == 0).all(), "nonzero gradient at clamped samples %s" % np.unique(test[zero & (got != 0)])[:8]
    err = np.abs(got64 - ref)
    if name in ("linear", "absolute"):          # the derivative is exactly 1: the result is w_c g0 rounded once
        w32 = wts.reshape(-1, 1, 1) * g0[None, :, 0]
        assert np.array_equal(got[live], np.broadcast_to(w32, got.shape)[live])
        return
    rel = err[live] / np.abs(ref[live])
    floor = FP32_TINY * np.abs(wts.astype(np.float64).reshape(-1, 1, 1) * g0[None, :, 0])
    worst = float((np.maximum(err - floor, 0.0)[live] / np.abs(ref[live])).max())
    at = np.unravel_index(np.argmax(np.where(live, err / np.maximum(np.abs(ref), 1e-300), 0)), err.shape)
    print("%s C=%d: worst |got - ref| / |ref| = %.3e (plain %.3e, at V = %r); excluded %.4f; %d exact zeros" % (
        name, C_ch, worst, float(rel.max()), float(test[at]), share, int(zero.sum())))
    assert worst <= DERIV_TOL[name]
    if kind == nat.EOTF_SRGB:                   # the samples on the linear branch, V = 0 and the knee itself among them
        lin = live & (test <= np.float32(0.04045))
        assert (test[lin] == 0).any() and (test[lin] == np.float32(0.04045)).any()
        assert (err[lin] <= LINEAR_BRANCH_TOL * np.abs(ref[lin])).all()
        assert live[test == 1].all()            # V = 1 is inside the range
    else:                                       # gamma and PQ: V = 0 itself is an exact zero (checked above as part of `zero`)
        assert zero[test == 0].all()
