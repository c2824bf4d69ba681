"""fvvdp_video_grad_input_held alone, through the C ABI, against the float64 reference of tests/held_ref.py: every output sample of
every (ring size FL, pixels per lane PX) instantiation of video_input_held_kernel, at filter lengths on both sides of each ring
size, display counts on both sides of the filter length, all three paddings, frame maps that hold, skip, start above zero and stay
constant, frame sizes that exercise the tail of each variant, and strided / offset layouts whose gaps must survive.  Then the
identity map against fvvdp_video_grad_input_st, bit for bit, for float32, float16 and bfloat16."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from fovvideovdp_amd import _native as nat
from fovvideovdp_amd.fvvdp import window_frame_indices
from fovvideovdp_amd.grad_passes import _fold_arrays, fold_list, held_fold_arrays

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import held_cases as hc                      # noqa: E402
import held_ref as href                      # noqa: E402
from test_gpu_video_grad_input import (DEV, GUARD, LAYOUTS, RGB2Y, SENTINEL, U, eotf_struct, expected_variant, layout_strides,      # noqa: E402
                                       real_taps, shapes)

pytestmark = pytest.mark.gpu
TORCH_DTYPE = {nat.FVVDP_F32: torch.float32, nat.FVVDP_F16: torch.float16, nat.FVVDP_BF16: torch.bfloat16}


def _lay_out(x, layout, dtype):
    """x [C, F, HW] (a torch tensor of the sample type, on the host) -> (device buffer, payload mask, strides, offset)."""
    C_ch, F, HW = x.shape
    cs, fs, off = layout_strides(layout, C_ch, F, HW)
    span = off + (C_ch - 1) * cs + (F - 1) * fs + HW
    sent = torch.tensor([SENTINEL], dtype=torch.int32).view(torch.float32).to(TORCH_DTYPE[dtype])      # a NaN in every sample type
    hb = sent.repeat(span + GUARD)
    payload = np.zeros(span + GUARD, bool)
    for c in range(C_ch):
        for f in range(F):
            o = off + c * cs + f * fs
            hb[o:o + HW] = x[c, f]
            payload[o:o + HW] = True
    return hb.to(DEV), payload, (cs, fs, off)


def run_held(W, H, N, m, F, fl, padding, taps, g0, src, eotf, layout, dtype=nat.FVVDP_F32, entry="held"):
    """The entry point on g0 [N, 2, HW] and src [C, F, HW] (numpy fp32; converted to `dtype`) laid out as `layout` -> grad [C, F, HW]
    as a torch tensor of the sample type.  Everything between and behind the samples of d_grad and behind the side buffer holds a
    sentinel that must survive.  entry="st": fvvdp_video_grad_input_st on the same buffers (the identity map only)."""
    HW, C_ch = W * H, src.shape[0]
    es = 4 if dtype == nat.FVVDP_F32 else 2
    x = torch.from_numpy(np.ascontiguousarray(src)).to(TORCH_DTYPE[dtype])
    tbuf, payload, (cs, fs, off) = _lay_out(x, layout, dtype)
    gbuf = torch.full_like(tbuf, float("nan"))
    mb = nat.held_map_bytes(N) // 4 if entry == "held" else 0
    head = torch.full((mb + fl * HW + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    g0d = torch.from_numpy(np.ascontiguousarray(g0, dtype=np.float32)).to(DEV)
    widx = window_frame_indices(N, fl, padding)
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    assert taps.shape == (2, fl) and g0d.shape == (N, 2, HW) and src.shape[1] == F
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    i32p = C.POINTER(C.c_int32)
    lib = nat.lib()
    if entry == "held":
        ff, fp = held_fold_arrays(m, widx, fl)
        m = np.ascontiguousarray(m, dtype=np.int32)
        nat.check(lib.fvvdp_video_grad_input_held(
            W, H, N, F, C.c_void_p(g0d.data_ptr()), m.ctypes.data_as(i32p), ff.ctypes.data_as(i32p), fp.ctypes.data_as(i32p),
            nat.fptr(taps), fl, C.c_void_p(tbuf.data_ptr() + es * off), C.c_void_p(gbuf.data_ptr() + es * off), dtype, C_ch, cs, fs,
            C.byref(eotf), nat.fptr(RGB2Y), C.c_void_p(head.data_ptr()), (mb + fl * HW) * 4, stream))
    else:
        assert F == N and np.array_equal(m, np.arange(N))
        ff, fp = _fold_arrays(fold_list(widx, fl, N))
        nat.check(lib.fvvdp_video_grad_input_st(
            W, H, N, C.c_void_p(g0d.data_ptr()), ff.ctypes.data_as(i32p), fp.ctypes.data_as(i32p), nat.fptr(taps), fl,
            C.c_void_p(tbuf.data_ptr() + es * off), C.c_void_p(gbuf.data_ptr() + es * off), dtype, C_ch, cs, fs, C.byref(eotf),
            nat.fptr(RGB2Y), C.c_void_p(head.data_ptr()), fl * HW * 4, stream))
    out = gbuf.cpu()
    assert torch.isnan(out[torch.from_numpy(~payload)]).all(), "the kernel wrote outside the samples of d_grad (%s)" % layout
    assert (head[mb + fl * HW:].cpu().numpy() == SENTINEL).all(), "the kernel wrote behind the side buffer"
    if entry == "held":
        assert np.array_equal(head[:N].cpu().numpy(), m) and (head[N:mb].cpu().numpy() == SENTINEL).all()
    got = torch.empty((C_ch, F, HW), dtype=TORCH_DTYPE[dtype])
    for c in range(C_ch):
        for f in range(F):
            o = off + c * cs + f * fs
            got[c, f] = out[o:o + HW]
    return got, widx


def bits(t):
    return t.view(torch.int32 if t.dtype is torch.float32 else torch.int16).numpy()


FILTER_LENGTHS = (1, 6, 8, 9, 15, 16, 17, 30, 32)


def display_counts(fl):
    return sorted({n for n in (2, fl - 1, fl, fl + 1, 2 * fl + 3) if n >= 2})


def structure_cases():
    """One case per (filter length, display count, padding); the map, frame size, channels, layout and taps rotate so that every
    choice meets every padding and ring size somewhere."""
    out, j = [], 0
    for fl in FILTER_LENGTHS:
        FL = 8 if fl <= 8 else 16 if fl <= 16 else 32
        for N in display_counts(fl):
            for p, padding in enumerate(hc.PADDINGS):
                kind, W, H = shapes(FL)[(j + 4 * p) % 9]
                layout = LAYOUTS[(j + 3 * p) % 7]
                mk = hc.MAP_KINDS[(j + 2 * p) % 7]
                C_ch = 3 if layout == "fchw" or (j + p) % 3 == 0 else 1
                tk = "rand" if ((j + p) % 2 == 0 or fl == 1) else "real"
                m, F = hc.c_abi_map(mk, N)
                cs, fs, off = layout_strides(layout, C_ch, F, W * H)
                FLx, PX = expected_variant(fl, W * H, C_ch, cs, fs, off)
                cid = "fl%d-N%d-%s-%s-%s-%s%dx%d-C%d-%s-FL%dxPX%d" % (fl, N, padding, mk, tk, kind, W, H, C_ch, layout, FLx, PX)
                out.append(pytest.param(fl, N, padding, mk, tk, W, H, C_ch, layout, 3 * j + p, (FLx, PX), id=cid))
            j += 1
    return out


STRUCTURE = structure_cases()
INSTANTIATIONS = {(8, 4), (8, 1), (16, 4), (16, 1), (32, 2), (32, 1)}


def test_cases_reach_every_instantiation_and_map():
    seen, maps = {}, {}
    for p in STRUCTURE:
        seen.setdefault(p.values[-1], set()).add(p.values[2])
        maps.setdefault(p.values[3], set()).add(p.values[2])
    assert set(seen) == INSTANTIATIONS and all(len(v) == 3 for v in seen.values()), seen
    assert set(maps) == set(hc.MAP_KINDS) and all(len(v) == 3 for v in maps.values()), maps
    assert any(N % int(mk[4:]) for fl, N, _, mk, *_ in (p.values for p in STRUCTURE) if mk.startswith("hold"))


def structure_inputs(fl, N, F, tk, HW, C_ch, seed):
    rng = np.random.default_rng(26000 + seed)
    taps = rng.standard_normal((2, fl)).astype(np.float32) if tk == "rand" else real_taps(fl)
    g0 = rng.standard_normal((N, 2, HW)).astype(np.float32)
    src = rng.uniform(1.0, 70.0, (C_ch, F, HW)).astype(np.float32)
    out = rng.random(src.shape) < 0.1                      # a tenth of the samples outside the display's range: exact zeros
    src[out] = np.where(rng.random(int(out.sum())) < 0.5, np.float32(1e-3), np.float32(500.0))
    src[0, F - 1, HW // 2] = np.float32(500.0)
    if seed % 2:
        return taps, g0, src, nat.EOTF_LINEAR, dict(Y_peak=100.0, Y_black=0.1)
    return taps, g0, src, nat.EOTF_ABSOLUTE, dict(L_min=0.5, L_max=80.0)


@pytest.mark.parametrize("fl,N,padding,mk,tk,W,H,C_ch,layout,seed,variant", STRUCTURE)
def test_held_transpose_per_sample(fl, N, padding, mk, tk, W, H, C_ch, layout, seed, variant):
    """Each output is one chain of fp32 additions of terms tap * g0 -- 2 fl fused multiply-adds per list position, up to fl head
    positions, and K_j streaming positions of frame j, each one more addition -- then two multiplications, so
        |got - ref| <= (3 fl + K_j + 6) 2^-24 w_c S,     S = the same sum over |tap * g0| in float64.
    DERIVED, not measured.  Where S = 0 (a sample outside the display's range, or a frame no position shows) the result is an
    exact zero."""
    HW = W * H
    m, F = hc.c_abi_map(mk, N)
    taps, g0, src, kind, prm = structure_inputs(fl, N, F, tk, HW, C_ch, seed)
    e = eotf_struct(kind, **prm)
    got_t, widx = run_held(W, H, N, m, F, fl, padding, taps, g0, src, e, layout)
    got = got_t.numpy()
    comp = href.composed(m, widx)
    wts = RGB2Y if C_ch == 3 else np.ones(1, np.float32)
    ref, S = href.grad_input(comp, taps, g0, src, wts, kind, **prm)
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    K = href.streaming_counts(m, F).reshape(1, F, 1)
    bound = (3 * fl + K + 6) * U * S
    zero = S == 0
    print("worst |got - ref| / bound %.3f; exact zeros %d of %d" % (float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0,
                                                                    int(zero.sum()), zero.size))
    assert (got[zero] == 0).all()
    bad = np.argwhere(err > bound)
    assert bad.size == 0, "(channel, frame, pixel) of the first misses: %s" % bad[:8].tolist()
    assert zero.any() and not zero.all()
    shown = np.zeros(F, bool)
    shown[comp] = True
    assert zero[:, ~shown].all() and (got[:, ~shown] == 0).all()          # a frame no position shows: written, exact zeros
    if mk in ("skip", "above0", "constant"):
        assert (~shown).any()
    # a second run gives the same bits
    if seed % 4 == 0:
        again, _ = run_held(W, H, N, m, F, fl, padding, taps, g0, src, e, layout)
        assert np.array_equal(bits(again), bits(got_t))
    # the scalar variant of the same ring adds the same terms in the same order: bit-identical
    if variant[1] > 1:
        assert layout != "off1"
        got1, _ = run_held(W, H, N, m, F, fl, padding, taps, g0, src, e, "off1" if layout == "cfhw" else "gap1")
        assert np.array_equal(bits(got1), bits(got_t))


IDENTITY = [(fl, N, padding, W, H, C_ch, layout)
            for fl, N, padding, (W, H), C_ch, layout in (
                (6, 9, "replicate", (4, 5), 3, "cfhw"), (8, 19, "circular", (121, 67), 1, "gap1"), (9, 8, "pingpong", (121, 68), 3, "fchw"),
                (16, 35, "circular", (2, 129), 1, "cfhw"), (17, 16, "replicate", (122, 69), 3, "cfhw"), (32, 67, "pingpong", (121, 67), 3, "off1"),
                (30, 2, "circular", (257, 2), 1, "gap4"))]


@pytest.mark.parametrize("dtype", [nat.FVVDP_F32, nat.FVVDP_F16, nat.FVVDP_BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("fl,N,padding,W,H,C_ch,layout", IDENTITY)
def test_identity_map_is_video_grad_input_st(fl, N, padding, W, H, C_ch, layout, dtype):
    HW = W * H
    rng = np.random.default_rng(fl * 100 + N)
    taps = rng.standard_normal((2, fl)).astype(np.float32)
    g0 = rng.standard_normal((N, 2, HW)).astype(np.float32)
    src = rng.uniform(-0.1, 1.1, (C_ch, N, HW)).astype(np.float32)
    e = eotf_struct(nat.EOTF_SRGB, Y_peak=200.0, Y_black=0.2)
    m = np.arange(N, dtype=np.int32)
    got, _ = run_held(W, H, N, m, N, fl, padding, taps, g0, src, e, layout, dtype)
    want, _ = run_held(W, H, N, m, N, fl, padding, taps, g0, src, e, layout, dtype, entry="st")
    assert torch.isfinite(want.float()).all() and (want != 0).any()
    assert np.array_equal(bits(got), bits(want))
