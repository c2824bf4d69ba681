"""GPU: a call that spans more than one launch window, for the three ingests whose kernels live outside fvvdp_hip.hip -- float YUV
planes (fvvdp_temporal_channels_yuv_planes), resized streams (fvvdp_temporal_channels_resized) and held frames
(fvvdp_temporal_channels_held) -- through the C ABI.  (The array ingest has tests/test_gpu_array_pixels.py for this.)

30 frames per second: 8 taps in the 8-slot ring, 313 output frames per launch.  314 output frames in one call (windows of 313 and
1) against the same frames in two calls split at 200 | 114 into the same slots (one window each, starting elsewhere): level 0 of
the two must be equal bit for bit, because the arithmetic of a pixel does not depend on where a window starts -- only the index
lists and the slot of a launch do, and those are what the shared host code (csrc/ingest_host.hpp) fills.  At 16x8 the ingests run
their vector variants; at 10x6 (4:2:0 needs even sizes) the per-pixel variants of those that have one.  The resized ingest has one
kernel family, so it runs at 16x8 alone."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd.fvvdp import window_frame_indices
from lowlevel import Pipeline

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
I32P = C.POINTER(C.c_int32)
FPS, N, SPLIT = 30, 314, 200
BT709 = (1.0, 0.0, 1.5748, 1.0, -0.187324, -0.468124, 1.0, 1.8556, 0.0)


@pytest.fixture(scope="module")
def metric():
    m = fv.fvvdp(display_name="standard_fhd", device=DEV)
    fl, _ = m._temporal_taps(FPS)
    assert fl == 8 and 320 - 7 == 313 < N           # two windows in the one call, one in each call of the split
    return m


def stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def rand(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).to(DEV)


def one_call_against_two(m, W, H, ingest):
    """ingest(handle, lists, fl, taps, n_out, slot0) with `lists` a function of (first output frame, n_out) that returns the call's
    window list: level 0 [N, 4, H, W] of the single call, and of the two calls, each in a context of its own."""
    fl, taps = m._temporal_taps(FPS)
    widx = np.ascontiguousarray(window_frame_indices(N, fl, "replicate"), dtype=np.int32)
    assert widx.shape == (fl - 1 + N,)
    out = []
    for calls in (((0, N),), ((0, SPLIT), (SPLIT, N - SPLIT))):
        pipe = Pipeline(m, W, H, 4, N)
        try:
            for b0, nb in calls:
                ingest(pipe.handle, np.ascontiguousarray(widx[b0:b0 + fl - 1 + nb]), fl, taps, nb, b0)
            out.append(pipe.export_level(0, N).clone())
            torch.cuda.synchronize(DEV)
        finally:
            pipe.close()
    return out


def assert_same_level0(one, two):
    assert one.shape == two.shape and bool(torch.isfinite(one).all())
    assert float(one.abs().max()) > 1.0 and float((one[1:] - one[:-1]).abs().max()) > 0.0       # a clip, not a constant
    diff = (one.view(torch.int32) != two.view(torch.int32))
    assert not bool(diff.any()), "level 0 differs in %d values, first in frame %d" % (int(diff.sum()),
                                                                                     int(diff.flatten(1).any(1).nonzero()[0]))


@pytest.mark.parametrize("W,H", [(16, 8), (10, 6)])
def test_yuv_planes_ingest_across_windows(metric, W, H):
    m = metric
    _, e = m._image_eotf(torch.float32)
    w = np.asarray(m._rgb2y(), np.float32)
    fmt = nat.YuvFormat(8, 1, (C.c_float * 9)(*BT709))
    planes = []
    for s in range(2):                              # 8-bit code values, limited range and a little beyond it
        y, u, v = rand((N, H, W), 10.0, 240.0, 10 + s), rand((N, H // 2, W // 2), 10.0, 245.0, 20 + s), rand((N, H // 2, W // 2), 10.0, 245.0, 30 + s)
        planes.append((nat.YuvPlanes(y.data_ptr(), u.data_ptr(), v.data_ptr(), y.stride(0), u.stride(0)), (y, u, v)))
    oob = torch.zeros(1, dtype=torch.int32, device=DEV)

    def ingest(handle, idx, fl, taps, n_out, slot0):
        nat.check(nat.lib().fvvdp_temporal_channels_yuv_planes(handle, C.byref(planes[0][0]), C.byref(planes[1][0]), C.byref(fmt),
                                                               C.byref(e), nat.fptr(w), idx.ctypes.data_as(I32P), nat.fptr(taps), fl,
                                                               n_out, slot0, C.c_void_p(oob.data_ptr()), stream()))

    assert_same_level0(*one_call_against_two(m, W, H, ingest))


def test_resized_ingest_across_windows(metric):
    m = metric
    W, H = 16, 8
    _, e = m._image_eotf(torch.float32)
    w = np.asarray(m._rgb2y(), np.float32)
    clips = [rand((3, N, 4, 8), 0.0, 1.0, 40), rand((3, N, 8, 16), 0.0, 1.0, 41)]       # the test is upscaled, the reference is not
    streams = [nat.ResizeStream(x.data_ptr(), nat.FVVDP_F32, 3, x.shape[3], x.shape[2], x.stride(1), x.stride(0)) for x in clips]

    def ingest(handle, idx, fl, taps, n_out, slot0):
        nat.check(nat.lib().fvvdp_temporal_channels_resized(handle, C.byref(streams[0]), C.byref(streams[1]),
                                                            nat.RESIZE_MODES["bilinear"], C.byref(e), nat.fptr(w),
                                                            idx.ctypes.data_as(I32P), nat.fptr(taps), fl, n_out, slot0, stream()))

    assert_same_level0(*one_call_against_two(m, W, H, ingest))


HELD_RE = re.compile(r"fvvdp: held ingest: (\S+), FL 8, fl 8, dtype 2, C 3, eotf kind \d+, n_out (\d+), t0 (\d+)\n")


@pytest.mark.parametrize("W,H,variant", [(16, 8, "vector"), (10, 6, "per-pixel")])
def test_held_ingest_across_windows(metric, W, H, variant, monkeypatch, capfd):
    """The test stream has half the frames, each held twice.  10x6: the test's samples start one element off the 16 bytes that a
    lane's four pixels want, which takes the per-pixel variant; the FVVDP_DEBUG_VARIANT lines say which ran, in which windows."""
    m = metric
    monkeypatch.setenv("FVVDP_DEBUG_VARIANT", "1")
    monkeypatch.delenv("FVVDP_TEMPORAL_SCALAR", raising=False)
    _, e = m._image_eotf(torch.float32)
    w = np.asarray(m._rgb2y(), np.float32)
    HW, F = H * W, N // 2
    off = 0 if variant == "vector" else 1
    t_buf, r_buf = rand((3 * F * HW + off,), 0.0, 1.0, 50), rand((3 * N * HW,), 0.0, 1.0, 51)
    ts = nat.HeldStream(t_buf.data_ptr() + 4 * off, F * HW, HW, F)
    rs = nat.HeldStream(r_buf.data_ptr(), N * HW, HW, N)
    m_t, m_r = np.arange(N, dtype=np.int32) // 2, np.arange(N, dtype=np.int32)
    oob = torch.zeros(1, dtype=torch.int32, device=DEV)

    def ingest(handle, idx, fl, taps, n_out, slot0):
        it, ir = np.ascontiguousarray(m_t[idx]), np.ascontiguousarray(m_r[idx])
        nat.check(nat.lib().fvvdp_temporal_channels_held(handle, C.byref(ts), C.byref(rs), nat.FVVDP_F32, 3, C.byref(e), nat.fptr(w),
                                                         it.ctypes.data_as(I32P), ir.ctypes.data_as(I32P), nat.fptr(taps), fl, n_out,
                                                         slot0, C.c_void_p(oob.data_ptr()), stream()))

    capfd.readouterr()
    one, two = one_call_against_two(m, W, H, ingest)
    ran = [(g[0], int(g[1]), int(g[2])) for g in HELD_RE.findall(capfd.readouterr().err)]
    assert ran == [(variant, 313, 0), (variant, 1, 313), (variant, SPLIT, 0), (variant, N - SPLIT, 0)]
    assert_same_level0(one, two)
    assert int(oob.item()) == 0
