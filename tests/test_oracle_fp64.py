"""The CPU oracle's float64 mode (`Oracle(..., dtype=np.float64)`, `dtype=` on the pyramid functions): the high-precision
yardstick that the GPU pixel tests (tests/test_gpu_band2_pixels.py) compare the kernels with.

Bounds against the reference captures are 3x the values measured when this mode was written (quoted next to each assert);
the fp32 mode stays pinned bit for bit by test_oracle_golden.py."""
import numpy as np
import pytest

from oracle import fvvdp_oracle as orc
from fovvideovdp_amd.synth import synth_video_pair
from test_oracle_golden import load

F64 = np.float64


def _rel(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return np.abs(a - b) / np.abs(b)


def test_fp64_mode_is_float64_end_to_end():
    test, ref = synth_video_pair(4, 36, 70)
    o = orc.Oracle("standard_fhd", dtype=F64)
    o.capture = {}
    jod, st = o.predict(test.numpy(), ref.numpy(), frames_per_second=30)
    assert isinstance(jod, np.float64) and st["Q_per_ch"].dtype == F64 and o.F.dtype == F64
    for key in ("R", "S", "D"):
        assert all(a.dtype == F64 for a in o.capture[key]), key
    assert all(b.dtype == F64 for bands in o.capture["bands"] for b in bands)
    assert all(b.dtype == F64 for lb in o.capture["L_bkg"] for b in lb)
    assert all(v.dtype == F64 for lut in o.lut for v in lut.values())
    assert o.photometry.forward(np.array([0.5], np.float32))[0].dtype == F64
    # the taps are the exact float64 values of the reference's expressions, not their fp32 roundings
    assert np.array_equal(orc._k(F64), np.array([0.25 - 0.4 / 2.0, 0.25, 0.4, 0.25, 0.25 - 0.4 / 2.0]))
    assert orc._k().dtype == np.float32 and not np.array_equal(orc._k().astype(F64), orc._k(F64))
    # the default stays float32
    jod32, st32 = orc.Oracle("standard_fhd").predict(test.numpy(), ref.numpy(), frames_per_second=30)
    assert isinstance(jod32, np.float32) and st32["Q_per_ch"].dtype == np.float32
    assert abs(float(jod) - float(jod32)) < 1e-5


def test_fp64_mode_foveated_and_hdr_are_float64():
    test, ref = synth_video_pair(3, 40, 64)
    jod, st = orc.Oracle("standard_fhd", foveated=True, dtype=F64).predict(test.numpy(), ref.numpy(), frames_per_second=30,
                                                                           fixation_point=[10, 20])
    assert st["Q_per_ch"].dtype == F64
    o = orc.Oracle("standard_hdr_pq", dtype=F64)
    V = np.linspace(0, 1, 17, dtype=np.float32)
    L, _ = o.photometry.forward(V)
    L32, _ = orc.Photometry.load("standard_hdr_pq").forward(V)
    assert L.dtype == F64 and np.all(_rel(L, L32)[V > 0.1] < 2e-4)


def test_fp64_mode_agrees_with_golden_g1():
    z = load("g1_crop512_blur_fhd")
    z0 = load("g0_wavy_facade_blur_4k")
    ref = z0["ref_u16"][85:597, 256:768]
    jod, st = orc.Oracle("standard_fhd", dtype=F64).predict(z["test_u16"], ref, dim_order="HWC")
    assert abs(float(jod) - float(z["jod"])) < 2e-5                                 # measured 7.2e-6
    e = _rel(st["Q_per_ch"][:, 0, 0], z["Q_per_ch"][:, 0, 0])
    assert np.all(e < 4e-5), e                                                       # measured 1.0e-5 (band 2)


@pytest.mark.parametrize("H,W,N,fps", [(135, 240, 10, 30), (68, 121, 12, 60)])
def test_fp64_mode_agrees_with_golden_g2(H, W, N, fps):
    test, ref = synth_video_pair(N, H, W)
    test, ref = test.numpy(), ref.numpy()
    for pad in ("replicate", "circular", "pingpong"):
        z = load(f"g2_video_{H}x{W}_{pad}")
        o = orc.Oracle("standard_fhd", temp_padding=pad, dtype=F64)
        jod, st = o.predict(test, ref, frames_per_second=fps)
        assert np.max(np.abs(o.F - z["F"])) < 6e-7 * np.max(np.abs(z["F"]))        # measured 1.7e-7
        assert abs(float(jod) - float(z["jod"])) < 2.5e-6, pad                        # measured 6.9e-7
        e = _rel(st["Q_per_ch"], z["Q_per_ch"])
        assert np.all(e[:3] < 1.5e-4), (pad, e[:3].max())                            # measured 5.0e-5 (the three finest bands)
        assert np.all(e < 4.5e-3), (pad, e.max())                                     # measured 1.4e-3 (the coarsest band)


def _reduce_matrix(n, parity_odd):
    """One axis of the reference's reduce as an [ceil(n/2), n] float64 matrix: 5-tap stride-2 taps on a zero-padded axis plus
    the first / last output fix-ups; the last one is chosen by `parity_odd` (fvvdp_lpyr_dec.py:190-205)."""
    K = [0.25 - 0.4 / 2.0, 0.25, 0.4, 0.25, 0.25 - 0.4 / 2.0]
    no = (n + 1) // 2
    M = np.zeros((no, n))
    for i in range(no):
        for k in range(5):
            j = 2 * i + k - 2
            if 0 <= j < n:
                M[i, j] += K[k]
    M[0, 0] += K[1]
    M[0, 1] += K[0]
    if parity_odd:
        M[no - 1, n - 1] += K[3]
        M[no - 1, n - 2] += K[4]
    else:
        M[no - 1, n - 1] += K[4]
    return M


@pytest.mark.parametrize("H,W", [(12, 16), (13, 16), (12, 17), (13, 17), (4, 5), (5, 4), (4, 4), (7, 9), (64, 33), (31, 120)])
def test_fp64_reduce_equals_independent_statement(H, W):
    """y = Mr(H) x Mc(W)^T, where BOTH fix-ups follow the parity of the ROW count H (the reference's quirk, :202)."""
    rng = np.random.RandomState(H * 100 + W)
    x = rng.rand(2, H, W) * 100 + 1
    y = orc.gausspyr_reduce(x, F64)
    assert y.dtype == F64
    Mr, Mc = _reduce_matrix(H, H % 2 == 1), _reduce_matrix(W, H % 2 == 1)
    want = np.einsum("ij,pjk,lk->pil", Mr, x, Mc)
    assert y.shape == want.shape
    assert np.max(_rel(y, want)) < 1e-14
    if H % 2 != W % 2:           # the quirk is live: the column-parity fix-up would give a different last column
        alt = np.einsum("ij,pjk,lk->pil", Mr, x, _reduce_matrix(W, W % 2 == 1))
        assert np.max(_rel(alt[:, :, -1], want[:, :, -1])) > 1e-3
        assert np.array_equal(alt[:, :, :-1], want[:, :, :-1]) or np.max(_rel(alt[:, :, :-1], want[:, :, :-1])) < 1e-14


def test_fp64_reduce_of_fp32_input_and_pyramid():
    rng = np.random.RandomState(3)
    x32 = (rng.rand(4, 45, 77) * 200 + 0.5).astype(np.float32)
    y64 = orc.gausspyr_reduce(x32, F64)
    y32 = orc.gausspyr_reduce(x32)
    assert y64.dtype == F64 and y32.dtype == np.float32
    assert np.max(_rel(y32, y64)) < 1e-6
    pyr = orc.gaussian_pyramid(x32.astype(F64), 4, F64)
    assert all(p.dtype == F64 for p in pyr)
    assert np.array_equal(pyr[2], orc.gausspyr_reduce(orc.gausspyr_reduce(x32, F64), F64))
    bands, lbkg = orc.contrast_pyr_decompose(x32.astype(F64), 3, F64)
    assert all(b.dtype == F64 for b in bands) and all(b.dtype == F64 for b in lbkg)
