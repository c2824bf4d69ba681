"""The float64 reference of fvvdp_video_grad_input (tests/video_grad_input_ref.py) without a GPU: its sum equals the dense
transpose of the forward's temporal filter, that forward matrix reproduces the oracle's temporal channels, and its display
derivatives equal central differences of the oracle's float64 display model.  The GPU test holds the kernel against this
reference, so the reference is pinned here, on code that shares nothing with the kernel."""
import os
import sys

import numpy as np
import pytest

from fovvideovdp_amd import _native as nat
from fovvideovdp_amd.fvvdp import window_frame_indices

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_grad_input_ref as vref          # noqa: E402

CASES = [(2, 30), (5, 6), (7, 6), (9, 8), (8, 8), (3, 1), (17, 16), (12, 17), (5, 64), (67, 33)]


def _taps(fl, seed):
    return np.random.default_rng(seed).standard_normal((2, fl)).astype(np.float32)


@pytest.mark.parametrize("N,fl", CASES)
@pytest.mark.parametrize("padding", ["replicate", "circular", "pingpong"])
def test_reference_is_the_dense_transpose(N, fl, padding):
    idx = window_frame_indices(N, fl, padding)
    taps = _taps(fl, 100 + fl)
    rng = np.random.default_rng(N * 1000 + fl)
    g0 = rng.standard_normal((N, 2, 11))
    M = vref.forward_matrix(idx, taps, N).reshape(N * 2, N)
    dense = M.T @ g0.reshape(N * 2, 11)
    got = vref.dlum(idx, taps, g0)
    scale = vref.forward_matrix(idx, np.abs(taps), N).reshape(N * 2, N).T @ np.abs(g0).reshape(N * 2, 11)
    assert np.abs(got - dense).max() <= 1e-13 * scale.max()
    # the error scale is the same sum over the absolute values, and it is zero exactly where no window shows a frame
    S = vref.dlum(idx, taps, g0, absolute=True)
    assert np.abs(S - scale).max() <= 1e-13 * scale.max()
    shown = np.zeros(N, bool)
    shown[np.asarray(idx)] = True
    assert ((S == 0).all(axis=1) == ~shown).all()
    if padding == "circular" and N > fl + 1:
        assert not shown[0] and (got[0] == 0).all()


@pytest.mark.parametrize("N,fl", CASES)
@pytest.mark.parametrize("padding", ["replicate", "circular", "pingpong"])
def test_forward_matrix_reproduces_the_oracles_temporal_channels(N, fl, padding):
    from oracle import fvvdp_oracle as orc
    idx = window_frame_indices(N, fl, padding)
    taps = _taps(fl, 200 + fl)
    if fl > 1:                                       # the metric's own taps as well (its filters need two taps)
        real = orc.temporal_filters(4 * fl - 2, fl=fl, dtype=np.float64)
        assert orc.filter_len(4 * fl - 2) == fl
    rng = np.random.default_rng(N * 1000 + fl + 1)
    lum_t, lum_r = rng.uniform(0.1, 200.0, (N, 3, 5)), rng.uniform(0.1, 200.0, (N, 3, 5))
    widx = orc.window_frame_indices(N, fl, padding)              # [N, fl], oldest first
    for tp in ([taps] if fl == 1 else [taps, real]):
        tp = np.asarray(tp, dtype=np.float64)
        M = vref.forward_matrix(idx, tp, N)
        X = np.einsum("fcj,jyx->fcyx", M, lum_t)
        for f in range(N):
            R = orc.temporal_channels(lum_t[widx[f]], lum_r[widx[f]], tp, dtype=np.float64)
            assert np.abs(X[f, 0] - R[0]).max() <= 1e-12 * np.abs(R[0]).max() + 1e-12
            assert np.abs(X[f, 1] - R[2]).max() <= 1e-12 * np.abs(lum_t).max() * np.abs(tp[1]).sum() + 1e-12


@pytest.mark.parametrize("eotf,kind,prm", [
    ("sRGB", nat.EOTF_SRGB, dict(Y_peak=200.0, contrast=1000)), ("gamma", nat.EOTF_GAMMA, dict(Y_peak=300.0, contrast=800, gamma=2.2)),
    ("gamma", nat.EOTF_GAMMA, dict(Y_peak=300.0, contrast=800, gamma=1.8)), ("PQ", nat.EOTF_PQ, dict(Y_peak=1500.0, contrast=1e6)),
    ("PQ", nat.EOTF_PQ, dict(Y_peak=400.0, contrast=1e6)), ("linear", nat.EOTF_LINEAR, dict(Y_peak=1500.0, contrast=1e6))])
def test_display_derivatives_are_those_of_the_oracles_display_model(eotf, kind, prm):
    from oracle import fvvdp_oracle as orc
    ph = orc.Photometry(prm["Y_peak"], contrast=prm["contrast"], EOTF=eotf, gamma=prm.get("gamma", 2.2), dtype=np.float64)
    if kind == nat.EOTF_LINEAR:
        V = np.concatenate([np.linspace(0.0, 0.004, 9), np.linspace(0.006, 1499.0, 301), np.linspace(1501.0, 1800.0, 7)])
    else:
        V = np.concatenate([np.linspace(-0.3, -0.01, 7), np.linspace(0.002, 0.998, 499), np.linspace(1.01, 1.4, 7)])
    V = V.astype(np.float32)
    h = 1e-6 * np.maximum(np.abs(V.astype(np.float64)), 1e-3)
    # the oracle clamps (and flags) a whole array when one value lies outside [0, 1]: the same values as per sample
    fd = (ph.forward(V.astype(np.float64) + h)[0] - ph.forward(V.astype(np.float64) - h)[0]) / (2 * h)
    d = vref.eotf_grad(V, kind, Y_peak=prm["Y_peak"], Y_black=ph.get_black_level(), gamma=prm.get("gamma", 2.2))
    # samples whose difference stencil straddles a kink (the sRGB knee, a clamp of PQ) are left out: at most a handful
    L = vref.pq_luminance(V) if kind == nat.EOTF_PQ else None
    near = np.abs(V - vref.SRGB_KNEE) < 1e-5 if kind == nat.EOTF_SRGB else np.zeros(V.shape, bool)
    if kind == nat.EOTF_PQ:
        near = (np.abs(L / 0.005 - 1) < 1e-3) | (np.abs(L / prm["Y_peak"] - 1) < 1e-3)
    assert near.sum() <= 4
    ok = ~near
    assert (d[ok] != 0).sum() > 250 and (d[ok] == 0).sum() >= 10
    assert (fd[ok][d[ok] == 0] == 0).all()
    nz = ok & (d != 0)
    assert np.abs(fd[nz] / d[nz] - 1).max() < 1e-6


def test_display_derivative_of_the_absolute_model():
    V = np.array([0.001, 0.0049, 0.005, 0.0051, 1.0, 9999.0, 10000.0, 10001.0], np.float32)
    d = vref.eotf_grad(V, nat.EOTF_ABSOLUTE, L_min=0.005, L_max=10000.0)
    assert d.tolist() == [0, 0, 1, 1, 1, 1, 1, 0]


def test_pq_inverse_round_trips():
    L = np.array([0.005, 0.1, 10.0, 400.0, 1500.0, 10000.0])
    assert np.abs(vref.pq_luminance(vref.pq_inverse(L)) / L - 1).max() < 1e-9
