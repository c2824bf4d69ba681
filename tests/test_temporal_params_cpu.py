"""Gradients with respect to sustained_sigma and sustained_beta without a GPU: the header and its binding, the argument checks
of its entry points, the code objects of the new kernels, the taps under phi against get_temporal_filters, the chain taps -> phi
against central differences of the oracle's float64 filters, the float64 tap sums of the helper against central differences
through the oracle's temporal_channels, and the refusals that come before any device work."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd.fvvdp import filter_length, temporal_filters, window_frame_indices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_grad_ref as ref            # noqa: E402
from temporal_grad_ref import orc           # noqa: E402

# the bound test_params_cpu.py uses for its chain: both sides float64, the differences' truncation and cancellation errors are of
# the order 1e-9 relative; here relative to the largest entry of the Jacobian
CHAIN_BOUND = 1e-6


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def test_taps_header_is_exported_and_bound():
    nat.build()
    names = declared("fvvdp_hip_taps.h")
    assert names == ["fvvdp_luminance_frames", "fvvdp_tap_grad", "fvvdp_tap_grad_workspace"]
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert sorted(nat.TAP_SYMBOLS) == names
    others = set(nat.SYMBOLS) | set(nat.IMAGE_SYMBOLS) | set(nat.GRAD_SYMBOLS) | set(nat.VIDEO_GRAD_SYMBOLS) | \
        set(nat.GAZE_SYMBOLS) | set(nat.GAZE_GRAD_SYMBOLS) | set(nat.REF_GRAD_SYMBOLS) | set(nat.PARAM_SYMBOLS)
    assert not set(names) & others
    lib = nat.lib()
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    hdr = open(os.path.join(ROOT, "include", "fvvdp_hip_taps.h")).read()
    assert "#define FVVDP_TAPS_MAX_POSITIONS %d\n" % nat.TAPS_MAX_POSITIONS in hdr
    assert "#define FVVDP_TAP_GROUP %d\n" % nat.TAP_GROUP in hdr


def test_argument_checks_need_no_device():
    lib = nat.lib()
    nbytes = ctypes.c_size_t(0)
    assert lib.fvvdp_tap_grad_workspace(64, 48, 8, None) == -1 and b"null" in lib.fvvdp_last_error()
    assert lib.fvvdp_tap_grad_workspace(0, 48, 8, ctypes.byref(nbytes)) == -1 and b"frame size" in lib.fvvdp_last_error()
    assert lib.fvvdp_tap_grad_workspace(64, 48, 0, ctypes.byref(nbytes)) == -1 and b"filter length" in lib.fvvdp_last_error()
    assert lib.fvvdp_tap_grad_workspace(64, 48, 65, ctypes.byref(nbytes)) == nat.FVVDP_EUNSUPPORTED
    assert b"65 taps" in lib.fvvdp_last_error()
    # partial [ceil(fl / 8)][ceil(HW / 256)][2][8] fp64
    assert lib.fvvdp_tap_grad_workspace(64, 48, 8, ctypes.byref(nbytes)) == 0 and nbytes.value == 1 * 12 * 16 * 8
    assert lib.fvvdp_tap_grad_workspace(121, 68, 15, ctypes.byref(nbytes)) == 0 and nbytes.value == 2 * 33 * 16 * 8
    assert lib.fvvdp_tap_grad_workspace(121, 68, 64, ctypes.byref(nbytes)) == 0 and nbytes.value == 8 * 33 * 16 * 8

    p = ctypes.c_void_p(256)
    pos = (ctypes.c_int32 * 400)()

    def taps(n=3, fl=8, g0=p, g0r=p, yt=p, yr=p, pos_=pos, n_lum=1, out=p, work=p, work_bytes=1 << 20):
        return lib.fvvdp_tap_grad(64, 48, n, fl, g0, g0r, yt, yr, pos_, n_lum, out, work, work_bytes, None)

    for hole in ("g0", "g0r", "yt", "yr", "pos_", "out", "work"):
        assert taps(**{hole: None}) == -1 and b"null" in lib.fvvdp_last_error(), hole
    assert taps(n=0) == -1 and b"window list" in lib.fvvdp_last_error()
    assert taps(n=314, fl=8) == -1 and b"window list" in lib.fvvdp_last_error()         # 7 + 314 entries
    assert taps(fl=65) == nat.FVVDP_EUNSUPPORTED
    assert taps(n_lum=0) == -1 and b"n_lum" in lib.fvvdp_last_error()
    assert taps(yt=ctypes.c_void_p(258)) == -1 and b"4 bytes" in lib.fvvdp_last_error()
    assert taps(out=ctypes.c_void_p(260)) == -1 and b"8 bytes" in lib.fvvdp_last_error()
    assert taps(work=ctypes.c_void_p(264)) == -1 and b"256-byte" in lib.fvvdp_last_error()
    assert taps(work_bytes=64) == -1 and b"workspace" in lib.fvvdp_last_error()
    pos[9] = 1
    assert taps(n_lum=1) == -1 and b"entry 9" in lib.fvvdp_last_error()
    pos[9] = -1
    assert taps(n_lum=4) == -1 and b"entry 9" in lib.fvvdp_last_error()
    pos[9] = 0

    e = nat.Eotf()
    e.kind, e.Y_peak, e.Y_black = nat.EOTF_SRGB, 100.0, 0.1
    w = np.asarray([0.2, 0.7, 0.1], dtype=np.float32)
    fr = (ctypes.c_int32 * 400)()

    def lum(test=p, ref_=p, dtype=nat.FVVDP_F32, C=3, W=64, H=48, eotf=e, w_=w, fr_=fr, n=2, out=p):
        return lib.fvvdp_luminance_frames(test, ref_, dtype, C, W, H, 64 * 48 * 4, 64 * 48, ctypes.byref(eotf) if eotf else None,
                                          nat.fptr(w_) if w_ is not None else None, fr_, n, out, None, None)

    for hole in ("test", "ref_", "eotf", "fr_", "out"):
        assert lum(**{hole: None}) == -1 and b"null" in lib.fvvdp_last_error(), hole
    assert lum(dtype=3) == -1 and b"uint8, uint16 and float32" in lib.fvvdp_last_error()
    assert lum(C=2) == -1 and b"1 or 3" in lib.fvvdp_last_error()
    assert lum(w_=None) == -1 and b"rgb2y" in lib.fvvdp_last_error()
    assert lum(W=0) == -1 and b"frame size" in lib.fvvdp_last_error()
    assert lum(n=0) == -1 and lum(n=321) == -1 and b"frames in one call" in lib.fvvdp_last_error()
    assert lum(dtype=nat.FVVDP_U8) == -1 and b"uint8 sources need" in lib.fvvdp_last_error()
    lut = nat.Eotf()
    lut.kind = nat.EOTF_LUT
    assert lum(eotf=lut, dtype=nat.FVVDP_U8) == -1 and b"table" in lib.fvvdp_last_error()
    assert lum(test=ctypes.c_void_p(258)) == -1 and b"element size" in lib.fvvdp_last_error()
    fr[1] = -2
    assert lum() == -1 and b"negative" in lib.fvvdp_last_error()


def test_new_kernels_do_not_spill():
    import codeobj
    nat.build()
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    names = list(md)
    nice = codeobj.demangle(names)
    # registers per lane: two waves per SIMD for the 4-pixel variant (ring 64 + sums 16 + 32 + two frames in flight), more
    # for the 1-pixel variant
    found = {"void tap_grad_kernel<8, 4>": 256, "void tap_grad_kernel<8, 1>": 128, "tap_finalize_kernel": 64}
    seen = dict.fromkeys(found, 0)
    for m, n in zip(names, nice):
        base = n.split("(")[0]
        if base in found:
            seen[base] += 1
            x = md[m]
            assert (x["sgpr_spill_count"], x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), (n, x)
            assert x["vgpr_count"] + x.get("agpr_count", 0) <= found[base], (n, x)
    assert seen == {k: 1 for k in found}


# (values at which the filter keeps several taps of comparable size: a filter that has collapsed onto one tap has derivatives
# of the order of the differences' own cancellation error)
PHIS = ((0.5, 0.06), (0.6, 0.048), (0.41, 0.0725), (1.3, 0.2), (0.35, 0.03))


@pytest.mark.parametrize("fps", [24, 30, 60, 120, 240])
def test_taps_under_phi_are_the_bits_of_get_temporal_filters(fps):
    base = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    own = (base.sustained_sigma, base.sustained_beta)
    fl = filter_length(fps)
    for sigma, beta in PHIS:
        m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
        m.set_temporal_parameters(torch.tensor([sigma, beta], dtype=torch.float64))
        assert (m.sustained_sigma, m.sustained_beta) == (sigma, beta) and type(m.sustained_sigma) is float
        m.filter_len = fl
        F, omega = m.get_temporal_filters(fps)
        T = temporal_filters(fps, fl, sigma, beta)
        assert T.dtype == torch.float32 and T.shape == (2, fl) and torch.equal(T, F) and omega.tolist() == [0, 5]
        got_fl, taps = m._temporal_taps(fps)
        assert got_fl == fl and np.array_equal(taps, T.numpy())
        assert T[1, -1] == 0
    assert (base.sustained_sigma, base.sustained_beta) == own
    # the oracle's fp32 restatement of the same expressions agrees to rounding
    T = temporal_filters(fps, fl, *own).numpy()
    assert np.allclose(T, orc.temporal_filters(fps, own[0], own[1], fl), rtol=2e-5, atol=1e-7)


def test_temporal_parameter_vector_round_trip():
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    assert fv.fvvdp.TEMPORAL_PARAMETER_NAMES == ("sustained_sigma", "sustained_beta") == ref.NAMES
    assert len(fv.fvvdp.PARAMETER_NAMES) == 12 and not set(ref.NAMES) & set(fv.fvvdp.PARAMETER_NAMES)
    phi = m.temporal_parameter_tensor()
    assert phi.dtype == torch.float64 and phi.device.type == "cpu" and phi.shape == (2,)
    assert np.array_equal(phi.numpy(), ref.phi0())
    m.set_temporal_parameters(phi * torch.tensor([1.25, 0.5], dtype=torch.float64))
    assert torch.equal(m.temporal_parameter_tensor(), phi * torch.tensor([1.25, 0.5], dtype=torch.float64))
    assert type(m.sustained_sigma) is float and type(m.sustained_beta) is float
    m.set_temporal_parameters([0.5, 0.06])
    assert torch.equal(m.temporal_parameter_tensor(), phi)
    for bad, msg in ((phi[:1], "1-D vector of the 2 parameters"), (phi.view(1, 2), "1-D vector"),
                     (torch.tensor([float("nan"), 0.06]), "non-finite.*sustained_sigma"),
                     (torch.tensor([0.5, 0.0]), "sustained_beta must be positive")):
        with pytest.raises(RuntimeError, match=msg):
            m.set_temporal_parameters(bad)
    assert torch.equal(m.temporal_parameter_tensor(), phi)


def test_refusals_come_before_any_device_work():
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    th, phi = m.parameter_tensor(), m.temporal_parameter_tensor()
    before = dict(vars(m))
    x, r = torch.rand((1, 3, 4, 32, 48)), torch.rand((1, 3, 4, 32, 48))

    def video(temporal, fps=30, metric=m, theta=th):
        return metric.calibration_jod_video(x, r, theta, frames_per_second=fps, temporal=temporal)

    with pytest.raises(RuntimeError, match="1-D vector of the 2 parameters"):
        video(phi[:1])
    with pytest.raises(RuntimeError, match="1-D vector"):
        video(torch.cat([phi, phi]).view(2, 2))
    with pytest.raises(RuntimeError, match="float32 or float64"):
        video(torch.tensor([1, 1]))
    for i, n in enumerate(ref.NAMES):
        for v in (float("nan"), float("inf")):
            bad = phi.clone()
            bad[i] = v
            with pytest.raises(RuntimeError, match="non-finite.*%s" % n):
                video(bad)
        for v in (0.0, -0.5):
            bad = phi.clone()
            bad[i] = v
            with pytest.raises(RuntimeError, match="%s must be positive" % n):
                video(bad)
    # more than VIDEO_GRAD_MAX_TAPS taps: refused with a gradient; the forward alone goes on to the next refusal (no device)
    assert filter_length(260) == 65 > nat.VIDEO_GRAD_MAX_TAPS
    with pytest.raises(RuntimeError, match="65 taps.*covers 64"):
        video(phi.clone().requires_grad_(True), fps=260)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        video(phi, fps=260)
    # theta's own checks come first, a heat-map metric stays refused, a still-image call has no such keyword
    with pytest.raises(RuntimeError, match="1-D vector of the 12 parameters"):
        video(phi, theta=th[:11])
    hm = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True, heatmap="raw")
    with pytest.raises(RuntimeError, match="no heat maps"):
        video(phi, metric=hm)
    with pytest.raises(TypeError):
        m.calibration_jod_images(x[:, :, 0], r[:, :, 0], th, temporal=phi)
    # accepted: float32 / float64, with and without grad, theta with and without grad -- the next refusal is the missing device
    for temporal in (None, phi, phi.float(), phi.clone().requires_grad_(True), phi.float().requires_grad_(True)):
        for theta in (th, th.clone().requires_grad_(True)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                video(temporal, theta=theta)
    now = vars(m)
    assert all(now[k] is before[k] or now[k] == before[k] for k in ref.NAMES + tuple(fv.fvvdp.PARAMETER_NAMES)) and m._ctx is None
    assert len(m._filters) == len(before["_filters"])             # phi's taps are not cached


@pytest.mark.parametrize("fps", [24, 30, 60, 120, 240])
def test_chain_from_taps_to_phi_matches_central_differences(fps):
    from fovvideovdp_amd import param_grad as pg
    fl = filter_length(fps)
    worst = 0.0
    for sigma, beta in PHIS:
        F, J = pg.taps_jacobian(float(fps), fl, sigma, beta)
        assert F.dtype == J.dtype == torch.float64 and J.shape == (2, fl, 2)
        phi = np.array([sigma, beta])
        F64 = orc.temporal_filters(fps, sigma, beta, fl, np.float64)
        assert np.abs(F.numpy() - F64).max() <= 1e-12 * np.abs(F64).max()
        fd = ref.dtaps_dphi_fd(fps, fl, phi)
        for i in range(2):
            err = np.abs(J.numpy()[:, :, i] - fd[:, :, i]).max() / np.abs(fd[:, :, i]).max()
            worst = max(worst, err)
            assert err < CHAIN_BOUND, (fps, sigma, beta, i, err)
        assert (J[1, -1] == 0).all() and F[1, -1] == 0              # the last transient tap is a constant
        g = torch.from_numpy(np.random.default_rng(fps).standard_normal((2, fl)))
        want = np.einsum("ck,cki->i", g.numpy(), J.numpy())
        assert np.allclose(pg.tap_chain(g.float().double(), float(fps), fl, sigma, beta).numpy(),
                           np.einsum("ck,cki->i", g.float().double().numpy(), J.numpy()), rtol=1e-12, atol=0) and want.shape == (2,)
    print("fps %d worst %.2e" % (fps, worst))


@pytest.mark.parametrize("pad", ["replicate", "circular", "pingpong"])
@pytest.mark.parametrize("N,fps", [(5, 30), (12, 30), (4, 60)])
def test_tap_sums_ref_pairs_taps_and_window_slots_as_the_oracle(pad, N, fps):
    """sum G Z is linear in every tap, Z from the oracle's own temporal_channels: its central differences are the tap sums."""
    fl = orc.filter_len(fps)
    rng = np.random.default_rng(N * 1000 + fps + len(pad))
    H, W = 5, 7
    Y_T, Y_R = rng.uniform(1.0, 100.0, (N, H, W)), rng.uniform(1.0, 100.0, (N, H, W))
    G, G_r = rng.standard_normal((N, 2, H, W)), rng.standard_normal((N, 2, H, W))
    widx = orc.window_frame_indices(N, fl, pad)
    flat = window_frame_indices(N, fl, pad)
    assert np.array_equal(ref.windows(flat, N, fl), widx)            # the product's flat list is the same windows
    taps = orc.temporal_filters(fps, 0.5, 0.06, fl, np.float64)

    def total(tp):
        s = 0.0
        for t in range(N):
            Z = orc.temporal_channels(Y_T[widx[t]], Y_R[widx[t]], tp, np.float64)
            for cc in range(2):
                s += (G[t, cc] * Z[2 * cc]).sum() + (G_r[t, cc] * Z[2 * cc + 1]).sum()
        return s

    out, mag = ref.tap_sums_ref(G, G_r, Y_T, Y_R, widx)
    h = 1e-3
    for cc in range(2):
        for k in range(fl):
            P, M = taps.copy(), taps.copy()
            P[cc, k] += h
            M[cc, k] -= h
            fd = (total(P) - total(M)) / (2 * h)
            assert abs(fd - out[cc, k]) <= 1e-9 * mag[cc, k], (cc, k, fd, out[cc, k])
    # a batch that starts at b0 > 0 is the same windows, shifted
    if N > 3:
        sub, _ = ref.tap_sums_ref(G[2:], G_r[2:], Y_T, Y_R, ref.windows(flat, N - 2, fl, 2))
        head, _ = ref.tap_sums_ref(G[:2], G_r[:2], Y_T, Y_R, ref.windows(flat, 2, fl, 0))
        assert np.allclose(sub + head, out, rtol=1e-12, atol=1e-9)
