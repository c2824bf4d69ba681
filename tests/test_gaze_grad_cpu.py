"""Many-gaze gradients without a GPU: the sixth C header and its binding, the argument checks of its entry points, the code
objects of gaze_layer_kernel, the numpy restatement of its CSF query against the oracle's interpolation, and the refusals of
fvvdp.jod_gazes that come before any device work."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gaze_grad_cases import s_query          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["void gaze_layer_kernel<%d>" % ng for ng in (1, 2, 4, 8)]


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def test_gaze_grad_header_is_exported_and_bound():
    nat.build()
    names = declared("fvvdp_hip_gaze_grad.h")
    assert names == ["fvvdp_gaze_grad_frames", "fvvdp_gaze_grad_workspace"]
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert sorted(nat.GAZE_GRAD_SYMBOLS) == names
    others = set(nat.SYMBOLS) | set(nat.IMAGE_SYMBOLS) | set(nat.GRAD_SYMBOLS) | set(nat.VIDEO_GRAD_SYMBOLS) | set(nat.GAZE_SYMBOLS)
    assert not set(names) & others
    lib = nat.lib()
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    # the helpers the new unit shares with the video backward stay internal
    for name in ("video_coef_launch", "video_level0_launch", "grad_sweep_launch"):
        assert not hasattr(L, name), name


def test_workspace_is_the_single_gaze_layout_plus_coefficients():
    lib = nat.lib()
    nbytes, one = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.fvvdp_gaze_grad_workspace(64, 48, 4, 3, 5, None) == -1
    assert lib.fvvdp_gaze_grad_workspace(64, 48, 0, 3, 5, ctypes.byref(nbytes)) == -1
    assert lib.fvvdp_gaze_grad_workspace(64, 48, 17, 3, 5, ctypes.byref(nbytes)) == -1
    assert lib.fvvdp_gaze_grad_workspace(64, 48, 4, 0, 5, ctypes.byref(nbytes)) == -1
    assert lib.fvvdp_gaze_grad_workspace(0, 48, 4, 3, 5, ctypes.byref(nbytes)) == -1
    assert lib.fvvdp_gaze_grad_workspace(64, 48, 4, 3, 0, ctypes.byref(nbytes)) == -1 and b"n_gazes" in lib.fvvdp_last_error()
    assert lib.fvvdp_gaze_grad_workspace(64, 48, 4, 3, -3, ctypes.byref(nbytes)) == -1
    al = lambda x: (x + 63) // 64 * 64
    prev = 0
    for n in (1, 2, 3, 7, 30):                   # monotone in n; the gazes add their coefficients and nothing else
        assert lib.fvvdp_video_grad_workspace(64, 48, 4, n, ctypes.byref(one)) == 0
        for G in (1, 5, 17):
            assert lib.fvvdp_gaze_grad_workspace(64, 48, 4, n, G, ctypes.byref(nbytes)) == 0
            assert nbytes.value == one.value + 4 * G * al(n * 2 * 4)
        assert nbytes.value > prev
        prev = nbytes.value


def test_frames_argument_checks_need_no_device():
    lib = nat.lib()
    prm, pp = nat.Params(), nat.PoolParams(1, 0.67, 1, 0.25, -0.016, 0.6)
    prm.beta = 0.96
    geom = nat.Geom()
    geom.display_size_m[0], geom.display_size_m[1], geom.distance_m, geom.ppd_centre = 0.66, 0.37, 0.75, 60.0
    maps = (nat.BandMaps * 4)()
    for b in range(4):
        maps[b].d_D = maps[b].d_contrast = maps[b].d_lbkg = maps[b].d_S = 256
    rho = np.array([30.0, 9.7, 4.8, 2.4, 1.2], np.float64)
    axes = np.stack([np.linspace(-10, 13, 32), np.linspace(-4, 6, 32), np.linspace(0, 11, 32)]).astype(np.float32)
    p = ctypes.c_void_p(256)
    dp = ctypes.POINTER(ctypes.c_double)

    def call(n_bands=4, n=2, G=3, n_frames=5, f0=0, work=1 << 30, work_ptr=256, mp=maps, pool=pp, stride=10, lut0=p, lut1=p,
             d_axes=p, h_axes=axes, g=geom, gaze=p, rb=rho, cap=0):
        return lib.fvvdp_gaze_grad_frames(64, 48, n_bands, n, G, cap, ctypes.byref(prm), ctypes.byref(pool), ctypes.byref(g),
                                          rb.ctypes.data_as(dp) if rb is not None else None, lut0, lut1, d_axes,
                                          nat.fptr(h_axes) if h_axes is not None else None, gaze, stride, p, n_frames, f0, p, mp,
                                          p, ctypes.c_void_p(work_ptr), work, None)

    assert lib.fvvdp_gaze_grad_frames(64, 48, 4, 2, 3, 0, None, None, None, None, None, None, None, None, None, 10, None, 5, 0,
                                      None, None, None, None, 0, None) == -1
    assert b"null" in lib.fvvdp_last_error()
    assert call(gaze=None) == -1 and b"null" in lib.fvvdp_last_error()
    assert call(rb=None) == -1 and b"null" in lib.fvvdp_last_error()
    for kw in ({"lut0": None}, {"lut1": None}, {"d_axes": None}, {"h_axes": None}):
        assert call(**kw) == -1 and b"null CSF table" in lib.fvvdp_last_error(), kw
    assert call(G=0) == -1 and b"n_gazes" in lib.fvvdp_last_error()
    assert call(G=-3) == -1 and b"n_gazes" in lib.fvvdp_last_error()
    for cap in (3, 5, 16, -1):
        assert call(cap=cap) == -1 and b"group_max" in lib.fvvdp_last_error(), cap
    assert call(n_bands=17) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert call(n_bands=0) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert call(n=0) == -1
    assert call(stride=3) == -1 and b"gaze_stride" in lib.fvvdp_last_error()
    assert call(f0=4) == -1 and b"outside the clip" in lib.fvvdp_last_error()
    assert call(f0=-1) == -1
    assert call(n_frames=1) == -1
    assert call(work=16) == -1 and b"workspace" in lib.fvvdp_last_error()
    assert call(work_ptr=260) == -1 and b"aligned" in lib.fvvdp_last_error()
    assert call(pool=nat.PoolParams(1, 0.67, 0, 0.25, -0.016, 0.6)) == -1 and b"exponents" in lib.fvvdp_last_error()
    holes = (nat.BandMaps * 4)()
    for b in range(4):
        holes[b].d_D = holes[b].d_contrast = holes[b].d_S = 256
    assert call(mp=holes) == -1 and b"every map" in lib.fvvdp_last_error()
    flat = nat.Geom()
    flat.display_size_m[0], flat.display_size_m[1], flat.distance_m, flat.ppd_centre = 0.66, 0.37, 0.0, 60.0
    assert call(g=flat) == -1 and b"geometry" in lib.fvvdp_last_error()
    assert call(h_axes=axes[:, ::-1].copy()) == -1 and b"ascending" in lib.fvvdp_last_error()
    # the workspace of G gazes is needed, not that of one
    need, one = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.fvvdp_gaze_grad_workspace(64, 48, 4, 2, 3, ctypes.byref(need)) == 0
    assert lib.fvvdp_video_grad_workspace(64, 48, 4, 2, ctypes.byref(one)) == 0
    assert call(work=one.value) == -1 and b"workspace" in lib.fvvdp_last_error()
    assert call(work=need.value - 1) == -1 and b"workspace" in lib.fvvdp_last_error()


def test_gaze_layer_kernels_exist_and_do_not_spill():
    import codeobj
    nat.build()
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    names = list(md)
    nice = codeobj.demangle(names)
    found = {k: 0 for k in KERNELS}
    for m, n in zip(names, nice):
        base = n.split("(")[0]
        if base in found:
            found[base] += 1
            x = md[m]
            assert (x["sgpr_spill_count"], x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), n
            print(base, "VGPRs", x["vgpr_count"], "SGPRs", x["sgpr_count"])
    assert found == {k: 1 for k in KERNELS}
    # the kernels the new unit launches through the video backward's unit are still defined once
    for k in ("video_coef_kernel", "video_layer_kernel", "video_level0_kernel", "adj_sweep_kernel"):
        assert sum(1 for n in nice if n.split("(")[0] == k) == 1, k


def test_s_query_restatement_against_the_oracle_interpolation():
    """gaze_layer_kernel takes the interval of a query from the uniform grid and the fraction from the stored knots; the
    reference bucketizes (interp.py:11-20).  Both describe the same piecewise-linear function up to the + 1e-6 in the
    fraction's denominator: per axis the fraction moves by at most 1e-6 / step, and the trilinear blend by that times the
    largest difference of neighbouring table entries along the axis.  float64 on both sides, so nothing else enters."""
    from oracle import fvvdp_oracle as orc
    m = fv.fvvdp(display_name="standard_4k", foveated=True, device="cpu", quiet=True)
    rng = np.random.default_rng(5)
    for cc in range(2):
        lut = m.csf_lut[cc]
        S = np.asarray(lut["S_log"], np.float64)
        ax = [np.asarray(lut[k], np.float64).ravel() for k in ("Y_log", "rho_log", "ecc_sqrt")]
        steps = [float(np.diff(a).min()) for a in ax]
        dmax = [float(np.abs(np.diff(S, axis=i)).max()) for i in range(3)]
        tol = 2.0 * sum(d * 1e-6 / s for d, s in zip(dmax, steps))
        n = 4000
        rho = 2.0 ** rng.uniform(-6, 8, n)                  # beyond both ends of rho_log (-4 .. 6)
        Y = 2.0 ** rng.uniform(-12, 15, n)                  # ... of Y_log
        ecc = rng.uniform(0, 150, n)                        # ... of ecc (0 .. 120)
        # exact knots on every axis, first and last included
        rho[:32], Y[32:64], ecc[64:96] = 2.0 ** ax[1], 2.0 ** ax[0], ax[2] ** 2
        rho[96:128], Y[96:128], ecc[96:128] = 2.0 ** ax[1], 2.0 ** ax[0][::-1], ax[2] ** 2
        ecc[128:140] = 0.0
        got = s_query(lut, rho, Y, ecc)
        want = np.log2(orc.cached_sensitivity({k: np.asarray(v, np.float64) for k, v in lut.items()}, rho, Y, ecc,
                                              dtype=np.float64))
        err = float(np.abs(got - want).max())
        print("cc %d: max |S_log - oracle| = %.3e, bound %.3e" % (cc, err, tol))
        assert np.isfinite(got).all() and err <= tol


def test_jod_gazes_refusals_without_device():
    x = torch.rand((1, 3, 4, 32, 48))
    r = torch.rand((1, 3, 4, 32, 48))
    gz = np.float32([[3, 4], [20, 10]])
    with pytest.raises(RuntimeError, match="needs a foveated metric"):
        fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True).jod_gazes(x, r, gz, frames_per_second=30)
    with pytest.raises(RuntimeError, match="makes no heat maps"):
        fv.fvvdp(display_name="standard_4k", foveated=True, heatmap="threshold", device="cpu",
                 quiet=True).jod_gazes(x, r, gz, frames_per_second=30)
    m = fv.fvvdp(display_name="standard_4k", foveated=True, device="cpu", quiet=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.jod_gazes(x.clone().requires_grad_(True), r, gz, frames_per_second=30)
    with pytest.raises(RuntimeError, match="gradients with respect to the reference are not supported"):
        m.jod_gazes(x, r.clone().requires_grad_(True), gz, frames_per_second=30)
    with pytest.raises(RuntimeError, match="at least 2 frames"):
        m.jod_gazes(x[:, :, :1], r[:, :, :1], gz, frames_per_second=30)
    with pytest.raises(RuntimeError, match="B must be 1"):
        m.jod_gazes(torch.rand((2, 3, 4, 32, 48)), torch.rand((2, 3, 4, 32, 48)), gz, frames_per_second=30)
    with pytest.raises(RuntimeError, match="float32"):
        m.jod_gazes((x * 255).to(torch.uint8), (r * 255).to(torch.uint8), gz, frames_per_second=30)
    with pytest.raises(RuntimeError, match="frames_per_second"):
        m.jod_gazes(x, r, gz)
    with pytest.raises(RuntimeError, match="frame rate too high"):
        m.jod_gazes(x, r, gz, frames_per_second=300)
    with pytest.raises(RuntimeError, match="colour channels"):
        m.jod_gazes(x[:, :2], r[:, :2], gz, frames_per_second=30)
    with pytest.raises(RuntimeError, match="same shape"):
        m.jod_gazes(x, r[..., :40], gz, frames_per_second=30)
    for bad in (np.zeros((2, 3), np.float32), np.zeros((2, 5, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros(2, np.float32)):
        with pytest.raises(RuntimeError, match="fixation_points must be"):
            m.jod_gazes(x, r, bad, frames_per_second=30)
