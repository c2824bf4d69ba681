"""Gradients with respect to the model parameters without a GPU: the header and its binding, the argument checks of its entry
points, the code objects of the new kernels, the chain of param_grad.py against central differences of the float64 oracle, the
refusals that come before any device work, and the metric's attributes staying as they were."""
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
import param_grad_ref as ref               # noqa: E402

# Both sides are float64: the chain on sums made from the oracle's capture, and central differences of the oracle with a step
# of 1e-5 max(|theta|, 1), whose truncation and cancellation errors are of the order 1e-9 relative.  Relative to the sum of the
# absolute per-(band, channel, frame) terms of each entry.
CHAIN_BOUND = 1e-6


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def test_params_header_is_exported_and_bound():
    nat.build()
    names = declared("fvvdp_hip_params.h")
    assert names == ["fvvdp_ctx_set_params", "fvvdp_param_sums", "fvvdp_param_sums_workspace"]
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert sorted(nat.PARAM_SYMBOLS) == names
    others = set(nat.SYMBOLS) | set(nat.IMAGE_SYMBOLS) | set(nat.GRAD_SYMBOLS) | set(nat.VIDEO_GRAD_SYMBOLS) | \
        set(nat.GAZE_SYMBOLS) | set(nat.GAZE_GRAD_SYMBOLS) | set(nat.REF_GRAD_SYMBOLS)
    assert not set(names) & others
    assert len(declared("fvvdp_hip.h")) == 24
    lib = nat.lib()
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    assert nat.PARAM_SUMS == 5


def test_argument_checks_need_no_device():
    lib = nat.lib()
    prm = fv.fvvdp(device="cpu", quiet=True).native_params()
    assert lib.fvvdp_ctx_set_params(None, ctypes.byref(prm)) == -1 and b"null" in lib.fvvdp_last_error()
    nbytes = ctypes.c_size_t(0)
    assert lib.fvvdp_param_sums_workspace(64, 48, 4, 3, None) == -1
    assert lib.fvvdp_param_sums_workspace(64, 48, 17, 3, ctypes.byref(nbytes)) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert lib.fvvdp_param_sums_workspace(64, 48, 4, 0, ctypes.byref(nbytes)) == -1
    assert lib.fvvdp_param_sums_workspace(64, 48, 4, 65536, ctypes.byref(nbytes)) == -1
    # partial [blocks][n][2][5] fp64, one block per 4096 band pixels: 64x48, 32x24, 16x12, 8x6 -> 1 block each
    assert lib.fvvdp_param_sums_workspace(64, 48, 4, 3, ctypes.byref(nbytes)) == 0 and nbytes.value == 4 * 3 * 2 * 5 * 8
    assert lib.fvvdp_param_sums_workspace(240, 135, 2, 1, ctypes.byref(nbytes)) == 0 and nbytes.value == (8 + 2) * 2 * 5 * 8

    maps = (nat.BandMaps * 4)()
    for b in range(4):
        maps[b].d_D = maps[b].d_contrast = maps[b].d_lbkg = maps[b].d_S = 256
    p = ctypes.c_void_p(256)

    def sums(n_bands=4, n=2, planes=4, prm_=prm, maps_=maps, out=p, work=p, work_bytes=1 << 20):
        return lib.fvvdp_param_sums(64, 48, n_bands, n, planes, ctypes.byref(prm_) if prm_ is not None else None, maps_, out, work,
                                    work_bytes, None)

    assert sums(prm_=None) == -1 and b"null" in lib.fvvdp_last_error()
    assert sums(maps_=None) == -1 and sums(out=None) == -1 and sums(work=None) == -1
    assert sums(planes=3) == -1 and b"planes" in lib.fvvdp_last_error()
    assert sums(n_bands=17) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert sums(n=0) == -1
    assert sums(work_bytes=16) == -1 and b"workspace" in lib.fvvdp_last_error()
    assert sums(work=ctypes.c_void_p(264)) == -1 and b"aligned" in lib.fvvdp_last_error()
    assert sums(out=ctypes.c_void_p(260)) == -1 and b"8 bytes" in lib.fvvdp_last_error()
    holes = (nat.BandMaps * 4)()
    for b in range(4):
        holes[b].d_D = holes[b].d_contrast = holes[b].d_S = 256
    holes[2].d_S = None
    assert sums(maps_=holes) == -1 and b"band 2" in lib.fvvdp_last_error()
    bad = fv.fvvdp(device="cpu", quiet=True).native_params()
    bad.beta = 0.0
    assert sums(prm_=bad) == -1 and b"positive" in lib.fvvdp_last_error()
    bad.beta, bad.mask_q[1] = 0.9, float("nan")
    assert sums(prm_=bad) == -1 and b"positive" in lib.fvvdp_last_error()


def test_new_kernels_do_not_spill():
    import codeobj
    nat.build()
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    names = list(md)
    nice = codeobj.demangle(names)
    found = {"void param_sums_kernel<2>": 0, "void param_sums_kernel<4>": 0, "param_finalize_kernel": 0}
    for m, n in zip(names, nice):
        base = n.split("(")[0]
        if base in found:
            found[base] += 1
            x = md[m]
            assert (x["sgpr_spill_count"], x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), (n, x)
            assert x["vgpr_count"] <= 128, (n, x)          # four waves per SIMD at least: a streaming kernel
    assert found == {k: 1 for k in found}


@pytest.mark.parametrize("name", ref.CPU_CASES)
def test_chain_matches_central_differences_of_the_float64_oracle(name):
    from fovvideovdp_amd import param_grad as pg
    assert tuple(fv.fvvdp.PARAMETER_NAMES) == ref.NAMES == tuple(pg.PARAMETER_NAMES)
    c = ref.oracle_case(name)
    assert c["clamped"] == 0                      # a pixel that crosses the d_max clamp inside the step breaks the differences
    per_column = c["channels"] == 1
    J, scale = pg.chain(torch.from_numpy(c["Q"]), torch.from_numpy(c["sums"]), torch.from_numpy(c["npx"]), list(ref.theta0()),
                        c["channels"], per_column, with_scale=True)
    assert J.shape == (1, 12) and J.dtype == torch.float64
    J, scale = J[0].numpy(), scale[0].numpy()
    fd = ref.central_differences(name)
    acts = np.ones(12, bool)
    if per_column:                                # a still image: no transient channel, no pooling over channels or frames
        for n in ("mask_q_trans", "w_transient", "beta_t", "beta_tch"):
            acts[ref.NAMES.index(n)] = False
    worst = 0.0
    for i, n in enumerate(ref.NAMES):
        if not acts[i]:
            assert J[i] == 0.0 and abs(fd[i]) < 1e-9, (n, J[i], fd[i])
            continue
        err = abs(J[i] - fd[i]) / scale[i]
        worst = max(worst, err)
        print("%-16s %-24s chain % .9e  differences % .9e  rel %.2e" % (name, n, J[i], fd[i], err))
        assert scale[i] > 0 and err < CHAIN_BOUND, (n, J[i], fd[i], scale[i])
    print("worst", worst)


def test_chain_gives_finite_zeros_for_zero_columns():
    """An identical pair (every Q zero), a clip whose transient channel is zero, and beta_tch < 1 (0^(beta - 1) 0)."""
    from fovvideovdp_amd import param_grad as pg
    nb, F = 4, 3
    th = list(ref.theta0())
    npx = torch.tensor([100.0, 25.0, 9.0, 4.0], dtype=torch.float64)
    zeros_q, zeros_s = torch.zeros((nb, 2, F), dtype=torch.float64), torch.zeros((nb, 2, F, 5), dtype=torch.float64)
    for per_column, ch in ((True, 1), (False, 2)):
        J = pg.chain(zeros_q, zeros_s, npx, th, ch, per_column)
        assert J.shape == ((F if per_column else 1), 12) and (J == 0).all()
    Q = torch.rand((nb, 2, F), dtype=torch.float64) + 0.5
    Q[:, 1] = 0                                    # a static clip: nothing in the transient channel
    Q[:, :, 1] = 0                                 # ... and one frame identical
    s = torch.rand((nb, 2, F, 5), dtype=torch.float64) * (Q > 0)[..., None]
    J = pg.chain(Q, s, npx, th, 2, False)
    assert torch.isfinite(J).all() and (J[0, :6] != 0).sum() >= 4
    assert J[0, ref.NAMES.index("mask_q_trans")] == 0 and J[0, ref.NAMES.index("w_transient")] == 0


def test_parameter_vector_round_trip_and_refusals():
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    th = m.parameter_tensor()
    assert th.dtype == torch.float64 and th.device.type == "cpu" and th.shape == (12,)
    assert [float(v) for v in th] == [float(getattr(m, n)) for n in fv.fvvdp.PARAMETER_NAMES]
    assert np.array_equal(th.numpy(), ref.theta0())
    before = dict(vars(m))
    x, r = torch.rand((2, 3, 32, 48)), torch.rand((2, 3, 32, 48))
    clip_x, clip_r = torch.rand((1, 3, 4, 32, 48)), torch.rand((1, 3, 4, 32, 48))

    def images(theta, a=x, b=r, metric=m):
        return metric.calibration_jod_images(a, b, theta)

    def video(theta, a=clip_x, b=clip_r, metric=m):
        return metric.calibration_jod_video(a, b, theta, frames_per_second=30)

    def unchanged():
        now = vars(m)
        return all(now[k] is before[k] or now[k] == before[k] for k in fv.fvvdp.PARAMETER_NAMES) and m._ctx is None

    for call in (images, video):
        with pytest.raises(RuntimeError, match="1-D vector of the 12 parameters"):
            call(th[:11])
        with pytest.raises(RuntimeError, match="1-D vector"):
            call(th.view(3, 4))
        bad = th.clone()
        bad[3] = float("nan")
        with pytest.raises(RuntimeError, match="non-finite.*mask_c"):
            call(bad)
        bad = th.clone()
        bad[10] = float("inf")
        with pytest.raises(RuntimeError, match="non-finite.*jod_a"):
            call(bad)
        for n in ("beta", "beta_sch", "beta_tch", "beta_t", "mask_p"):
            for v in (0.0, -1.0):
                bad = th.clone()
                bad[fv.fvvdp.PARAMETER_NAMES.index(n)] = v
                with pytest.raises(RuntimeError, match="%s must be positive" % n):
                    call(bad)
        bad = th.clone()
        bad[10] = 0.0
        with pytest.raises(RuntimeError, match="jod_a must not be 0"):
            call(bad)
        assert unchanged()
    xg = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="model parameters only.*jod_images"):
        images(th, a=xg)
    with pytest.raises(RuntimeError, match="model parameters only.*jod_images"):
        images(th, b=xg)
    cg = clip_x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="model parameters only.*jod_video"):
        video(th, a=cg)
    with pytest.raises(RuntimeError, match="B must be 1"):
        video(th, a=torch.rand((2, 3, 4, 32, 48)), b=torch.rand((2, 3, 4, 32, 48)))
    hm = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True, heatmap="raw")
    for call in (images, video):
        with pytest.raises(RuntimeError, match="no heat maps"):
            call(th, metric=hm)
        # accepted: the next refusal is the missing device, for float32 and float64 vectors, with and without grad
        for theta in (th, th.float(), th.clone().requires_grad_(True)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call(theta)
    assert unchanged()

    # set_parameters writes the attributes, as Python floats, and checks the vector the same way
    new = th.clone()
    new[3] -= 0.1
    new[4] += 0.5
    m.set_parameters(new.float())
    assert m.mask_c == float(new.float()[3]) and m.sensitivity_correction == float(new.float()[4]) and isinstance(m.mask_c, float)
    assert torch.equal(m.parameter_tensor(), new.float().double())
    with pytest.raises(RuntimeError, match="1-D vector"):
        m.set_parameters(th[:5])
    m.set_parameters(th)
    assert torch.equal(m.parameter_tensor(), th)


def test_theta_constants_are_converted_as_the_metric_converts_its_attributes():
    """The forward under theta is bit-identical to a metric whose attributes hold theta only if the fp32 constants are."""
    from fovvideovdp_amd import param_grad as pg
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    rng = np.random.default_rng(5)
    for trial in range(4):
        th = m.parameter_tensor() if trial == 0 else ref_theta(rng)
        other = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
        other.set_parameters(th)
        a, b = pg.native_params_of(pg.theta_values(th)), other.native_params()
        assert bytes(a) == bytes(b)
        a, b = pg.pool_params_of(pg.theta_values(th)), other._pool_params()
        assert bytes(a) == bytes(b)


def ref_theta(rng):
    th = torch.from_numpy(ref.theta0() * (1.0 + 0.05 * rng.standard_normal(12)))
    return th.float() if rng.random() < 0.5 else th
