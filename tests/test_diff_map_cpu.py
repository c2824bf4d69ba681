"""Differentiable difference maps without a GPU: the header and its binding, the argument checks of its entry points, every
refusal that comes before any device work, the float64 restatement's adjoint against torch autograd of its own forward, and the
golden cases: inputs and cotangents rebuild from their seeds, the goldens load, and the pixels the units="jod" comparison leaves
out stay within their cap."""
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
import map_grad_cases as mc                 # noqa: E402
import map_grad_ref as ref                  # noqa: E402

# both sides float64 and analytic: relative to the largest entry of the level
ADJOINT_BOUND = 1e-12


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def test_diffmap_header_is_exported_and_bound():
    nat.build()
    names = declared("fvvdp_hip_diffmap.h")
    assert names == ["fvvdp_diffmap_grad_levels", "fvvdp_diffmap_grad_workspace", "fvvdp_diffmap_images_grad",
                     "fvvdp_diffmap_video_grad_frames", "fvvdp_heatmap_reconstruct_linear"]
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert sorted(nat.DIFFMAP_SYMBOLS) == names
    lib = nat.lib()
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    hdr = open(os.path.join(ROOT, "include", "fvvdp_hip_diffmap.h")).read()
    assert "#define FVVDP_DIFFMAP_JOD %d\n" % nat.DIFFMAP_JOD in hdr and "#define FVVDP_DIFFMAP_LINEAR %d\n" % nat.DIFFMAP_LINEAR in hdr
    assert callable(fv.fvvdp.diff_map_images) and callable(fv.fvvdp.diff_map_video)
    from fovvideovdp_amd import map_grad
    assert map_grad.UNITS == {"jod": 0, "linear": 1}


def test_argument_checks_need_no_device():
    lib = nat.lib()
    W, H, nb, n = 121, 67, 4, 3
    nbytes, jbytes, vbytes = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    gl, a = (ctypes.c_size_t * nb)(), (ctypes.c_size_t * nb)()
    assert lib.fvvdp_diffmap_grad_workspace(W, H, nb, n, 1, None, None, None) == -1 and b"null" in lib.fvvdp_last_error()
    assert lib.fvvdp_diffmap_grad_workspace(W, H, nb, n, 3, None, None, ctypes.byref(nbytes)) == -1
    assert b"channels must be 1" in lib.fvvdp_last_error()
    assert lib.fvvdp_diffmap_grad_workspace(W, H, 0, n, 1, None, None, ctypes.byref(nbytes)) == -1 and b"bad shape" in lib.fvvdp_last_error()
    # the JOD backward's workspace, then A_b [n][h_b][w_b], every part rounded up to 64 floats
    sizes = ref.level_sizes(W, H, nb)
    chain = sum((n * w * h + 63) // 64 * 64 for w, h in sizes) * 4
    assert lib.fvvdp_images_grad_workspace(W, H, nb, n, ctypes.byref(jbytes)) == 0
    assert lib.fvvdp_video_grad_workspace(W, H, nb, n, ctypes.byref(vbytes)) == 0
    for channels, base in ((1, jbytes.value), (2, vbytes.value)):
        assert lib.fvvdp_diffmap_grad_workspace(W, H, nb, n, channels, gl, a, ctypes.byref(nbytes)) == 0
        assert nbytes.value == base + chain
        assert a[0] * 4 == base and list(a) == sorted(a) and list(gl) == sorted(gl) and gl[nb - 1] < a[0]
        assert all(x % 64 == 0 for x in list(gl) + list(a))

    prm, pp = nat.Params(), nat.PoolParams()
    pp.beta_jod, pp.jod_a, pp.w_transient, prm.beta = 0.5, -0.25, 0.25, 1.0
    maps = (nat.BandMaps * nb)(*[nat.BandMaps(256, 256, 256, 256) for _ in range(nb)])
    p = ctypes.c_void_p
    big = 1 << 30

    def levels(channels=1, units=0, G=0x1000, v0=0x2000, work=0x4000, work_bytes=big, maps=maps, pp=pp):
        return lib.fvvdp_diffmap_grad_levels(W, H, nb, n, channels, ctypes.byref(prm), ctypes.byref(pp), units, p(G), p(v0), maps,
                                             p(work), work_bytes, None)

    assert levels(G=None) == -1 and b"null" in lib.fvvdp_last_error()
    assert levels(work=None) == -1 and b"null" in lib.fvvdp_last_error()
    assert levels(units=2) == -1 and b"units must be" in lib.fvvdp_last_error()
    assert levels(v0=None) == -1 and b"need d_v0" in lib.fvvdp_last_error()
    assert levels(channels=0) == -1 and b"channels must be 1" in lib.fvvdp_last_error()
    assert levels(G=0x1002) == -1 and b"aligned to 4 bytes" in lib.fvvdp_last_error()
    assert levels(work=0x4010) == -1 and b"256-byte aligned" in lib.fvvdp_last_error()
    assert levels(work_bytes=nbytes.value - 1, channels=2) == -1 and b"workspace of" in lib.fvvdp_last_error()
    holes = (nat.BandMaps * nb)(*[nat.BandMaps(256, 256, 256, 0) for _ in range(nb)])
    assert levels(maps=holes) == -1 and b"every map" in lib.fvvdp_last_error()
    bad = nat.PoolParams()
    bad.beta_jod, bad.jod_a, bad.w_transient = 0.0, -0.25, 0.25
    assert levels(pp=bad) == -1 and b"exponents must be positive" in lib.fvvdp_last_error()

    e = nat.Eotf()
    e.kind = nat.EOTF_SRGB
    one = (ctypes.c_void_p * n)(*([258] * n))                          # 2-byte aligned, not 4
    w = np.ones(3, dtype=np.float32)

    def img(dtype=nat.FVVDP_F32, C=3, e=e):
        return lib.fvvdp_diffmap_images_grad(W, H, nb, n, ctypes.byref(prm), ctypes.byref(pp), 0, p(0x1000), p(0x2000), maps, one,
                                             dtype, C, W * H, ctypes.byref(e), nat.fptr(w), one, p(0x4000), big, None)

    assert img(dtype=nat.FVVDP_U8) == -1 and b"float32, float16 and bfloat16" in lib.fvvdp_last_error()
    assert img(C=2) == -1 and b"1 or 3 colour channels" in lib.fvvdp_last_error()
    assert img() == -1 and b"aligned to 4 bytes" in lib.fvvdp_last_error()
    lut = nat.Eotf()
    lut.kind = nat.EOTF_LUT
    assert img(dtype=nat.FVVDP_F16, e=lut) == -1 and b"closed-form" in lib.fvvdp_last_error()

    def vid(n_frames=9, f0=0, g0=0x8000):
        return lib.fvvdp_diffmap_video_grad_frames(W, H, nb, n, ctypes.byref(prm), ctypes.byref(pp), 1, p(0x1000), None, n_frames, f0,
                                                   maps, p(g0), p(0x4000), big, None)

    assert vid(g0=None) == -1 and b"null" in lib.fvvdp_last_error()
    assert vid(f0=7) == -1 and b"outside the clip" in lib.fvvdp_last_error()
    assert vid(g0=0x8002) == -1 and b"d_g0 must be aligned" in lib.fvvdp_last_error()
    assert lib.fvvdp_heatmap_reconstruct_linear(None, 1, None, 0.25, None, None) == -1 and b"null" in lib.fvvdp_last_error()


def test_refusals_without_device():
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True, heatmap="raw")       # whatever `heatmap`
    x, r = torch.rand((1, 3, 32, 48)), torch.rand((1, 3, 32, 48))
    v, rv = torch.rand((1, 3, 4, 32, 48)), torch.rand((1, 3, 4, 32, 48))
    for units in ("JOD", "log", None):
        with pytest.raises(ValueError, match='units must be "jod" or "linear"'):
            m.diff_map_images(x, r, units=units)
        with pytest.raises(ValueError, match='units must be "jod" or "linear"'):
            m.diff_map_video(v, rv, frames_per_second=30, units=units)
    with pytest.raises(RuntimeError, match="diff_map_images differentiates the map with respect to the test only.*detach the reference"):
        m.diff_map_images(x.clone().requires_grad_(True), r.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="diff_map_video differentiates the map with respect to the test only.*detach the reference"):
        m.diff_map_video(v, rv.clone().requires_grad_(True), frames_per_second=30)
    for bad in (torch.float64, torch.uint8, torch.int16):
        with pytest.raises(RuntimeError, match="diff_map_images needs float32, float16 or bfloat16 test and reference images"):
            m.diff_map_images((x * 255).to(bad).requires_grad_(bad is torch.float64), (r * 255).to(bad))
        with pytest.raises(RuntimeError, match="diff_map_video needs float32, float16 or bfloat16 test and reference clips"):
            m.diff_map_video((v * 255).to(bad), (rv * 255).to(bad), frames_per_second=30)
    with pytest.raises(RuntimeError, match="diff_map_video: frame rate too high for the backward: its temporal filter has 65 taps"):
        m.diff_map_video(v.requires_grad_(True), rv, frames_per_second=260)
    with pytest.raises(RuntimeError, match="diff_map_video needs a clip"):
        m.diff_map_video(x, r, dim_order="BCHW", frames_per_second=30)
    with pytest.raises(RuntimeError, match="F axis"):
        m.diff_map_images(v, rv, dim_order="BCFHW")
    # everything accepted: the first device work is refused on a CPU metric
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.diff_map_images(x.clone().requires_grad_(True), r, units="linear")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.diff_map_video(v.half(), rv, frames_per_second=30)


def test_refuses_user_photometry():
    class MyDisplay(fv.fvvdp_display_photometry):
        def forward(self, V):
            return 100.0 * V + 0.5

        def get_peak_luminance(self):
            return 100.5

        def get_black_level(self):
            return 0.5

    m = fv.fvvdp(display_name="standard_4k", display_photometry=MyDisplay(), device="cpu", quiet=True)
    with pytest.raises(RuntimeError, match="diff_map_images needs a display model with a closed form"):
        m.diff_map_images(torch.rand((1, 3, 32, 48)), torch.rand((1, 3, 32, 48)))
    with pytest.raises(RuntimeError, match="diff_map_video needs a display model with a closed form"):
        m.diff_map_video(torch.rand((1, 3, 4, 32, 48)), torch.rand((1, 3, 4, 32, 48)), frames_per_second=30)


def test_expand_matrix_is_the_oracles_expand():
    from oracle import fvvdp_oracle as orc
    rng = np.random.default_rng(5)
    for h, w in ((5, 7), (68, 121), (2, 3), (1, 1)):
        hc, wc = (h + 1) // 2, (w + 1) // 2
        x = rng.standard_normal((hc, wc))
        want = orc.gausspyr_expand(x, (h, w), dtype=np.float64)
        got = ref.expand(torch.from_numpy(x), h, w).numpy()
        assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max()


@pytest.mark.parametrize("W,H,n_bands", [(7, 5, 3), (121, 68, 5), (3, 2, 2)])
@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("units", mc.UNITS)
def test_adjoint_is_the_autograd_of_the_restated_forward(W, H, n_bands, nc, units):
    """5x7, 68x121 and 2x3: both parities, a one-pixel coarse level and the coarsest band (which has no coarse term)."""
    k = ref.constants()
    n = 2
    layers, maps = ref.synthetic_maps(W, H, n_bands, n, nc, k, seed=W * H + nc)
    layers = [x.requires_grad_(True) for x in layers]
    ref.forward_maps(layers, maps, k, nc)
    vs = []
    v0 = ref.reconstruct([mp["D"] for mp in maps], k, nc, keep=vs)
    for v in vs:
        v.retain_grad()
    assert bool((v0 > 0).all())
    G = torch.rand((n, H, W), generator=torch.Generator().manual_seed(3), dtype=torch.float64) + 0.25
    (G * ref.diff_map(v0, k, units)).sum().backward()
    stored = [{key: val.detach() for key, val in mp.items()} for mp in maps]
    A, GL = ref.adjoint(G, v0.detach(), stored, k, units, nc)
    planted = 0
    for b in range(n_bands):
        assert float((A[b] - vs[b].grad).abs().max()) <= ADJOINT_BOUND * float(vs[b].grad.abs().max()), b
        want = layers[b].grad
        assert float((GL[b] - want).abs().max()) <= ADJOINT_BOUND * float(want.abs().max()), b
        flat = GL[b].reshape(n, nc, -1)
        npx = flat.shape[-1]
        assert bool((flat[:, :, :min(3, npx)] == 0).all())                # D == 0, the d_max clamp, the contrast clamp
        planted += int(npx > 3 and bool((flat[:, :, 3] != 0).all()))      # |T'| == |R'|: the split tie is not a zero
        assert bool((GL[b] != 0).any()) or npx <= 3
    assert planted >= 1 or W * H < 8


def test_identical_pair_has_a_zero_finite_adjoint():
    k = ref.constants()
    layers, maps = ref.synthetic_maps(7, 5, 2, 1, 2, k, seed=1, plant=False)
    g = torch.Generator().manual_seed(2)
    for b, mp in enumerate(maps):                                         # T == R everywhere (powers of two: exactly)
        a = 2.0 ** -torch.randint(2, 7, mp["ref"].shape, generator=g).double() * (torch.randint(0, 2, mp["ref"].shape, generator=g) * 2 - 1)
        mp["ref"] = a * (1.0 if b == 0 else 2.0)
        layers[b] = a * mp["lbkg"][:, None]
    ref.forward_maps(layers, maps, k, 2)
    v0 = ref.reconstruct([mp["D"] for mp in maps], k, 2)
    assert bool((v0 == 0).all())
    for units in mc.UNITS:
        A, GL = ref.adjoint(torch.ones_like(v0), v0, maps, k, units, 2)
        assert all(bool(torch.isfinite(x).all()) for x in A + GL) and all(bool((x == 0).all()) for x in GL)


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_golden_cases_rebuild_and_load(name):
    C, N, H, W, fps, padding, display, opt = mc.CASES[name]
    t, r = mc.case_inputs(name)
    t2, _ = mc.case_inputs(name)
    assert t.shape == r.shape == (C, N, H, W) and t.dtype == np.float32 and np.array_equal(t, t2)
    Wt = mc.case_weights(name)
    assert Wt.shape == (N, H, W) and Wt.dtype == np.float32 and Wt.min() >= 0.25 and np.array_equal(Wt, mc.case_weights(name))
    path = os.path.join(mc.GOLDEN, mc.golden_file(name))
    assert os.path.getsize(path) < 1 << 20
    g = mc.load_golden(name)
    assert g["map_jod"].shape == g["map_linear"].shape == (N, H, W)
    assert g["grad_jod"].shape == g["grad_linear"].shape == (C, N, H, W)
    assert all(np.isfinite(v).all() for v in g.values())
    assert (g["map_linear"] > 0).all() and (g["map_jod"] > 0).all()          # the tool asserts v > 0: the reference is finite
    # the JOD-unit map is the linear one through the power (both rounded to 16 significant bits)
    m = fv.fvvdp(display_name=display, device="cpu", quiet=True)
    k = ref.constants(m)
    again = ref.diff_map(torch.from_numpy(g["map_linear"]).double(), k, "jod").numpy()
    assert np.abs(again - g["map_jod"]).max() <= 4e-5 * g["map_jod"].max()
    # the pixels the units="jod" gradient comparison leaves out
    share = float((g["map_jod"] < mc.map_floor(name)).mean())
    print("%s: %.4f %% of the pixels below the floor %g" % (name, 100 * share, mc.map_floor(name)))
    assert share <= mc.MAX_EXCLUDED
    if opt.get("oob"):
        oob = (t < 0) | (t > 1)
        assert oob.any() and (g["grad_jod"][oob] == 0).all() and (g["grad_linear"][oob] == 0).all()
