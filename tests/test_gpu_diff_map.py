"""fvvdp.diff_map_images / diff_map_video on the GPU: the map against the heatmap="raw" output of predict_images / predict bit for
bit, map_level_kernel per pixel against the float64 restatement (tests/map_grad_ref.py) through the C ABI, map and gradient
against the reference's autograd (goldens g23), the exact invariants, half precision, composition with torch's own ops and the
code objects of the new kernels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_grad_cases as mc                 # noqa: E402
import map_grad_ref as ref                  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# Against the reference's autograd of sum(W * map), per case, in the order (jod, linear), as measured on MI355X:
#   max|g - g_ref| / max|g_ref|      a 3.7e-5, 3.6e-5   b 1.8e-5, 1.9e-5   c 2.2e-4, 3.2e-4   d 2.2e-4, 2.6e-4
#                                    e 1.1e-5, 1.1e-5   f 1.7e-5, 1.3e-5   g 9.5e-6, 1.2e-5
#   max|map - map_ref| / max|map_ref| a 2.2e-5, 2.4e-5   b 1.2e-5, 1.4e-5   c 1.6e-4, 2.3e-4   d 5.4e-4, 7.2e-4
#                                    e 1.1e-5, 9.3e-6   f 1.9e-5, 1.9e-5   g 1.0e-5, 1.1e-5
# (the goldens are stored with 16 significant bits, 8e-6).  The bounds are 3x the measurement, as the files next to this one
# set theirs; every gradient bound stays below the loosest bound of the image gradients (1.6e-3, foveated), and no case needs
# a floor on the map for units="jod": all pixels are compared.
GOLDEN_TOL = {"a_gray_fhd": (1.2e-4, 1.1e-4), "b_rgb_4k_oob": (5.5e-5, 5.8e-5), "c_rgb_hdr_pq": (6.6e-4, 9.8e-4),
              "d_gray_foveated": (6.7e-4, 7.9e-4), "e_clip_replicate": (3.2e-5, 3.3e-5), "f_clip_circular": (5.0e-5, 4.1e-5),
              "g_clip_pingpong": (2.9e-5, 3.6e-5)}
MAP_TOL = {"a_gray_fhd": (6.6e-5, 7.2e-5), "b_rgb_4k_oob": (3.5e-5, 4.3e-5), "c_rgb_hdr_pq": (4.8e-4, 6.8e-4),
           "d_gray_foveated": (1.7e-3, 2.2e-3), "e_clip_replicate": (3.2e-5, 2.8e-5), "f_clip_circular": (5.9e-5, 5.7e-5),
           "g_clip_pingpong": (3.1e-5, 3.3e-5)}
# map_level_kernel against float64, per pixel.  A_b: a sum of up to 25 positive terms per level crossed, each rounded once
# (2^-24), after A_0's powf and two multiplications.  GL_b: the error of A_b, plus the log2 / exp2 form of the powers that
# video_layer_one has against adj_layer_kernel's powf -- three v_log_f32 / v_exp_f32 pairs of 1 ulp under an exponent of up to
# p |lg u| ~ 2.4 x 20, relative ln 2 x 48 x 2^-23 = 4e-6 each -- for which test_gpu_video_grad.py leaves 3.4e-5 (its tightest
# golden bound on a non-zero gradient, case k), relative to the terms the value is the difference of.
A_ULPS = 8
FAST_SLACK = 3.4e-5


def _metric(display, foveated=False, padding="replicate", heatmap=None):
    return fv.fvvdp(display_name=display, foveated=foveated, quiet=True, device=DEV, temp_padding=padding, heatmap=heatmap)


def _case(name):
    """metric keywords, test, reference as device tensors ([B, C, H, W] for a still, [C, N, H, W] for a clip), call keywords."""
    Cc, N, H, W, fps, padding, display, opt = mc.CASES[name]
    t, r = mc.case_inputs(name)
    kw = dict(fixation_point=opt["fix"]) if "fix" in opt else {}
    mk = dict(display=display, foveated=bool(opt.get("foveated")), padding=padding)
    if N == 1:
        return mk, torch.from_numpy(t[:, 0][None]).to(DEV), torch.from_numpy(r[:, 0][None]).to(DEV), kw
    kw.update(dim_order="CFHW", frames_per_second=fps)
    return mk, torch.from_numpy(t).to(DEV), torch.from_numpy(r).to(DEV), kw


def _map(m, name, T, R, kw, **more):
    fn = m.diff_map_images if mc.CASES[name][1] == 1 else m.diff_map_video
    return fn(T, R, **kw, **more)


def _heatmap(m_raw, name, T, R, kw):
    """The fp16 host heat maps [n, H, W] of predict_images / predict on a heatmap="raw" metric."""
    if mc.CASES[name][1] == 1:
        _, st = m_raw.predict_images(T, R, **kw)
        return st["heatmap"][:, 0, 0]
    _, st = m_raw.predict(T, R, **kw)
    return st["heatmap"][0, 0]


# ---- 1. the forward is the heat map ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_forward_is_the_raw_heatmap_bit_for_bit(name):
    mk, T, R, kw = _case(name)
    if name == "b_rgb_4k_oob":                                            # B = 3
        T = torch.cat([T, T.flip(-1), (1 - T).clamp(0, 1)])
        R = torch.cat([R, R.flip(-1), (1 - R).clamp(0, 1)])
    m_raw = _metric(heatmap="raw", **mk)
    want = _heatmap(m_raw, name, T, R, kw)
    m = _metric(**mk)
    got = _map(m, name, T, R, kw)
    assert got.dtype is torch.float32 and got.device == DEV and got.grad_fn is None and got.shape == want.shape
    assert torch.equal(got.to(torch.float16).cpu(), want)
    assert torch.equal(_map(m_raw, name, T, R, kw), got)                 # whatever `heatmap` the metric was built with
    is_clip = mc.CASES[name][1] > 1
    m.batch_frames = 4 if is_clip else 1                                 # several forward batches
    assert torch.equal(_map(m, name, T, R, kw), got)
    m.batch_frames = None
    if not is_clip and T.shape[0] == 3:
        for k in range(3):
            assert torch.equal(_map(m, name, T[k:k + 1], R[k:k + 1], kw)[0], got[k]), k
    # units="linear" is the same reconstruction without the power: the float64 restatement of the power maps one on the other
    lin = _map(m, name, T, R, kw, units="linear")
    k64 = ref.constants(m)
    again = ref.diff_map(lin.double().cpu(), k64, "jod")
    err = float(((again - got.double().cpu()).abs() / got.double().cpu().clamp_min(1e-30)).max())
    print("%s: map in [%.3e, %.3e], linear -> jod in float64 against the kernel's powf: rel %.2e" % (
        name, float(got.min()), float(got.max()), err))
    assert bool((lin > 0).all()) and err <= 4 * 2.0 ** -23


# ---- 2. map_level_kernel per pixel, through the C ABI -------------------------------------------------------------------------
def _f32(x):
    return x.to(torch.float32).to(DEV).contiguous()


@pytest.mark.parametrize("W,H,n_bands", [(7, 5, 3), (121, 68, 5), (259, 3, 3)])
@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("units", mc.UNITS)
def test_level_kernel_per_pixel(W, H, n_bands, nc, units):
    k = ref.constants(_metric("standard_4k"))
    n = 2
    layers, maps = ref.synthetic_maps(W, H, n_bands, n, nc, k, seed=W + H + nc)
    # what the kernel reads is fp32: the restatement works on exactly those values
    maps32 = []
    for b, mp in enumerate(maps):
        lay = layers[b].float().double()
        mp = dict(lbkg=mp["lbkg"].float().double(), S=mp["S"].float().double(), ref=mp["ref"].float().double())
        layers[b] = lay
        maps32.append(mp)
    ref.forward_maps(layers, maps32, k, nc)
    for mp in maps32:
        mp["contrast"] = mp["contrast"].float().double()
        mp["D"] = mp["D"].float().double()
    v0 = ref.reconstruct([mp["D"] for mp in maps32], k, nc).float().double()
    G = (torch.rand((n, H, W), generator=torch.Generator().manual_seed(9), dtype=torch.float64) + 0.25).float().double()
    terms = []
    A64, GL64 = ref.adjoint(G, v0, maps32, k, units, nc, terms)

    lib = nat.lib()
    dev = [dict(D=_f32(mp["D"]), contrast=_f32(mp["contrast"]), lbkg=_f32(mp["lbkg"]), S=_f32(mp["S"])) for mp in maps32]
    arr = (nat.BandMaps * n_bands)()
    for b, d in enumerate(dev):
        arr[b].d_D, arr[b].d_contrast, arr[b].d_lbkg, arr[b].d_S = (d["D"].data_ptr(), d["contrast"].data_ptr(), d["lbkg"].data_ptr(),
                                                                  d["S"].data_ptr())
    nbytes = C.c_size_t(0)
    gl_off, a_off = (C.c_size_t * n_bands)(), (C.c_size_t * n_bands)()
    nat.check(lib.fvvdp_diffmap_grad_workspace(W, H, n_bands, n, nc, gl_off, a_off, C.byref(nbytes)))
    work = torch.full((nbytes.value // 4,), float("nan"), dtype=torch.float32, device=DEV)
    Gd, vd = _f32(G), _f32(v0)
    m = _metric("standard_4k")
    prm, pp = m.native_params(), m._pool_params()
    with torch.cuda.device(DEV):
        stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        nat.check(lib.fvvdp_diffmap_grad_levels(W, H, n_bands, n, nc, C.byref(prm), C.byref(pp), nat.DIFFMAP_JOD if units == "jod"
                                                else nat.DIFFMAP_LINEAR, C.c_void_p(Gd.data_ptr()),
                                                C.c_void_p(vd.data_ptr()) if units == "jod" else None, arr,
                                                C.c_void_p(work.data_ptr()), nbytes.value, stream))
    torch.cuda.synchronize()
    host = work.double().cpu()
    nonzero = 0
    for b, (w, h) in enumerate(ref.level_sizes(W, H, n_bands)):
        A = host[a_off[b]:a_off[b] + n * h * w].view(n, h, w)
        GL = host[gl_off[b]:gl_off[b] + n * nc * h * w].view(n, nc, h, w)
        a_rel = (A_ULPS + 25 * b) * 2.0 ** -24
        ea = float(((A - A64[b]).abs() / A64[b]).max())
        bound = (a_rel + 25 * 2.0 ** -24 + FAST_SLACK) * terms[b]
        eg = (GL - GL64[b]).abs()
        worst = float((eg / terms[b].clamp_min(1e-300)).max())
        print("%dx%d nc %d %s band %d: A rel %.2e (bound %.2e), GL rel to its terms %.2e (bound %.2e)" % (
            W, H, nc, units, b, ea, a_rel, worst, a_rel + 25 * 2.0 ** -24 + FAST_SLACK))
        assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(GL).all())
        assert ea <= a_rel, b
        assert bool((eg <= bound).all()), b
        assert bool(((GL64[b] == 0) == (GL == 0)).all()), b                  # the zero conventions, pixel for pixel
        flat = GL.reshape(n, nc, -1)
        assert bool((flat[:, :, :min(3, h * w)] == 0).all())               # D == 0, the d_max clamp, the contrast clamp
        if h * w > 3:
            assert bool((flat[:, :, 3] != 0).all())                        # |T'| == |R'|: the tie is split, not dropped
        nonzero += int((GL != 0).sum())
    assert nonzero > 0


# ---- 3. against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.CASES))
@pytest.mark.parametrize("units", mc.UNITS)
def test_map_and_gradient_against_the_reference(name, units):
    mk, T, R, kw = _case(name)
    gold = mc.load_golden(name)
    Wt = torch.from_numpy(mc.case_weights(name)).to(DEV)
    m = _metric(**mk)
    x = T.clone().requires_grad_(True)
    dm = _map(m, name, x, R, kw, units=units)
    assert dm.grad_fn is not None and dm.shape == Wt.shape
    (Wt * dm).sum().backward()
    got_map = dm.detach().cpu().numpy()
    want_map = gold["map_" + units]
    emap = float(np.abs(got_map - want_map).max() / want_map.max())
    g = x.grad.cpu().numpy()
    g = g[0][:, None] if mc.CASES[name][1] == 1 else g                     # [C, N, H, W]
    g_ref = gold["grad_" + units]
    assert np.isfinite(g).all() and g.shape == g_ref.shape
    keep = np.broadcast_to(gold["map_jod"][None] >= mc.map_floor(name), g.shape) if units == "jod" else np.ones(g.shape, bool)
    gmax = float(np.abs(g_ref).max())
    err = float(np.abs(g - g_ref)[keep].max())
    print("%s %s: map rel %.3e; max|g - g_ref| = %.3e, max|g_ref| = %.3e, rel %.3e (all pixels: %.3e)" % (
        name, units, emap, err, gmax, err / gmax, float(np.abs(g - g_ref).max()) / gmax))
    assert emap <= MAP_TOL[name][mc.UNITS.index(units)]
    assert err <= GOLDEN_TOL[name][mc.UNITS.index(units)] * gmax
    if mc.CASES[name][7].get("oob"):
        t = mc.case_inputs(name)[0]
        oob = (t < 0) | (t > 1)
        assert oob.any() and (g[oob] == 0).all()


# ---- 4. invariants, exact -----------------------------------------------------------------------------------------------------
def _pairs(B, Cc, H, W, seed):
    from fovvideovdp_amd.synth import synth_frame_pair
    ts, rs = [], []
    for k in range(B):
        t8, r8 = synth_frame_pair(1, H, W, C=Cc, seed_ref=seed + k, seed_test=seed + 40 + k)
        ts.append(t8.float() / 255.0)
        rs.append(r8.float() / 255.0)
    return torch.stack(ts).to(DEV), torch.stack(rs).to(DEV)


def _clip(Cc, N, H, W, seed):
    from fovvideovdp_amd.synth import synth_video_pair
    t8, r8 = synth_video_pair(N, H, W, C=Cc, seed_ref=seed, seed_test=seed + 40)
    return (t8.float() / 255.0).to(DEV), (r8.float() / 255.0).to(DEV)


def _grad(fn, T, G, **kw):
    x = T.clone().requires_grad_(True)
    dm = fn(x, **kw)
    dm.backward(G)
    return dm.detach(), x.grad


@pytest.mark.parametrize("units", mc.UNITS)
def test_image_invariants(units):
    m = _metric("standard_4k")
    T, R = _pairs(3, 3, 68, 121, seed=31)
    G = torch.rand((3, 68, 121), device=DEV) + 0.1
    fn = lambda x: m.diff_map_images(x, R, units=units)   # noqa: E731
    dm, g = _grad(fn, T, G)
    assert torch.isfinite(g).all() and (g != 0).any()
    _, g2 = _grad(fn, T, 2 * G)
    assert torch.equal(g2, 2 * g)                                        # linear in the cotangent, bit for bit
    m.grad_batch = 1
    _, g1 = _grad(fn, T, G)
    m.grad_batch = None
    assert torch.equal(g1, g)
    for k in range(3):                                                   # pair k of the stack is pair k alone
        x = T[k:k + 1].clone().requires_grad_(True)
        d1 = m.diff_map_images(x, R[k:k + 1], units=units)
        d1.backward(G[k:k + 1])
        assert torch.equal(d1[0], dm[k]) and torch.equal(x.grad[0], g[k]), k
    # an identical pair: an all-zero map and an all-zero, finite gradient
    x = R.clone().requires_grad_(True)
    d0 = m.diff_map_images(x, R, units=units)
    d0.backward(G)
    assert (d0 == 0).all() and (x.grad == 0).all()


@pytest.mark.parametrize("units", mc.UNITS)
@pytest.mark.parametrize("padding", ["replicate", "circular"])
def test_video_invariants(units, padding):
    m = _metric("standard_fhd", padding=padding)
    T, R = _clip(1, 6, 68, 121, seed=33)
    G = torch.rand((6, 68, 121), device=DEV) + 0.1
    fn = lambda x: m.diff_map_video(x, R, frames_per_second=30, units=units)   # noqa: E731
    dm, g = _grad(fn, T, G)
    assert dm.shape == (6, 68, 121) and g.shape == T.shape and torch.isfinite(g).all() and (g != 0).any()
    _, g2 = _grad(fn, T, 2 * G)
    assert torch.equal(g2, 2 * g)
    m.grad_batch = 1
    _, g1 = _grad(fn, T, G)
    m.grad_batch = None
    assert torch.equal(g1, g)
    m.batch_frames = 4
    dm4, g4 = _grad(fn, T, G)
    m.batch_frames = None
    assert torch.equal(dm4, dm) and torch.equal(g4, g)
    x = R.clone().requires_grad_(True)
    d0 = m.diff_map_video(x, R, frames_per_second=30, units=units)
    d0.backward(G)
    assert (d0 == 0).all() and (x.grad == 0).all()


def test_gradient_stays_inside_the_pyramids_support():
    """A cotangent that is zero outside a 16x16 window: the gradient is zero outside the window dilated by the support of the
    adjoint (tests/map_grad_ref.gradient_support) and non-zero inside the window."""
    m = _metric("standard_4k")
    H, W = 540, 960
    T, R = _pairs(1, 1, H, W, seed=35)
    n_bands, _ = m._band_count(W, H)
    G = torch.zeros((1, H, W), device=DEV)
    G[0, 8:24, 8:24] = 1.0
    sup = ref.gradient_support(G[0].cpu() != 0, n_bands).to(DEV)
    share = float(sup.double().mean())
    print("%d bands: the support covers %.1f %% of the frame" % (n_bands, 100 * share))
    assert share < 0.9                                                   # (else the test shows nothing)
    for units in mc.UNITS:
        _, g = _grad(lambda x: m.diff_map_images(x, R, units=units), T, G)
        assert (g[0, 0][~sup] == 0).all()
        assert float((g[0, 0, 8:24, 8:24] != 0).double().mean()) > 0.99
        assert (g[0, 0][sup] != 0).any()


# ---- 5. half precision ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_precision(dtype):
    m = _metric("standard_4k")
    T, R = _pairs(2, 3, 68, 121, seed=37)
    Th, Rh = T.to(dtype), R.to(dtype)
    G = torch.rand((2, 68, 121), device=DEV) * 64.0 + 1.0
    for units in mc.UNITS:
        fn = lambda x: m.diff_map_images(x, Rh, units=units)   # noqa: E731
        d32, g32 = _grad(lambda x: m.diff_map_images(x, Rh.float(), units=units), Th.float(), G)
        dh, gh = _grad(fn, Th, G)
        assert dh.dtype is torch.float32 and torch.equal(dh, d32)        # the fp32 map of the upcast input
        assert gh.dtype is dtype and torch.equal(gh, g32.to(dtype))      # the fp32 gradient rounded once
        # a mixed pair goes through the float32 kernels
        dmx, gmx = _grad(lambda x: m.diff_map_images(x, Rh.float(), units=units), Th, G)
        assert torch.equal(dmx, d32) and gmx.dtype is dtype and torch.equal(gmx, g32.to(dtype))
    Tc, Rc = _clip(1, 4, 68, 121, seed=38)
    Gc = torch.rand((4, 68, 121), device=DEV) * 64.0 + 1.0
    d32, g32 = _grad(lambda x: m.diff_map_video(x, Rc.to(dtype).float(), frames_per_second=30), Tc.to(dtype).float(), Gc)
    dh, gh = _grad(lambda x: m.diff_map_video(x, Rc.to(dtype), frames_per_second=30), Tc.to(dtype), Gc)
    assert torch.equal(dh, d32) and gh.dtype is dtype and torch.equal(gh, g32.to(dtype))


# ---- 6. composition with torch's own ops ------------------------------------------------------------------------------------
def test_losses_compose():
    m = _metric("standard_4k")
    T, R = _pairs(1, 3, 135, 240, seed=39)
    mask = torch.zeros((1, 135, 240), device=DEV)
    mask[:, 40:90, 60:180] = 1.0
    x = T.clone().requires_grad_(True)
    dm = m.diff_map_images(x, R)
    (mask * dm).amax().backward()                                        # worst pixel inside the mask: a one-hot cotangent
    g_max = x.grad.clone()
    n_bands, _ = m._band_count(240, 135)
    peak = (mask * dm.detach())[0] == (mask * dm.detach()).amax()
    assert int(peak.sum()) == 1
    sup = ref.gradient_support(peak.cpu(), n_bands).to(DEV)
    assert (g_max != 0).any() and (g_max[0][:, ~sup] == 0).all() and torch.isfinite(g_max).all()
    x.grad = None
    dm = m.diff_map_images(x, R)
    dm.flatten().topk(50).values.mean().backward()                       # a top-k mean
    assert (x.grad != 0).any() and torch.isfinite(x.grad).all() and not torch.equal(x.grad, g_max)
    # a host leaf in another layout: the gradient lands there
    xh = T.cpu().permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    dmh = m.diff_map_images(xh, R.cpu().permute(0, 2, 3, 1), dim_order="BHWC")
    assert torch.equal(dmh, dm.detach())
    dmh.flatten().topk(50).values.mean().backward()
    assert xh.grad.device.type == "cpu" and torch.equal(xh.grad.permute(0, 3, 1, 2).to(DEV), x.grad)
    # no gradient asked for: no graph
    assert m.diff_map_images(T, R).grad_fn is None
    with torch.no_grad():
        assert m.diff_map_images(x, R).grad_fn is None
    (gg,) = torch.autograd.grad(m.diff_map_images(x, R).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        gg.sum().backward()                                              # double backward is refused


# ---- 7. the code objects ------------------------------------------------------------------------------------------------------
def test_new_kernels_do_not_spill():
    import codeobj
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    found = [n for n in md if "map_level_kernel" in n]
    assert len(found) == 2, found                                        # one per number of temporal channels
    for n in found:
        x = md[n]
        assert (x["sgpr_spill_count"], x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), n
        assert x["max_flat_workgroup_size"] == 256, n
