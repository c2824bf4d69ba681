"""The kernels every differentiable entry point ends in, per pixel against the float64 restatement (tests/pyramid_grad_ref.py),
through the C ABI: fvvdp_images_grad, fvvdp_video_grad_frames, fvvdp_images_ref_grad and fvvdp_video_ref_grad_frames on synthetic
maps with every branch of the layer kernels planted.  The checks are stage-wise -- coef, GL_b (and GX_b), GG_L and level 0 are
read back from the workspace at the documented offsets and each is held against the restatement applied to the kernel's OWN
upstream output, widened from fp32 -- so errors do not compound and every stage bound is derived (pyramid_grad_ref.py), then
the whole chain once against the float64 composition.  No context and no forward pass: the entry points read only what they
are given.  tests/test_pyramid_grad_cpu.py shows that these bounds see a wrong kernel."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_grad_ref as ref                  # noqa: E402
import pyramid_grad_ref as pg               # noqa: E402
import video_grad_input_ref as vref         # noqa: E402
from test_gpu_diff_map import A_ULPS, FAST_SLACK           # noqa: E402
from test_gpu_video_grad_input import DERIV_TOL            # noqa: E402  (the project's allowance for eotf_grad's arithmetic)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F64 = torch.float64
U = pg.U
RGB2Y = np.array([0.2126, 0.7152, 0.0722], np.float32)
# display models of the still chain: the parameters DERIV_TOL was measured with; LINEAR's derivative is exactly 0 or 1
EOTFS = {"srgb": (nat.EOTF_SRGB, dict(Y_peak=200.0, Y_black=0.2), DERIV_TOL["srgb"]),
         "gamma": (nat.EOTF_GAMMA, dict(Y_peak=300.0, Y_black=0.375, gamma=2.2), DERIV_TOL["gamma2.2"]),
         "pq": (nat.EOTF_PQ, dict(Y_peak=1500.0, Y_black=0.0175), DERIV_TOL["pq1500"]),
         "linear": (nat.EOTF_LINEAR, dict(Y_peak=1500.0, Y_black=0.0175), 0.0)}
PQ_MARGIN = 1e-4        # no PQ sample within this relative distance of a luminance clamp (test_gpu_video_grad_input.py)
# The whole chain against the float64 composition, relative to the composed terms: the one MEASURED bound of this file.  Per entry
# point (and, for the stills, per display model: PQ's derivative carries most of the error there) the worst value over every
# shape and batch of this file on MI355X; the bound is CHAIN_FACTOR x that, as the files next to this one set theirs.  In
# brackets the smallest cap among the cases, pyramid_grad_ref.chain_cap: the sum of the stage bounds along the deepest path,
# which the test asserts no bound exceeds.
#   fvvdp_images_grad            sRGB 4.6e-7 (1.6e-5), gamma 3.5e-7 (1.5e-5), PQ 1.83e-5 (8.0e-5), linear 3.3e-7 (1.5e-5)
#   fvvdp_images_ref_grad        sRGB 1.23e-6 (5.1e-5), gamma 1.28e-6 (5.0e-5), PQ 1.62e-5 (1.15e-4), linear 1.23e-6 (5.0e-5)
#   fvvdp_video_grad_frames      1.51e-6 (4.9e-5)
#   fvvdp_video_ref_grad_frames  1.28e-6 (5.0e-5)
# The stages, worst over the same runs: coef 7.6e-8 relative (bound 2^-23); adj_layer_kernel 1.3e-6 of its terms (bound 7.3e-6),
# layer_term<false> 3.7e-6 (4.1e-5), ref_layer_one 3.4e-6 (4.2e-5); the sweep 2.1e-7 and video_level0_kernel 2.2e-7 of their
# terms (2.4e-6); grad_input_kernel 5.7e-7 (sRGB), 3.1e-7 (gamma), 2.3e-5 (PQ), 2.5e-7 (linear).
CHAIN_MEASURED = {("images_grad", "srgb"): 4.6e-7, ("images_grad", "gamma"): 3.5e-7, ("images_grad", "pq"): 1.83e-5,
                  ("images_grad", "linear"): 3.3e-7, ("images_ref_grad", "srgb"): 1.23e-6, ("images_ref_grad", "gamma"): 1.28e-6,
                  ("images_ref_grad", "pq"): 1.62e-5, ("images_ref_grad", "linear"): 1.23e-6,
                  ("video_grad_frames", None): 1.51e-6, ("video_ref_grad_frames", None): 1.28e-6}
CHAIN_FACTOR = 3.0
_k = []


def consts():
    if not _k:
        m = fv.fvvdp(display_name="standard_4k", quiet=True, device=DEV)
        _k.append((pg.pool_constants(m), m.native_params(), m._pool_params()))
    return _k[0]


def chain_tol(entry, kind, cap):
    """CHAIN_FACTOR x the measurement, which may not exceed the sum of the stage bounds of the case"""
    tol = CHAIN_FACTOR * CHAIN_MEASURED[(entry, kind)]
    assert tol <= cap, "3x the measured chain error exceeds the sum of the stage bounds: a finding, not a reason to widen"
    return tol


@functools.lru_cache(maxsize=None)
def inputs(W, H, nb, n, nc):
    """The stored maps of a synthetic pyramid (float64 tensors holding fp32 values), computed once per shape and left unchanged"""
    k = consts()[0]
    layers, maps = pg.synthetic_ref_maps(W, H, nb, n, nc, k, seed=W + H + nc)
    return pg.stored_maps(layers, maps, k, nc)


def _f32(x):
    return x.to(torch.float32).to(DEV).contiguous()


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def layout(W, H, nb, n, P, ref_side):
    """The documented workspace layout (include/fvvdp_hip_grad.h, fvvdp_hip_video_grad.h, fvvdp_hip_ref_grad.h), in floats:
    dict(coef, gl[b], gg[L], gx[b], total, sizes)"""
    a64 = lambda x: (x + 63) // 64 * 64      # noqa: E731
    sizes = ref.level_sizes(W, H, nb + 1)
    off = a64(n * P * nb)
    gl, gg, gx = [], {}, []
    for b in range(nb):
        gl.append(off)
        off += a64(n * P * sizes[b][0] * sizes[b][1])
    for lv in range(1, nb + 1):
        gg[lv] = off
        off += a64(n * P * sizes[lv][0] * sizes[lv][1])
    if ref_side:
        for b in range(nb):
            gx.append(off)
            off += a64(n * P * sizes[b][0] * sizes[b][1])
    return dict(coef=0, gl=gl, gg=gg, gx=gx, total=off, sizes=sizes)


def device_maps(maps, nc):
    dev = [dict(D=_f32(mp["D"]), contrast=_f32(mp["contrast"]), lbkg=_f32(mp["lbkg"]), S=_f32(mp["S"]), kappa=_f32(mp["kappa"]))
           for mp in maps]
    arr = (nat.BandMaps * len(maps))()
    for b, d in enumerate(dev):
        arr[b].d_D, arr[b].d_contrast, arr[b].d_lbkg, arr[b].d_S = (d["D"].data_ptr(), d["contrast"].data_ptr(), d["lbkg"].data_ptr(),
                                                                  d["S"].data_ptr())
    slopes = (C.c_void_p * len(maps))(*[d["kappa"].data_ptr() for d in dev])
    return dev, arr, slopes


def band_qs(maps, nc):
    """Q [n_bands, nc, n] in float64 from the stored D maps"""
    k = consts()[0]
    return torch.stack([pg.band_q(mp["D"][:, :nc], k).T for mp in maps])


def read_workspace(host, lay, n, P, nb, ref_side):
    """coef [n, P, nb], GL[b], GG[L], GX[b] ([n, P, h, w]) as float64, every part finite and every gap between the parts still
    NaN: nothing the layout says is written is left out, nothing beyond it is touched."""
    written = torch.zeros(lay["total"], dtype=torch.bool)

    def part(off, shape):
        cnt = int(np.prod(shape))
        written[off:off + cnt] = True
        x = host[off:off + cnt].view(*shape)
        assert bool(torch.isfinite(x).all()), "NaN or inf left in a part of the workspace that the layout says is written"
        return x

    sizes = lay["sizes"]
    coef = part(lay["coef"], (n, P, nb))
    GL = [part(lay["gl"][b], (n, P, sizes[b][1], sizes[b][0])) for b in range(nb)]
    GG = {lv: part(lay["gg"][lv], (n, P, sizes[lv][1], sizes[lv][0])) for lv in range(1, nb + 1)}
    GX = [part(lay["gx"][b], (n, P, sizes[b][1], sizes[b][0])) for b in range(nb)] if ref_side else GL
    assert bool(torch.isnan(host[:lay["total"]][~written]).all()), "a kernel wrote into the alignment gaps of the workspace"
    return coef, GL, GG, GX


def same_zeros(got, want, what):
    assert bool(((got == 0) == (want == 0)).all()), "%s: the zero pattern differs from the reference's" % (what,)


def worst(got, want, scale):
    """max |got - want| / scale over the entries with a positive scale (0 when there is none)"""
    live = scale > 0
    return float(((got - want).abs()[live] / scale[live]).max()) if bool(live.any()) else 0.0


def check_stages(entry, side, fast, maps, coef64, host, lay, n, nc, nb, stats):
    """coef, the layer maps and the sweep, each against the restatement of that stage alone on the kernel's own upstream output.
    Returns (coef, GL, GG) as read."""
    k = consts()[0]
    ref_side = side == "ref"
    coef, GL, GG, GX = read_workspace(host, lay, n, nc, nb, ref_side)
    # coef: double arithmetic rounded once; exact zeros where the reference has zeros
    same_zeros(coef, coef64, "coef")
    assert bool(((coef - coef64).abs() <= pg.coef_bound(coef64)).all())
    stats["coef"] = max(stats.get("coef", 0.0), worst(coef, coef64, coef64.abs()))
    # layer maps
    for b in range(nb):
        wGL, wGX, tGL, tGX = pg.band_layers(maps[b], coef[:, :, b], b, k, side, nc)
        for name, got, want, t in (("GL", GL[b], wGL, tGL),) + ((("GX", GX[b], wGX, tGX),) if ref_side else ()):
            assert bool(((got - want).abs() <= pg.layer_bound(t, fast, ref_side)).all()), (name, b)
            same_zeros(got, want, "%s of band %d" % (name, b))
            stats["layer"] = max(stats.get("layer", 0.0), worst(got, want, t))
        fl, fx = GL[b].reshape(n, nc, -1), GX[b].reshape(n, nc, -1)
        for i in range(n):
            for cc in range(nc):
                g, x = fl[i, cc], fx[i, cc]
                if float(coef[i, cc, b]) == 0.0:                          # an identical band or frame: no weight anywhere
                    assert bool((g == 0).all()) and bool((x == 0).all())
                    continue
                assert float(g[pg.PX_D0]) == 0.0 and float(x[pg.PX_D0]) == 0.0                  # D == 0
                assert float(g[pg.PX_DMAX]) == 0.0 and float(x[pg.PX_DMAX]) == 0.0              # the d_max clamp binds
                assert float(g[pg.PX_COLLAPSED]) == 0.0 and float(x[pg.PX_COLLAPSED]) == 0.0    # D > 0 stored, T' == R' in fp32
                assert float(g[pg.PX_TIE]) != 0.0                                              # the tie is split, not dropped
                assert float(g[pg.PX_LBKG_AT]) != 0.0 and float(g[pg.PX_LBKG_BELOW]) != 0.0
                if not ref_side:
                    assert float(g[pg.PX_TCLAMP]) == 0.0 and float(g[pg.PX_RCLAMP]) != 0.0      # only the test's clamp counts
                else:
                    assert float(g[pg.PX_TCLAMP]) != 0.0 and float(g[pg.PX_RCLAMP]) == 0.0      # only the reference's clamp
                    if cc == 0:
                        # [E > lbkg_min]: no GB at or below the floor, so GX is GLR bit for bit; GB alone where r is clamped
                        assert float(x[pg.PX_LBKG_AT]) == float(g[pg.PX_LBKG_AT])
                        assert float(x[pg.PX_LBKG_BELOW]) == float(g[pg.PX_LBKG_BELOW])
                        assert float(x[pg.PX_RCLAMP]) != 0.0 and float(x[pg.PX_TCLAMP]) != float(g[pg.PX_TCLAMP])
                    else:
                        assert bool((x == g).all())                       # GB goes to plane 0 only
    # the sweep, coarse to fine
    for lv in range(nb, 0, -1):
        want, t = pg.sweep_level(GL[lv] if lv < nb else None, GX[lv - 1], GG[lv + 1] if lv < nb else None)
        assert bool(((GG[lv] - want).abs() <= pg.sweep_bound(t)).all()), lv
        same_zeros(GG[lv], want, "GG of level %d" % lv)
        stats["sweep"] = max(stats.get("sweep", 0.0), worst(GG[lv], want, t))
    return coef, GL, GG


def report(entry, case, stats):
    print("%s %s: worst error per stage -- coef rel %.2e (bound %.2e), layer / terms %.2e, sweep / terms %.2e (bound %.2e), "
          "level 0 / terms %.2e, whole chain / composed terms %.2e (bound %.2e)" % (
              entry, case, stats.get("coef", 0.0), pg.COEF_REL, stats.get("layer", 0.0), stats.get("sweep", 0.0),
              pg.SWEEP_ULPS * U, stats.get("level0", 0.0), stats["chain"], stats["chain_tol"]))


# ---- clips -------------------------------------------------------------------------------------------------------------------------
CLIP_CASES = [(W, H, nb, 5, 3, 1) for W, H, nb in pg.SHAPES] + [(7, 5, 2, 300, 2, 297)]


@pytest.mark.parametrize("W,H,nb,N,n,f0", CLIP_CASES)
@pytest.mark.parametrize("side", ["test", "ref"])
def test_clip_backbone_per_pixel(side, W, H, nb, N, n, f0):
    """fvvdp_video_grad_frames / fvvdp_video_ref_grad_frames: n frames at f0 of a clip of N (the second case: the strided clip
    norm over 300 frames, the last batch).  At 32x32 one frame of the batch has an all-zero Q."""
    k, prm, pp = consts()
    entry = "video_grad_frames" if side == "test" else "video_ref_grad_frames"
    ref_side = side == "ref"
    maps = inputs(W, H, nb, n, 2)
    g = torch.Generator().manual_seed(N + W)
    Qb = band_qs(maps, 2)
    Q = Qb.mean(dim=-1, keepdim=True) * (0.5 + torch.rand((nb, 2, N), generator=g, dtype=F64))
    Q[:, :, f0:f0 + n] = Qb
    if (W, H) == (32, 32):
        Q[:, :, f0 + 1] = 0.0                                            # an identical frame inside the batch
    Q32 = Q.float()
    gamma = float(np.float32(-1.3 if N == 300 else 0.7))
    lay = layout(W, H, nb, n, 2, ref_side)
    npx = [w * h for w, h in lay["sizes"][:nb]]
    coef64 = pg.video_coef(Q32.double(), gamma, k, npx, f0, n)

    lib = nat.lib()
    dev, arr, slopes = device_maps(maps, 2)
    nbytes = C.c_size_t(0)
    if ref_side:
        nat.check(lib.fvvdp_ref_grad_workspace(W, H, nb, n, 2, C.byref(nbytes)))
    else:
        nat.check(lib.fvvdp_video_grad_workspace(W, H, nb, n, C.byref(nbytes)))
    assert nbytes.value == 4 * lay["total"]                               # the documented layout is the library's
    work = torch.full((lay["total"],), float("nan"), dtype=torch.float32, device=DEV)
    g0 = torch.full((N, 2, H, W), float("nan"), dtype=torch.float32, device=DEV)
    Qd, gd = Q32.to(DEV).contiguous(), torch.tensor([gamma], dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        if ref_side:
            nat.check(lib.fvvdp_video_ref_grad_frames(W, H, nb, n, C.byref(prm), C.byref(pp), _ptr(Qd), N, f0, _ptr(gd), arr, slopes,
                                                      _ptr(g0), _ptr(work), nbytes.value, stream))
        else:
            nat.check(lib.fvvdp_video_grad_frames(W, H, nb, n, C.byref(prm), C.byref(pp), _ptr(Qd), N, f0, _ptr(gd), arr, _ptr(g0),
                                                  _ptr(work), nbytes.value, stream))
    torch.cuda.synchronize()
    host, g0h = work.double().cpu(), g0.double().cpu()
    stats = {}
    coef, GL, GG = check_stages(entry, side, True, maps, coef64, host, lay, n, 2, nb, stats)
    if (W, H) == (32, 32):
        assert bool((coef[1] == 0).all()) and bool((coef[0] != 0).all()) and bool((coef[2] != 0).all())
    # level 0: the batch's columns of the clip-long buffer, every other frame untouched
    got = g0h[f0:f0 + n]
    assert bool(torch.isfinite(got).all())
    assert bool(torch.isnan(g0h[:f0]).all()) and bool(torch.isnan(g0h[f0 + n:]).all())
    want, t = pg.level0(GL[0], GG[1])
    assert bool(((got - want).abs() <= pg.sweep_bound(t)).all())
    same_zeros(got, want, "g0")
    stats["level0"] = worst(got, want, t)
    # the whole chain: maps and Q -> g0, composed in float64
    full = pg.backbone(maps, coef64, k, side, 2)
    same_zeros(got, full["g0"], "g0 against the composition")
    stats["chain"] = worst(got, full["g0"], full["tg0"])
    stats["chain_tol"] = chain_tol(entry, None, pg.chain_cap(nb, True, ref_side))
    report(entry, "%dx%d, %d bands, frames [%d, %d) of %d" % (W, H, nb, f0, f0 + n, N), stats)
    assert stats["chain"] <= stats["chain_tol"]
    assert bool((got != 0).any())


# ---- stills ------------------------------------------------------------------------------------------------------------------------
def make_images(kind, n, HW, seed):
    """[n, 3, HW] fp32 samples with the edges of the display model planted behind the planted map pixels"""
    rng = np.random.default_rng(seed)
    V = rng.uniform(0.0, 1.0, (n, 3, HW)).astype(np.float32)
    f = np.float32
    if kind == "linear":
        V *= f(1600.0)                                                    # some beyond the peak
        plant = [f(0.005), np.nextafter(f(0.005), f(0)), np.nextafter(f(0.005), f(1)), f(1500.0), np.nextafter(f(1500.0), f(2000)),
                 f(0.0), f(-1.0), f(1e4)]
    else:
        knee = f(0.04045)
        plant = [f(0.0), f(1.0), knee, np.nextafter(knee, f(0)), np.nextafter(knee, f(1)), f(-0.25), f(1.5),
                 np.nextafter(f(1.0), f(2)), f(-1e-30)]
    V[:, :, pg.N_PLANTED:pg.N_PLANTED + len(plant)] = np.array(plant, np.float32)
    if kind == "pq":
        L = vref.pq_luminance(V)
        near = (np.abs(L / 0.005 - 1) < PQ_MARGIN) | (np.abs(L / 1500.0 - 1) < PQ_MARGIN)
        V[near] = f(0.5)                                                  # fp32 and fp64 could fall on different sides of a clamp
    return V, len(plant)


@pytest.mark.parametrize("W,H,nb", pg.SHAPES)
@pytest.mark.parametrize("kind", sorted(EOTFS))
@pytest.mark.parametrize("side", ["test", "ref"])
def test_still_backbone_per_pixel(side, kind, W, H, nb):
    """fvvdp_images_grad / fvvdp_images_ref_grad: two pairs with different upstream gradients, RGB behind each display model.  At
    32x32 one band of the second pair has Q == 0."""
    k, prm, pp = consts()
    entry = "images_grad" if side == "test" else "images_ref_grad"
    ref_side = side == "ref"
    n, HW = 2, W * H
    maps = inputs(W, H, nb, n, 1)
    Qb = band_qs(maps, 1)[:, 0]                                           # [nb, n]
    q_stride, q_col0 = n + 3, 2
    Q = torch.full((nb, 2, q_stride), 7.0, dtype=F64)                     # what is not the pairs' sustained column: never read
    Q[:, 0, q_col0:q_col0 + n] = Qb
    if (W, H) == (32, 32):
        Q[1, 0, q_col0 + 1] = 0.0
    Q32 = Q.float()
    gamma = torch.tensor([0.7, -1.3], dtype=torch.float32)
    lay = layout(W, H, nb, n, 1, ref_side)
    npx = [w * h for w, h in lay["sizes"][:nb]]
    coef64 = pg.still_coef(Q32.double()[:, 0, q_col0:q_col0 + n], gamma.double(), k, npx)[:, None]
    kind_id, ekw, deriv = EOTFS[kind]
    V, n_plant = make_images(kind, n, HW, seed=W + len(kind))
    cs = HW + 5                                                            # a gap between the channels

    lib = nat.lib()
    dev, arr, slopes = device_maps(maps, 1)
    nbytes = C.c_size_t(0)
    if ref_side:
        nat.check(lib.fvvdp_ref_grad_workspace(W, H, nb, n, 1, C.byref(nbytes)))
    else:
        nat.check(lib.fvvdp_images_grad_workspace(W, H, nb, n, C.byref(nbytes)))
    assert nbytes.value == 4 * lay["total"]
    work = torch.full((lay["total"],), float("nan"), dtype=torch.float32, device=DEV)
    imgs, grads = [], []
    for i in range(n):
        buf = np.full(3 * cs, np.nan, np.float32)
        for c in range(3):
            buf[c * cs:c * cs + HW] = V[i, c]
        imgs.append(torch.from_numpy(buf).to(DEV))
        grads.append(torch.full((3 * cs,), float("nan"), dtype=torch.float32, device=DEV))
    iptr = (C.c_void_p * n)(*[t.data_ptr() for t in imgs])
    gptr = (C.c_void_p * n)(*[t.data_ptr() for t in grads])
    eotf = nat.Eotf(kind_id, ekw["Y_peak"], ekw["Y_black"], ekw.get("gamma", 2.2), 0.0, 0.0, None)
    Qd, gd = Q32.to(DEV).contiguous(), gamma.to(DEV)
    with torch.cuda.device(DEV):
        stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        if ref_side:
            nat.check(lib.fvvdp_images_ref_grad(W, H, nb, n, C.byref(prm), C.byref(pp), _ptr(Qd), q_stride, q_col0, _ptr(gd), arr,
                                                slopes, iptr, 3, cs, C.byref(eotf), nat.fptr(RGB2Y), gptr, _ptr(work), nbytes.value,
                                                stream))
        else:
            nat.check(lib.fvvdp_images_grad(W, H, nb, n, C.byref(prm), C.byref(pp), _ptr(Qd), q_stride, q_col0, _ptr(gd),
                                            C.cast(arr, C.c_void_p), iptr, 3, cs, C.byref(eotf), nat.fptr(RGB2Y), gptr, _ptr(work),
                                            nbytes.value, stream))
    torch.cuda.synchronize()
    host = work.double().cpu()
    stats = {}
    coef, GL, GG = check_stages(entry, side, ref_side, maps, coef64, host, lay, n, 1, nb, stats)
    if (W, H) == (32, 32):
        assert float(coef[1, 0, 1]) == 0.0 and int((coef == 0).sum()) == 1
    out = torch.stack([x.double().cpu() for x in grads])                  # [n, 3 cs]
    got = torch.stack([out[:, c * cs:c * cs + HW] for c in range(3)], dim=1)          # [n, 3, HW]
    assert bool(torch.isfinite(got).all())
    gaps = torch.cat([out[:, c * cs + HW:(c + 1) * cs] for c in range(3)], dim=1)
    assert bool(torch.isnan(gaps).all()), "grad_input_kernel wrote between the channels"
    # level 0 and the display model: w_c EOTF'(V) (GL_0 + Reduce^T(GG_1)) on the kernel's own GL_0 and GG_1
    dv = torch.from_numpy(RGB2Y.astype(np.float64)[None, :, None] * vref.eotf_grad(V, kind_id, **ekw))      # [n, 3, HW]
    own, t = pg.level0(GL[0], GG[1])
    want, scale = dv * own.reshape(n, 1, HW), dv.abs() * t.reshape(n, 1, HW)
    assert bool(((got - want).abs() <= (pg.SWEEP_ULPS * U + deriv + 2 * U) * scale).all())
    same_zeros(got, want, "the gradient")
    stats["level0"] = worst(got, want, scale)
    # the planted samples: inside the closed range a gradient, outside an exact zero
    p0 = pg.N_PLANTED
    if kind == "linear":
        assert bool((got[:, :, [p0, p0 + 2, p0 + 3]] != 0).all()) and bool((got[:, :, [p0 + 1, p0 + 4, p0 + 5, p0 + 6, p0 + 7]] == 0).all())
    else:
        assert bool((got[:, :, p0 + 5:p0 + 9] == 0).all())                # -0.25, 1.5, the neighbours beyond 0 and 1
        if kind == "srgb":
            assert bool((got[:, :, p0:p0 + 5] != 0).all())                # 0, 1, the knee and its neighbours
        else:
            assert bool((got[:, :, p0] == 0).all())                       # V == 0: gamma and PQ have no slope there
    # the whole chain: maps, Q and image -> gradient, composed in float64
    full = pg.backbone(maps, coef64, k, side, 1)
    want, scale = dv * full["g0"].reshape(n, 1, HW), dv.abs() * full["tg0"].reshape(n, 1, HW)
    same_zeros(got, want, "the gradient against the composition")
    stats["chain"] = worst(got, want, scale)
    stats["chain_tol"] = chain_tol(entry, kind, pg.chain_cap(nb, ref_side, ref_side, deriv))
    report(entry, "%dx%d, %d bands, %s" % (W, H, nb, kind), stats)
    assert stats["chain"] <= stats["chain_tol"]
    assert bool((got != 0).any())


# ---- the collapsed difference on map_level_kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,nb", pg.SHAPES[:2])
def test_map_level_kernel_on_the_planted_pixels(W, H, nb):
    """fvvdp_diffmap_grad_levels (layer_term with a plane as the weight) on the same maps: the collapsed pixel is an exact zero
    there too, the other planted pixels sit on their branches, and every pixel meets test_gpu_diff_map.py's bound."""
    k, prm, pp = consts()
    n, nc = 3, 2
    maps = inputs(W, H, nb, n, nc)
    G = (torch.rand((n, H, W), generator=torch.Generator().manual_seed(9), dtype=F64) + 0.25).float().double()
    terms = []
    A64, GL64 = ref.adjoint(G, None, maps, k, "linear", nc, terms)
    lib = nat.lib()
    dev, arr, _ = device_maps(maps, nc)
    nbytes = C.c_size_t(0)
    gl_off, a_off = (C.c_size_t * nb)(), (C.c_size_t * nb)()
    nat.check(lib.fvvdp_diffmap_grad_workspace(W, H, nb, n, nc, gl_off, a_off, C.byref(nbytes)))
    work = torch.full((nbytes.value // 4,), float("nan"), dtype=torch.float32, device=DEV)
    Gd = _f32(G)
    with torch.cuda.device(DEV):
        stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        nat.check(lib.fvvdp_diffmap_grad_levels(W, H, nb, n, nc, C.byref(prm), C.byref(pp), nat.DIFFMAP_LINEAR, _ptr(Gd), None, arr,
                                                _ptr(work), nbytes.value, stream))
    torch.cuda.synchronize()
    host = work.double().cpu()
    for b, (w, h) in enumerate(ref.level_sizes(W, H, nb)):
        GL = host[gl_off[b]:gl_off[b] + n * nc * h * w].view(n, nc, h, w)
        assert bool(torch.isfinite(GL).all())
        bound = ((A_ULPS + 25 * b) * U + 25 * U + FAST_SLACK) * terms[b]
        assert bool(((GL - GL64[b]).abs() <= bound).all()), b
        same_zeros(GL, GL64[b], "GL of band %d" % b)
        flat = GL.reshape(n, nc, -1)
        assert bool((flat[:, :, [pg.PX_D0, pg.PX_DMAX, pg.PX_TCLAMP, pg.PX_COLLAPSED]] == 0).all())
        assert bool((flat[:, :, [pg.PX_TIE, pg.PX_LBKG_AT, pg.PX_LBKG_BELOW, pg.PX_RCLAMP]] != 0).all())
