"""The float64 restatement of the shared pyramid backward (tests/pyramid_grad_ref.py) without a GPU: its matrices against the
oracle's reduce, its pointwise formulas, its sweep and its coefficients against torch autograd of float64 forwards written from
the definitions, and the mutants: wrong variants of the REFERENCE that the bounds of tests/test_gpu_pyramid_grad.py must see at
the shapes that test runs."""
import os
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_grad_ref as ref                  # noqa: E402
import pyramid_grad_ref as pg               # noqa: E402

F64 = torch.float64
# both sides float64 and analytic: relative to the largest entry compared
AUTOGRAD_BOUND = 1e-11
_k = []


def consts():
    if not _k:
        _k.append(pg.pool_constants(fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)))
    return _k[0]


def rel(got, want):
    return float((got - want).abs().max()) / float(want.abs().max())


def test_reduce_matrix_is_the_oracles_reduce():
    from oracle import fvvdp_oracle as orc
    rng = np.random.default_rng(7)
    sizes = [(h, w) for h in range(2, 10) for w in range(2, 10)]
    for W, H, nb in pg.SHAPES:
        sizes += [(h, w) for w, h in ref.level_sizes(W, H, nb + 1)[:-1]]       # every level that is reduced
    for h, w in sizes:
        hc, wc = (h + 1) // 2, (w + 1) // 2
        x = rng.standard_normal((1, h, w))
        want = orc.gausspyr_reduce(x, dtype=np.float64)[0]
        Rh, Rw = ref.reduce_matrix(h, h % 2 == 1), ref.reduce_matrix(w, h % 2 == 1)
        got = (Rh @ torch.from_numpy(x[0]) @ Rw.T).numpy()
        assert got.shape == want.shape == (hc, wc)
        assert np.abs(got - want).max() <= 4e-16 * np.abs(x).max(), (h, w)
        # the transpose, as pyramid_grad_ref.reduce_t applies it: <Reduce x, y> == <x, Reduce^T y>
        y = rng.standard_normal((hc, wc))
        back = pg.reduce_t(torch.from_numpy(y), h, w).numpy()
        assert abs(float((want * y).sum()) - float((x[0] * back).sum())) <= 1e-14 * float(np.abs(x).sum() * np.abs(y).max()), (h, w)


def _clip_q(maps, k, nc):
    """Q [n_bands, nc, n] of the stored (differentiable) D maps: the n frames as one clip"""
    return torch.stack([pg.band_q(mp["D"][:, :nc], k).T for mp in maps])


@pytest.mark.parametrize("W,H,n_bands", pg.SHAPES[:1] + pg.SHAPES[3:])
@pytest.mark.parametrize("nc", [1, 2])
def test_test_side_formula_is_the_autograd_of_the_forward(W, H, n_bands, nc):
    """layers -> band_forward -> (mean D^beta)^(1/beta) -> pooling -> JOD, in float64: a clip of n frames (nc 2), n stills (nc 1)"""
    k = consts()
    n = 3
    layers, maps = pg.synthetic_ref_maps(W, H, n_bands, n, nc, k, seed=W + nc)
    layers = [x.requires_grad_(True) for x in layers]
    ref.forward_maps(layers, maps, k, nc)
    Q = _clip_q(maps, k, nc)
    npx = [w * h for w, h in ref.level_sizes(W, H, n_bands)]
    gamma = torch.tensor([0.7, -1.3, 0.4], dtype=F64)
    if nc == 2:
        (gamma[0] * pg.pool_jod(Q, k)).backward()
        coef = pg.video_coef(Q.detach(), gamma[0], k, npx, 0, n)
    else:
        sum(gamma[i] * pg.pool_jod(Q[:, :, i:i + 1], k) for i in range(n)).backward()
        coef = pg.still_coef(Q.detach()[:, 0], gamma, k, npx)[:, None]
    stored = [{key: val.detach() for key, val in mp.items()} for mp in maps]
    skip = [pg.PX_D0, pg.PX_COLLAPSED]                                     # not differentiable / a convention on fp32 maps
    for b in range(n_bands):
        got = pg.band_layers(stored[b], coef[:, :, b], b, k, "test", nc)[0].reshape(n, nc, -1)
        want = layers[b].grad.reshape(n, nc, -1).clone()
        assert bool((got[:, :, skip] == 0).all()) and bool((got[:, :, [pg.PX_DMAX, pg.PX_TCLAMP]] == 0).all())
        assert bool((got[:, :, [pg.PX_TIE, pg.PX_LBKG_AT, pg.PX_LBKG_BELOW, pg.PX_RCLAMP]] != 0).all())
        want[:, :, skip] = 0.0
        assert bool(torch.isfinite(want).all()) and rel(got, want) <= AUTOGRAD_BOUND, b


def _ref_forward_D(layerT, layerR, E, mp, b, nc, k):
    """D [n, nc, h, w] of one band as a function of the reference's layer and of E = Expand(G^RS_{b+1}): L = max(E, lbkg_min),
    S = S0 (L / L0)^kappa, both contrasts divided by L and clamped."""
    m = 1.0 if b == 0 else 2.0
    L = torch.maximum(E, torch.tensor(k.lbkg_min, dtype=F64))[:, None]
    S = mp["S"][:, :nc] * (L / mp["lbkg"][:, None]) ** mp["kappa"][:, :nc]
    T = m * torch.clamp(layerT / L, max=k.cmax)
    R = m * torch.clamp(layerR / L, max=k.cmax)
    s = S * k.gain
    Tp, Rp = T * s, R * s
    q = torch.tensor(k.q[:nc], dtype=F64).view(1, nc, 1, 1)
    D = (Tp - Rp).abs() ** k.p / (1.0 + (k.k_mask * torch.minimum(Tp.abs(), Rp.abs())) ** q)
    return torch.clamp(D, max=k.dmax), T, R


@pytest.mark.parametrize("W,H,n_bands", pg.SHAPES[:1] + pg.SHAPES[3:])
@pytest.mark.parametrize("nc", [1, 2])
def test_reference_side_formulas_are_the_autograd_of_the_forward(W, H, n_bands, nc):
    k = consts()
    n = 3
    layers, maps = pg.synthetic_ref_maps(W, H, n_bands, n, nc, k, seed=W + nc + 50)
    npx = [w * h for w, h in ref.level_sizes(W, H, n_bands)]
    gamma = torch.tensor([0.7, -1.3, 0.4], dtype=F64)
    LR, EE, Ds = [], [], []
    for b, mp in enumerate(maps):
        m = 1.0 if b == 0 else 2.0
        L = mp["lbkg"]
        # the reference's layer that gives the stored contrast; a clamped one lies well beyond the clamp
        layerR = torch.where(mp["ref"] >= k.cmax * m, 2000.0 * L[:, None], mp["ref"] * L[:, None] / m).requires_grad_(True)
        E = L.clone()
        E.view(n, -1)[:, pg.PX_LBKG_AT] = 0.05                            # below the floor: L is lbkg_min, as stored
        E.requires_grad_(True)
        D, T, R = _ref_forward_D(layers[b], layerR, E, mp, b, nc, k)
        mp["D"] = torch.cat([D, torch.zeros_like(D)], dim=1)[:, :2]
        mp["contrast"] = torch.stack([T, R], dim=2).reshape(n, 2 * nc, *T.shape[-2:])
        LR.append(layerR)
        EE.append(E)
    Q = _clip_q(maps, k, nc)
    if nc == 2:
        (gamma[0] * pg.pool_jod(Q, k)).backward()
        coef = pg.video_coef(Q.detach(), gamma[0], k, npx, 0, n)
    else:
        sum(gamma[i] * pg.pool_jod(Q[:, :, i:i + 1], k) for i in range(n)).backward()
        coef = pg.still_coef(Q.detach()[:, 0], gamma, k, npx)[:, None]
    stored = [{key: val.detach() for key, val in mp.items()} for mp in maps]
    # D == 0 and the collapsed pair: not differentiable / a convention; L_bkg below the floor: no forward stores it
    skip = [pg.PX_D0, pg.PX_COLLAPSED, pg.PX_LBKG_BELOW]
    for b in range(n_bands):
        GLR, GX, _, _ = pg.band_layers(stored[b], coef[:, :, b], b, k, "ref", nc)
        GLR, GX = GLR.reshape(n, nc, -1), GX.reshape(n, nc, -1)
        want_lr = LR[b].grad.reshape(n, nc, -1).clone()
        want_e = EE[b].grad.reshape(n, -1).clone()
        want_lr[:, :, skip] = 0.0
        want_e[:, skip] = 0.0
        GB = (GLR - GX)[:, 0]
        assert bool(((GLR - GX)[:, 1:] == 0).all())                        # only plane 0 carries GB
        assert bool((GLR[:, :, [pg.PX_D0, pg.PX_COLLAPSED, pg.PX_DMAX, pg.PX_RCLAMP]] == 0).all())
        assert bool((GX[:, :, [pg.PX_D0, pg.PX_COLLAPSED, pg.PX_DMAX]] == 0).all())
        assert bool((GB[:, [pg.PX_LBKG_AT, pg.PX_LBKG_BELOW]] == 0).all())
        assert bool((GLR[:, :, [pg.PX_TCLAMP, pg.PX_TIE, pg.PX_LBKG_AT, pg.PX_LBKG_BELOW]] != 0).all())
        assert bool((GB[:, [pg.PX_TCLAMP, pg.PX_RCLAMP, pg.PX_TIE]] != 0).all())
        GB = GB.clone()
        GB[:, pg.PX_LBKG_BELOW] = 0.0
        GLRc = GLR.clone()
        GLRc[:, :, pg.PX_LBKG_BELOW] = 0.0
        assert bool(torch.isfinite(want_lr).all()) and bool(torch.isfinite(want_e).all())
        assert rel(GLRc, want_lr) <= AUTOGRAD_BOUND, b
        assert rel(GB, want_e) <= AUTOGRAD_BOUND, b


@pytest.mark.parametrize("W,H,n_bands", pg.SHAPES + ((3, 2, 1), (2, 3, 2)))
def test_sweep_and_level0_are_the_autograd_of_the_matrix_pyramid(W, H, n_bands):
    """J = sum_b <GL_b, G_b> - <GX_b, Expand(G_{b+1})>, G_{b+1} = Reduce(G_b): with GX = GL the layers' pairing of the test side,
    with GX = GLR - GB the reference side's.  dJ/dG_0 is level 0 of the sweep."""
    g = torch.Generator().manual_seed(W * H)
    sizes = ref.level_sizes(W, H, n_bands + 1)
    n = 2
    G0 = torch.randn((n, H, W), generator=g, dtype=F64).requires_grad_(True)
    GL = [torch.randn((n, h, w), generator=g, dtype=F64) for w, h in sizes[:-1]]
    GX = [torch.randn((n, h, w), generator=g, dtype=F64) for w, h in sizes[:-1]]
    G, J = G0, 0.0
    for b in range(n_bands):
        w, h = sizes[b]
        Gn = ref.reduce_matrix(h, h % 2 == 1) @ G @ ref.reduce_matrix(w, h % 2 == 1).T
        J = J + (GL[b] * G).sum() - (GX[b] * ref.expand(Gn, h, w)).sum()
        G = Gn
    J.backward()
    GG = None
    for lv in range(n_bands, 0, -1):
        GG, t = pg.sweep_level(GL[lv] if lv < n_bands else None, GX[lv - 1], GG)
        assert GG.shape[-2:] == (sizes[lv][1], sizes[lv][0]) and bool((t > 0).all())
    g0, t0 = pg.level0(GL[0], GG)
    assert bool((t0 > 0).all()) and rel(g0, G0.grad) <= AUTOGRAD_BOUND


def test_coefficients_are_the_autograd_of_the_pooling():
    k = consts()
    g = torch.Generator().manual_seed(11)
    nb, N = 4, 5
    npx = [640, 160, 40, 12]
    npx_t = torch.tensor(npx, dtype=F64).view(nb, 1, 1)
    clip = torch.rand((nb, 2, N), generator=g, dtype=F64) + 0.1
    frame0 = clip.clone()
    frame0[:, :, 2] = 0.0                                                  # one identical frame
    band0 = clip.clone()
    band0[1] = 0.0                                                         # an identical band, both channels, every frame
    chan0 = clip.clone()
    chan0[:, 1, 3] = 0.0                                                   # an identical transient channel in one frame
    # an identical clip: the JOD mapping itself has no derivative at Q = 0 (autograd: inf x 0); the coefficients are zero
    assert bool((pg.video_coef(torch.zeros_like(clip), -1.3, k, npx, 1, 3) == 0).all())
    for Q in (clip, frame0, band0, chan0):
        x = Q.clone().requires_grad_(True)
        pg.pool_jod(x, k).backward()
        scale = torch.where(Q > 0, torch.where(Q > 0, Q, torch.ones_like(Q)) ** (1.0 - k.beta), torch.zeros_like(Q)) / npx_t
        want = (-1.3 * x.grad * scale)[:, :, 1:4].permute(2, 1, 0)
        got = pg.video_coef(Q, -1.3, k, npx, 1, 3)
        assert got.shape == (3, 2, nb) and bool(torch.isfinite(got).all())
        assert bool(((got == 0) == (want == 0)).all()) and bool(((Q[:, :, 1:4].permute(2, 1, 0) == 0) == (got == 0)).all())
        if bool((want != 0).any()):
            assert rel(got, want) <= AUTOGRAD_BOUND
    # stills: a pair with one band at Q == 0
    Qs = torch.rand((nb, 2), generator=g, dtype=F64) + 0.1
    Qs[2, 1] = 0.0
    gam = torch.tensor([0.7, -1.3], dtype=F64)
    x = Qs.clone().requires_grad_(True)
    sum(gam[i] * pg.pool_jod(x[:, None, i:i + 1], k) for i in range(2)).backward()
    want = (x.grad * torch.where(Qs > 0, torch.where(Qs > 0, Qs, torch.ones_like(Qs)) ** (1.0 - k.beta), torch.zeros_like(Qs))
            / npx_t[:, 0]).T
    got = pg.still_coef(Qs, gam, k, npx)
    assert got.shape == (2, nb) and float(got[1, 2]) == 0.0 and int((got == 0).sum()) == 1
    assert rel(got, want) <= AUTOGRAD_BOUND


# ---- the mutants ---------------------------------------------------------------------------------------------------------------
def _seen(got, want, bound):
    """pixels at which the difference exceeds the bound the GPU test applies there"""
    return int(((got - want).abs() > bound).sum())


def _sweep_mutant(mutant, W, H, nb):
    g = torch.Generator().manual_seed(W + H)
    sizes = ref.level_sizes(W, H, nb + 1)
    seen = 0
    for lv in range(nb, -1, -1):
        w, h = sizes[lv]
        GL = torch.randn((2, h, w), generator=g, dtype=F64)
        GGc = torch.randn((2, sizes[lv + 1][1], sizes[lv + 1][0]), generator=g, dtype=F64) if lv < nb else None
        if lv == 0:
            want, t = pg.level0(GL, GGc)
            got, _ = pg.level0(GL, GGc, mutant)
        else:
            GXf = torch.randn((2, sizes[lv - 1][1], sizes[lv - 1][0]), generator=g, dtype=F64)
            want, t = pg.sweep_level(GL if lv < nb else None, GXf, GGc)
            got, _ = pg.sweep_level(GL if lv < nb else None, GXf, GGc, mutant)
        seen += _seen(got, want, pg.sweep_bound(t))
    return seen


def _layer_mutant(mutant, W, H, nb, side):
    k = consts()
    n, nc = 2, 2
    layers, maps = pg.synthetic_ref_maps(W, H, nb, n, nc, k, seed=W + H)
    pg.stored_maps(layers, maps, k, nc)
    coef = torch.rand((n, nc, nb), generator=torch.Generator().manual_seed(5), dtype=F64) + 0.5
    seen = 0
    for b in range(nb):
        want = pg.band_layers(maps[b], coef[:, :, b], b, k, side, nc)
        got = pg.band_layers(maps[b], coef[:, :, b], b, k, side, nc, mutant)
        # the loosest bound a layer kernel of that side is held to
        seen += _seen(got[0], want[0], pg.layer_bound(want[2], True, side == "ref"))
        seen += _seen(got[1], want[1], pg.layer_bound(want[3], True, side == "ref"))
    return seen


def _coef_mutant(mutant, W, H, nb):
    k = consts()
    npx = [w * h for w, h in ref.level_sizes(W, H, nb)]
    Q = torch.rand((nb, 2, 5), generator=torch.Generator().manual_seed(W), dtype=F64) + 0.1
    want = pg.video_coef(Q, 0.7, k, npx, 1, 3)
    return _seen(pg.video_coef(Q, 0.7, k, npx, 1, 3, mutant), want, pg.coef_bound(want))


@pytest.mark.parametrize("mutant", sorted(pg.MUTANTS))
def test_a_wrong_kernel_would_be_seen(mutant):
    """Each mutant perturbs the reference.  At one of the GPU test's shapes or more it must differ from the unperturbed
    reference, at one pixel or more, by more than the bound the GPU test applies at that pixel."""
    seen = {}
    for W, H, nb in pg.SHAPES:
        if mutant in "abcd":
            seen[(W, H, nb)] = _sweep_mutant(mutant, W, H, nb)
        elif mutant in "efgh":
            seen[(W, H, nb)] = _layer_mutant(mutant, W, H, nb, "test")
        elif mutant in "ijk":
            seen[(W, H, nb)] = _coef_mutant(mutant, W, H, nb)
        else:
            seen[(W, H, nb)] = _layer_mutant(mutant, W, H, nb, "ref")
    print("mutant %s (%s): pixels beyond the bound per shape %s" % (mutant, pg.MUTANTS[mutant], seen))
    assert any(v > 0 for v in seen.values())


def test_mutant_list_covers_every_hook():
    assert sorted(pg.MUTANTS) == list("abcdefghijklm")


# ---- the inputs of the GPU test --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,n_bands", pg.SHAPES)
@pytest.mark.parametrize("side", ["test", "ref"])
def test_terms_are_positive_wherever_the_value_is_not_zero(W, H, n_bands, side):
    """No pixel of the GPU comparison needs an exemption: a non-zero value always has positive terms to be relative to, every
    planted pixel sits on its branch, and every reduced level has two rows and columns or more."""
    k = consts()
    n, nc = 2, 2
    assert all(w >= 2 and h >= 2 for w, h in ref.level_sizes(W, H, n_bands + 1)[:-1])
    layers, maps = pg.synthetic_ref_maps(W, H, n_bands, n, nc, k, seed=W + H + 2)
    for x in layers + [mp[key] for mp in maps for key in ("lbkg", "S", "ref", "kappa")]:
        assert torch.equal(x, x.float().double())                         # what the kernel reads is what the restatement reads
    pg.stored_maps(layers, maps, k, nc)
    hi = 1.0 - ref.CLAMP_EPS
    for b, mp in enumerate(maps):
        m = 1.0 if b == 0 else 2.0
        D, Cn, L = mp["D"].reshape(n, 2, -1), mp["contrast"].reshape(n, 4, -1), mp["lbkg"].reshape(n, -1)
        T, R = Cn[:, 0::2], Cn[:, 1::2]
        assert bool((D[:, :, pg.PX_D0] == 0).all()) and bool((D[:, :, pg.PX_DMAX] == float(np.float32(k.dmax))).all())
        for px in (pg.PX_TCLAMP, pg.PX_RCLAMP, pg.PX_TIE, pg.PX_COLLAPSED, pg.PX_LBKG_AT, pg.PX_LBKG_BELOW):
            assert bool((D[:, :, px] > 0).all()) and bool((D[:, :, px] < k.dmax * hi).all()), px
        assert bool((T[:, :, pg.PX_TCLAMP] >= m * k.cmax * hi).all()) and bool((R[:, :, pg.PX_TCLAMP] < m * k.cmax * hi).all())
        assert bool((R[:, :, pg.PX_RCLAMP] >= m * k.cmax * hi).all()) and bool((T[:, :, pg.PX_RCLAMP] < m * k.cmax * hi).all())
        assert bool((T[:, :, pg.PX_TIE] == -R[:, :, pg.PX_TIE]).all())
        assert bool((T[:, :, pg.PX_COLLAPSED] != R[:, :, pg.PX_COLLAPSED]).all())
        col = ref.collapsed(T, R, mp["S"].reshape(n, 2, -1), k)
        assert bool(col[:, :, [pg.PX_D0, pg.PX_COLLAPSED]].all()) and int(col.sum()) == 2 * n * nc
        assert bool((L[:, pg.PX_LBKG_AT] == k.lbkg_min).all()) and bool((L[:, pg.PX_LBKG_BELOW] < k.lbkg_min).all())
        # the rest of the band keeps the cancellation in T' - R' bounded, as the derivation of LAYER_ULPS assumes
        rest = torch.ones(T.shape[-1], dtype=torch.bool)
        rest[[pg.PX_D0, pg.PX_COLLAPSED]] = False
        assert bool(((T - R).abs()[:, :, rest] * 9.0 >= (T.abs() + R.abs())[:, :, rest] * (1.0 - 1e-6)).all())
    coef = torch.rand((n, nc, n_bands), generator=torch.Generator().manual_seed(6), dtype=F64) + 0.5
    out = pg.backbone(maps, coef, k, side, nc)
    for GL, GX, tGL, tGX in out["per"]:
        assert bool((tGL[GL != 0] > 0).all()) and bool((tGX[GX != 0] > 0).all())
        assert bool((tGL >= GL.abs() * (1 - 1e-12)).all()) and bool((tGX >= GX.abs() * (1 - 1e-12)).all())
    for lv in range(1, n_bands + 1):
        assert bool((out["tGG"][lv] > 0).all()) and bool((out["tGG"][lv] >= out["GG"][lv].abs() * (1 - 1e-12)).all())
    assert bool((out["tg0"] > 0).all()) and bool(torch.isfinite(out["g0"]).all())
