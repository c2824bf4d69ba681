"""Float64 torch restatement of the difference map and of its per-level adjoint (include/fvvdp_hip_diffmap.h), written from
the forward's definition: the expand of the pyramid as a dense matrix per axis, the heat-map reconstruction, the masked
difference of one band from its layer, and the adjoint (A_b, GL_b) as map_level_kernel states it.  Test helper, no GPU.

  expand_matrix(n_out, n_in)       one axis of gausspyr_expand (closed form of oracle._expand_axis) as [n_out, n_in]
  reconstruct(D, w_transient, nc)  v_0 from the bands' difference maps D[b] [n, 2, h_b, w_b]
  band_forward(layer, ...)         T (stored contrast) and D of one band and channel from the test's layer
  adjoint(G, v0, maps, k, units)   (A, GL): lists per band, A[b] [n, h_b, w_b], GL[b] [n, nc, h_b, w_b]
"""
from types import SimpleNamespace

import numpy as np
import torch

F64 = torch.float64
K2 = (0.1, 0.5, 0.8, 0.5, 0.1)            # 2 x the 5-tap kernel of the pyramid (kernel_a = 0.4)
CLAMP_EPS = 2.0 ** -20                    # a stored value within 2^-20 of a clamp counts as clamped (grad_fill_layer)


def constants(metric=None, **over):
    """The constants the adjoint reads: of a metric (fvvdp) or the defaults of the model, overridden by keywords."""
    k = SimpleNamespace(p=2.4, q=(3.237, 3.02), k_mask=10.0 ** -0.544583, gain=10.0 ** (3.0 / 20.0), beta=0.9575,
                        cmax=1000.0, dmax=1e4, w_transient=0.25, beta_jod=10.0 ** -0.3, jod_a=-0.25)
    if metric is not None:
        prm, pp = metric.native_params(), metric._pool_params()
        k = SimpleNamespace(p=float(prm.mask_p), q=(float(prm.mask_q[0]), float(prm.mask_q[1])), k_mask=float(prm.mask_k),
                            gain=float(prm.sens_gain), beta=float(prm.beta), cmax=float(prm.contrast_max), dmax=float(prm.d_max),
                            w_transient=float(pp.w_transient), beta_jod=float(pp.beta_jod), jod_a=float(pp.jod_a))
    for name, v in over.items():
        setattr(k, name, v)
    return k


def level_sizes(W, H, n_bands):
    out = [(W, H)]
    for _ in range(n_bands - 1):
        w, h = out[-1]
        out.append(((w + 1) // 2, (h + 1) // 2))
    return out


def expand_matrix(n_out, n_in):
    """E [n_out, n_in]: even i = 2c -> 0.1 x[c-1] + 0.8 x[c] + 0.1 x[c+1], odd i -> 0.5 x[c] + 0.5 x[c+1], indices clamped."""
    E = np.zeros((n_out, n_in))
    for i in range(n_out):
        c = i // 2
        cm, cp = max(c - 1, 0), min(c + 1, n_in - 1)
        if i % 2 == 0:
            E[i, cm] += K2[0]
            E[i, c] += K2[2]
            E[i, cp] += K2[4]
        else:
            E[i, c] += K2[1]
            E[i, cp] += K2[3]
    return torch.from_numpy(E)


def expand(x, h, w):
    """x [..., hc, wc] -> [..., h, w]"""
    return expand_matrix(h, x.shape[-2]) @ x @ expand_matrix(w, x.shape[-1]).T


def expand_t(y, hc, wc):
    """The transpose: y [..., h, w] -> [..., hc, wc]"""
    return expand_matrix(y.shape[-2], hc).T @ y @ expand_matrix(y.shape[-1], wc)


def reduce_matrix(n, odd_rows):
    """One axis of gausspyr_reduce as [ceil(n / 2), n]: the zero-padded stride-2 5-tap filter plus the edge fix-ups (reduce_w,
    grad_common.hpp); odd_rows: the parity of the fine level's ROW count, which the reference tests on both axes."""
    K = (0.05, 0.25, 0.4, 0.25, 0.05)
    nr = (n + 1) // 2
    Rm = np.zeros((nr, n))
    for r in range(nr):
        for j in range(n):
            kk = j - 2 * r + 2
            w = K[kk] if 0 <= kk <= 4 else 0.0
            if r == 0:
                w += (K[1] if j == 0 else 0.0) + (K[0] if j == 1 else 0.0)
            if r == nr - 1:
                if odd_rows:
                    w += (K[3] if j == n - 1 else 0.0) + (K[4] if j == n - 2 else 0.0)
                else:
                    w += K[4] if j == n - 1 else 0.0
            Rm[r, j] = w
    return torch.from_numpy(Rm)


def gradient_support(G_support, n_bands):
    """The level-0 pixels a cotangent with the boolean support G_support [H, W] can reach through the adjoint -- A_b, the layer
    gradients, the coarse-to-fine sweep and level 0 -- as a boolean [H, W]: the same chain on indicators (every stencil weight
    is positive, so nothing cancels)."""
    H, W = G_support.shape
    sizes = level_sizes(W, H, n_bands + 1)
    A = [G_support.double()]
    for b in range(1, n_bands):
        A.append((expand_t(A[-1], sizes[b][1], sizes[b][0]) > 0).double())
    GG = None
    for lv in range(n_bands, 0, -1):                                       # GG_L = GL_L - Expand^T(GL_{L-1}) + Reduce^T(GG_{L+1})
        w, h = sizes[lv]
        g = expand_t(A[lv - 1], h, w)
        if lv < n_bands:
            g = g + A[lv]
            g = g + reduce_matrix(h, h % 2 == 1).T @ GG @ reduce_matrix(w, h % 2 == 1)
        GG = (g > 0).double()
    g0 = A[0] + reduce_matrix(H, H % 2 == 1).T @ GG @ reduce_matrix(W, H % 2 == 1)
    return g0 > 0


def band_sum(D, b, k, nc):
    """(D_b[0] + w_transient D_b[1]) / m_b"""
    v = D[:, 0]
    if nc == 2:
        v = v + k.w_transient * D[:, 1]
    return v / (1.0 if b == 0 else 2.0)


def reconstruct(D, k, nc, keep=None):
    """v_0 [n, H, W] from D[b] [n, 2, h_b, w_b] (float64 tensors), coarse to fine; keep: a list that receives v_b per band."""
    v = None
    vs = [None] * len(D)
    for b in range(len(D) - 1, -1, -1):
        s = band_sum(D[b], b, k, nc)
        v = s if v is None else expand(v, s.shape[-2], s.shape[-1]) + s
        vs[b] = v
    if keep is not None:
        keep[:] = vs
    return v


def diff_map(v0, k, units):
    return v0 if units == "linear" else v0 ** k.beta_jod * abs(k.jod_a)


def band_forward(layer, Rc, S, L, b, cc, k):
    """One band and channel from the test's layer: T = m min(layer / L, cmax) (what the contrast map stores), T' = T S gain,
    D = min(|T' - R'|^p / (1 + (k min(|T'|, |R'|))^q), d_max).  Rc: the stored reference contrast."""
    m = 1.0 if b == 0 else 2.0
    T = m * torch.clamp(layer / L, max=k.cmax)
    s = S * k.gain
    Tp, Rp = T * s, Rc * s
    M = k.k_mask * torch.minimum(Tp.abs(), Rp.abs())
    D = (Tp - Rp).abs() ** k.p / (1.0 + M ** k.q[cc])
    return T, torch.clamp(D, max=k.dmax)


def collapsed(T, R, S, k):
    """Where the fp32 maps give T s == R s with s = S gain, all in fp32: the difference of the stored contrasts is gone, whatever
    D the forward stored, and every layer kernel treats the pixel as an identical one.  (A convention on fp32 maps, so it is
    stated in fp32; float64 maps that keep |T' - R'| well above an ulp are never collapsed.)"""
    s32 = S.detach().float() * torch.tensor(k.gain, dtype=torch.float32)
    return T.detach().float() * s32 == R.detach().float() * s32


def layer_gradient(weight, T, R, Dm, S, L, b, cc, k, terms=None, mutant=None):
    """weight dD/dT' S gain m / L_bkg per pixel, with the zero conventions of adj_layer_kernel on the stored maps.
    mutant: a deliberately wrong variant, for the tests that show a comparison can see it ("tie_share_one": the masker term of a
    tie |T'| == |R'| goes to T' whole; "masker_to_larger": the masker term goes to the larger of |T'|, |R'|)."""
    m = 1.0 if b == 0 else 2.0
    s = S * k.gain
    Tp, Rp = T * s, R * s
    u = Tp - Rp
    au, aT, aR = u.abs(), Tp.abs(), Rp.abs()
    M = k.k_mask * torch.minimum(aT, aR)
    q = k.q[cc]
    Mq = torch.where(M > 0, M ** q, torch.zeros_like(M))
    den = 1.0 + Mq
    num = au ** k.p
    D = num / den
    safe_au = torch.where(au > 0, au, torch.ones_like(au))
    dD0 = torch.where(au > 0, torch.sign(u) * k.p * num / safe_au / den, torch.zeros_like(u))
    safe_aT = torch.where(aT > 0, aT, torch.ones_like(aT))
    share = torch.where(aT < aR, torch.ones_like(aT), torch.full_like(aT, 1.0 if mutant == "tie_share_one" else 0.5))
    masker = share * torch.sign(Tp) * D / den * q * Mq / safe_aT
    has_masker = (M > 0) & (aT <= aR)
    if mutant == "masker_to_larger":
        masker = torch.where(aT > aR, masker / share, masker)
        has_masker = (M > 0) & (aT >= aR)
    dD = dD0 - torch.where(has_masker, masker, torch.zeros_like(masker))
    live = (weight != 0) & (Dm > 0) & (Dm < k.dmax * (1.0 - CLAMP_EPS)) & (T < m * k.cmax * (1.0 - CLAMP_EPS))
    live = live & ~collapsed(T, R, S, k)
    if terms is not None:                 # the sum of the absolute values of the two terms of dD, scaled like the result
        both = dD0.abs() + torch.where(has_masker, masker.abs(), torch.zeros_like(masker))
        terms.append(torch.where(live, weight.abs() * both * s * (m / L), torch.zeros_like(dD)))
    return torch.where(live, weight * dD * s * (m / L), torch.zeros_like(dD))


def adjoint(G, v0, maps, k, units, nc, terms=None):
    """G [n, H, W] cotangent, v0 [n, H, W] (units "jod"), maps[b]: dict D [n, 2], contrast [n, 2 nc], lbkg [n], S [n, 2]
    (float64 tensors) -> (A, GL) per band.  terms: a list that receives, per band, [n, nc, h, w] the magnitude of the terms
    each GL entry is the difference of (what a rounding error of the kernel is relative to)."""
    if units == "linear":
        A0 = G.clone()
    else:
        safe = torch.where(v0 > 0, v0, torch.ones_like(v0))
        A0 = torch.where(v0 > 0, G * k.beta_jod * abs(k.jod_a) * safe ** (k.beta_jod - 1.0), torch.zeros_like(G))
    A, GL = [], []
    for b, mp in enumerate(maps):
        Ab = A0 if b == 0 else expand_t(A[-1], mp["D"].shape[-2], mp["D"].shape[-1])
        A.append(Ab)
        m = 1.0 if b == 0 else 2.0
        gl, tm = [], (None if terms is None else [])
        for cc in range(nc):
            w_cc = 1.0 if cc == 0 else k.w_transient
            gl.append(layer_gradient(Ab * w_cc / m, mp["contrast"][:, 2 * cc], mp["contrast"][:, 2 * cc + 1], mp["D"][:, cc],
                                     mp["S"][:, cc], mp["lbkg"], b, cc, k, tm))
        GL.append(torch.stack(gl, dim=1))
        if terms is not None:
            terms.append(torch.stack(tm, dim=1))
    return A, GL


def synthetic_maps(W, H, n_bands, n, nc, k, seed, plant=True):
    """Layers and maps of a synthetic pyramid, float64: per band the test's layer [n, nc, h, w] (what the gradient is taken
    for) and the maps the forward of it stores.  plant: the first pixels of every band and channel sit at D == 0 (T' == R'),
    beyond the d_max clamp, beyond the contrast clamp and at |T'| == |R'| with opposite signs."""
    g = torch.Generator().manual_seed(seed)
    layers, maps = [], []
    for b, (w, h) in enumerate(level_sizes(W, H, n_bands)):
        m = 1.0 if b == 0 else 2.0
        L = torch.rand((n, h, w), generator=g, dtype=F64) * 50.0 + 0.5
        S = torch.rand((n, 2, h, w), generator=g, dtype=F64) * 30.0 + 1.0
        layer = (torch.rand((n, nc, h, w), generator=g, dtype=F64) - 0.5) * 0.2 * L[:, None]
        # |R| = |T| x a ratio in [0.2, 0.8] or [1.25, 5], either sign: |T' - R'| >= (|T'| + |R'|) / 9, so the cancellation in the
        # fp32 difference T' - R' -- which any fp32 evaluation has -- amplifies a rounding of 2^-24 by 9 (p - 1) at the most
        u1, u2, u3 = (torch.rand((n, nc, h, w), generator=g, dtype=F64) for _ in range(3))
        ratio = torch.where(u1 < 0.5, 0.2 + 0.6 * u2, 1.25 + 3.75 * u2) * torch.where(u3 < 0.5, -1.0, 1.0)
        Rc = m * layer / L[:, None] * ratio
        if plant:
            flat_l, flat_r = layer.view(n, nc, -1), Rc.view(n, nc, -1)
            Lf = L.reshape(n, 1, -1)
            npx = h * w
            if npx > 0:                                                                  # (powers of two: T == R exactly)
                flat_r[:, :, 0] = 0.0625 * m
                flat_l[:, :, 0] = 0.0625 * Lf[:, :, 0]                                   # T' == R': D == 0
            if npx > 1:
                flat_l[:, :, 1] = 900.0 * Lf[:, :, 1]                                    # D beyond d_max
            if npx > 2:
                flat_l[:, :, 2] = 2000.0 * Lf[:, :, 2]                                   # the contrast clamp
                flat_r[:, :, 2] = 999.5 * m                                              # ... with D below d_max
            if npx > 3:
                flat_r[:, :, 3] = 0.0625 * m
                flat_l[:, :, 3] = -0.0625 * Lf[:, :, 3]                                  # |T'| == |R'|, opposite signs
        layers.append(layer)
        maps.append(dict(lbkg=L, S=S, ref=Rc))
    return layers, maps


def forward_maps(layers, maps, k, nc):
    """Fills maps[b] with D [n, 2, h, w] and contrast [n, 2 nc, h, w] from the layers (differentiable in the layers)."""
    for b, (layer, mp) in enumerate(zip(layers, maps)):
        n, _, h, w = layer.shape
        Ds, Cs = [], []
        for cc in range(nc):
            T, D = band_forward(layer[:, cc], mp["ref"][:, cc], mp["S"][:, cc], mp["lbkg"], b, cc, k)
            Ds.append(D)
            Cs += [T, mp["ref"][:, cc]]
        if nc == 1:
            Ds.append(torch.zeros_like(Ds[0]))
        mp["D"] = torch.stack(Ds, dim=1)
        mp["contrast"] = torch.stack(Cs, dim=1)
    return maps
