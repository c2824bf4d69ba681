"""Float64 restatement of the backbone every differentiable entry point ends in (include/fvvdp_hip_grad.h, fvvdp_hip_video_grad.h,
fvvdp_hip_ref_grad.h): the pooling coefficients, the layer gradients of the test and of the reference side, one level of the
coarse-to-fine sweep and level 0.  Written from the forward's definition on top of tests/map_grad_ref.py (the pyramid as dense
matrices, the masked difference of a band, its derivative and the `terms` device: next to every value the sum of the absolute
values of the terms it is the sum or difference of, which is what a rounding error of any fp32 evaluation is relative to).
Test helper, no GPU.  The bounds the GPU test (tests/test_gpu_pyramid_grad.py) applies per stage are defined here, so that
tests/test_pyramid_grad_cpu.py can show with the same functions that a wrong kernel would be seen.

  pool_constants(metric)                 map_grad_ref.constants plus beta_sch, beta_tch, beta_t, lbkg_min
  pool_jod(Q, k)                         the pooling of oracle.do_pooling_and_jods in torch float64 (differentiable)
  band_q(D, k)                           (mean D^beta)^(1/beta) over the pixels
  video_coef / still_coef                the coefficients c[f][cc][b] / c[k][b] from Q
  test_layer(c, ...)                     c D^(beta-1) dD/dT' S gain m / L_bkg
  ref_layer(c, ...)                      (GLR, GX) of the reference side
  sweep_level / level0                   GG_L = GL_L - Expand^T(GX_{L-1}) + Reduce^T(GG_{L+1}),  g0 = GL_0 + Reduce^T(GG_1)
  synthetic_ref_maps                     synthetic maps with a slope plane and every branch of the layer kernels planted
Every function that a mutant of the CPU test perturbs takes `mutant`, a name of MUTANTS; None is the restatement itself.
"""
import copy
import math

import numpy as np
import torch

import map_grad_ref as ref
from test_gpu_diff_map import FAST_SLACK    # the allowance the project gives the fast log2 / exp2 form of the powers
from video_grad_input_ref import eotf_grad  # noqa: F401  (the display model's derivative, for the callers of this module)

F64 = torch.float64
U = 2.0 ** -24                              # unit roundoff of fp32

# ---- the bounds of the GPU test, per stage -------------------------------------------------------------------------------------
# coef: evaluated in double and rounded to fp32 once.  The double evaluation is a dozen pow / multiplications of 2^-53 each; what
# is left is the one rounding (2^-24) and the fp32 reciprocal pixel count the kernel is given (2^-24): 2^-23, relative.
COEF_REL = 2.0 ** -23
# Sweep and level 0: an output is GL (1 term) - Expand^T (up to 5 x 5 = 25 terms) + Reduce^T (up to 3 x 3 = 9 terms), each term a
# fused multiply-add on an fp32 weight.  A weight is a sum of at most three of the constants 0.05, 0.25, 0.4 (x 2 for the expand),
# each 2^-24 from its decimal value, and a term carries a row and a column weight; a sum of n terms evaluated in any order has
# an error of at most n roundings of the running sum, each below 2^-24 of the sum of the absolute values.  35 terms: 35 roundings
# of the sums + 2 of the weights + the last additions: 40 x 2^-24 of `terms`.
SWEEP_ULPS = 40
# adj_layer_kernel, in units of 2^-24 relative to the quantity named, every error taken at its worst and added:
#   s = S gain                                                1
#   T' = T s, R' = R s                                        2 each (s, the product)
#   u = T' - R': the roundings of T' and R' are 2^-24 (|T'| + |R'|) <= 9 x 2^-24 |u| on the synthetic maps, plus s, plus the
#   subtraction                                               11
#   num = powf(|u|, p): p x 11 + 2 (powf: 1 ulp = 2^-23)      28.4
#   M = k min(|T'|, |R'|)                                     3
#   Mq = powf(M, q): q x 3 + 2 (q <= 4.95 over both parameter sets)   16.8
#   den = 1 + Mq                                              17.8
#   D = num / den                                             47.2
#   difference term p num / |u| / den: 28.4 + 11 + 17.8 + 3   60.2
#   masker term D / den q Mq / |T'|: 47.2 + 17.8 + 16.8 + 2 + 4   87.8
#   dD = difference term - masker term: + 1, relative to the sum of the absolute values of the two (`terms`)   88.8
#   powf(D, beta - 1): |beta - 1| x 47.2 + 2 (|beta - 1| <= 0.53 over both parameter sets)   27.0
#   c, s, m / L_bkg and four products                         6
# 88.8 + 27.0 + 6 = 121.8: 122 x 2^-24 = 7.3e-6 of `terms`.
LAYER_ULPS = 122
# ref_layer_one beyond that: a hardware reciprocal of L_bkg (1 ulp: 2), kappa - [x < cmax] (1), T' cT - R' cR (2 products, 1
# subtraction, relative to |T' cT| + |R' cR|), dif x du and mk x (...) (2 each), their difference (1), w (1), the sum over the
# channels (1), the product with 1 / L_bkg (1), GLR - GB (1): 15.
REF_LAYER_ULPS = LAYER_ULPS + 15


def coef_bound(want):
    return COEF_REL * want.abs()


def sweep_bound(terms):
    return SWEEP_ULPS * U * terms


def layer_bound(terms, fast, ref_side=False):
    """adj_layer_kernel (fast False: powf), layer_term<false> (fast True) and ref_layer_one (fast True, ref_side True)."""
    return ((REF_LAYER_ULPS if ref_side else LAYER_ULPS) * U + (FAST_SLACK if fast else 0.0)) * terms


MUTANTS = {
    "a": "column fix-up of the reduce chosen by the column parity",
    "b": "the last row's fix-up of the reduce without its K[4] term",
    "c": "the first row's fix-up of the reduce missing",
    "d": "expand's c + 1 not clamped at the edge",
    "e": "tie share 1 in place of 0.5",
    "f": "masker term given to the larger of |T'| and |R'|",
    "g": "contrast clamp ignored",
    "h": "d_max clamp ignored",
    "i": "w_transient missing from the transient coefficient",
    "j": "1/N missing",
    "k": "f0 ignored",
    "l": "[E > lbkg_min] ignored on the reference side",
    "m": "kappa dropped",
}


# ---- constants and pooling -------------------------------------------------------------------------------------------------------
def pool_constants(metric):
    k = ref.constants(metric)
    pp, prm = metric._pool_params(), metric.native_params()
    k.beta_sch, k.beta_tch, k.beta_t = float(pp.beta_sch), float(pp.beta_tch), float(pp.beta_t)
    k.lbkg_min = float(prm.lbkg_min)
    return k


def _lp_norm(x, p, dim, normalize):
    """lp_norm of the oracle: a p-norm along dim (kept), divided by N^(1/p) when normalised.  torch's norm has the subgradient
    0 at an all-zero input, which is the zero convention of the coefficients."""
    n = x.shape[dim] if normalize else 1
    return torch.linalg.vector_norm(x, ord=p, dim=dim, keepdim=True) / float(n) ** (1.0 / p)


def pool_jod(Q, k):
    """do_pooling_and_jods on Q [n_bands, 1 or 2, N] (float64 tensor): bands, temporal channels (the transient one weighted),
    frames (mean), then the JOD mapping."""
    if Q.shape[1] == 2:
        Q = Q * torch.tensor([1.0, k.w_transient], dtype=F64).view(1, 2, 1)
    q_sc = _lp_norm(Q, k.beta_sch, 0, False)
    q_tc = _lp_norm(q_sc, k.beta_tch, 1, False)
    q = _lp_norm(q_tc, k.beta_t, 2, True).reshape(())
    sign = -1.0 if k.jod_a < 0 else 1.0
    return sign * (abs(k.jod_a) ** (1.0 / k.beta_jod) * q) ** k.beta_jod + 10.0


def band_q(D, k):
    """Q of one band: (mean over the pixels of D^beta)^(1/beta); D [..., h, w] -> [...]"""
    return (D ** k.beta).mean(dim=(-2, -1)) ** (1.0 / k.beta)


def _ratio_pow(a, b, e):
    """(a / b)^e, zero where a or b is zero: the derivative of a norm at an entry, 0 where the norm it divides by is zero"""
    ok = (a > 0) & (b > 0)
    one = torch.ones_like(a * b)
    return torch.where(ok, (torch.where(ok, a * one, one) / torch.where(ok, b * one, one)) ** e, torch.zeros_like(one))


def video_coef(Q, gamma, k, npx, f0, n, mutant=None):
    """c[f][cc][b] = gamma dJOD/dQ[b, cc, f0 + f] Q^(1 - beta) / npx_b for f in [0, n), as [n, P, n_bands] float64 -- the
    factor of D^(beta - 1) dD in the gradient of a band pixel, Q_b = (mean D^beta)^(1/beta).  Q [n_bands, P, N] float64, P = 2
    (a clip) or 1 (a still: no transient weight); npx: pixels per band.  The derivative of every norm of the pooling, written
    out: d||x||_p / dx_i = (x_i / ||x||_p)^(p - 1), zero where the norm is zero."""
    Q = Q.abs()
    nb, P, N = Q.shape
    w = torch.tensor([1.0, k.w_transient], dtype=F64)[:P].view(1, P, 1)
    qw = Q * w
    q_sc = (qw ** k.beta_sch).sum(0) ** (1.0 / k.beta_sch)                       # [P, N]
    q_tc = (q_sc ** k.beta_tch).sum(0) ** (1.0 / k.beta_tch)                     # [N]
    q_all = ((q_tc ** k.beta_t).sum() / N) ** (1.0 / k.beta_t)
    sign = -1.0 if k.jod_a < 0 else 1.0
    dj = torch.zeros((), dtype=F64)
    if float(q_all) > 0:
        dj = gamma * sign * k.beta_jod * (abs(k.jod_a) ** (1.0 / k.beta_jod) * q_all) ** k.beta_jod / q_all
    gf = dj * _ratio_pow(q_tc, q_all, k.beta_t - 1.0) / (1.0 if mutant == "j" else float(N))
    gc = gf[None] * _ratio_pow(q_sc, q_tc[None], k.beta_tch - 1.0)
    w_out = torch.ones_like(w) if mutant == "i" else w
    gb = gc[None] * w_out * _ratio_pow(qw, q_sc[None], k.beta_sch - 1.0)
    c = gb * torch.where(Q > 0, torch.where(Q > 0, Q, torch.ones_like(Q)) ** (1.0 - k.beta), torch.zeros_like(Q))
    c = c / torch.as_tensor(npx, dtype=F64).view(nb, 1, 1)
    if mutant == "k":
        f0 = 0
    return c[:, :, f0:f0 + n].permute(2, 1, 0).contiguous()


def still_coef(Q, gamma, k, npx):
    """c[k][b] [n, n_bands] for Q [n_bands, n] (the sustained column of each pair) and gamma [n]: a clip of one frame and one
    temporal channel per pair."""
    return torch.stack([video_coef(Q[:, None, i:i + 1], gamma[i], k, npx, 0, 1)[0, 0] for i in range(Q.shape[1])])


# ---- layer gradients -----------------------------------------------------------------------------------------------------------
def _with(k, **over):
    k = copy.copy(k)
    for name, v in over.items():
        setattr(k, name, v)
    return k


def _pool_weight(c, T, R, S, cc, k):
    """c D^(beta - 1) with D the masked difference of the stored contrasts (0 where D is 0)"""
    s = S * k.gain
    Tp, Rp = T * s, R * s
    D = (Tp - Rp).abs() ** k.p / (1.0 + (k.k_mask * torch.minimum(Tp.abs(), Rp.abs())) ** k.q[cc])
    pos = D > 0
    return torch.where(pos, c * torch.where(pos, D, torch.ones_like(D)) ** (k.beta - 1.0), torch.zeros_like(D))


def test_layer(c, T, R, Dm, S, L, b, cc, k, terms=None, mutant=None):
    """GL of one band and temporal channel: c D^(beta-1) dD/dT' S gain m / L_bkg with the zero conventions on the stored maps
    (no weight, D == 0, a binding d_max or contrast clamp, a collapsed difference).  c broadcasts against the maps."""
    if mutant == "g":
        k = _with(k, cmax=math.inf)
    if mutant == "h":
        k = _with(k, dmax=math.inf)
    inner = {"e": "tie_share_one", "f": "masker_to_larger"}.get(mutant)
    return ref.layer_gradient(_pool_weight(c, T, R, S, cc, k), T, R, Dm, S, L, b, cc, k, terms, inner)


test_layer.__test__ = False                 # (a helper, whatever its name says to a test collector)


def ref_layer(c, T, R, Dm, S, kap, L, b, k, terms=None, mutant=None):
    """(GLR, GX) [n, CH, h, w] of one band of the reference side for c [n, CH, 1, 1], T, R, Dm, S, kap [n, CH, h, w] and
    L [n, h, w].  With E = Expand(G^RS_{b+1}), L = max(E, lbkg_min), S = S(L) of slope kappa = dlog S / dlog L, t = layer^T / L,
    r = layer^R / L, T = m min(t, cmax), R = m min(r, cmax):
        GLR_cc = dJ/dlayer^R_cc = w A_R s m / L [r < cmax]
        GB     = dJ/dE at fixed layers = [E > lbkg_min] / L sum_cc w (A_T T' (kappa - [t < cmax]) + A_R R' (kappa - [r < cmax]))
        GX_0 = GLR_0 - GB, GX_1 = GLR_1
    (dT'/dL = T' (kappa - 1) / L where t is not clamped, T' kappa / L where it is.)  A_R is A_T with the roles of T and R
    swapped, so both come from map_grad_ref.layer_gradient, which returns w A s m / L: A X' = that times X L / m.
    terms: receives (terms of GLR, terms of GX)."""
    n, CH = T.shape[:2]
    m = 1.0 if b == 0 else 2.0
    if mutant == "m":
        kap = torch.zeros_like(kap)
    free = _with(k, cmax=math.inf)          # the contrast clamp is applied here, per use
    hi = m * k.cmax * (1.0 - ref.CLAMP_EPS)
    glr, tglr, gb, tgb = [], [], 0.0, 0.0
    for cc in range(CH):
        w = _pool_weight(c[:, cc], T[:, cc], R[:, cc], S[:, cc], cc, k)
        tT, tR = [], []
        gT = ref.layer_gradient(w, T[:, cc], R[:, cc], Dm[:, cc], S[:, cc], L, b, cc, free, tT)
        gR = ref.layer_gradient(w, R[:, cc], T[:, cc], Dm[:, cc], S[:, cc], L, b, cc, free, tR)
        t_in, r_in = (T[:, cc] < hi).double(), (R[:, cc] < hi).double()
        glr.append(gR * r_in)
        tglr.append(tR[0] * r_in)
        gb = gb + (gT * T[:, cc] * (kap[:, cc] - t_in) + gR * R[:, cc] * (kap[:, cc] - r_in)) / m
        tgb = tgb + (tT[0] * T[:, cc].abs() * (kap[:, cc].abs() + t_in) + tR[0] * R[:, cc].abs() * (kap[:, cc].abs() + r_in)) / m
    if mutant != "l":
        above = (L > k.lbkg_min).double()
        gb, tgb = gb * above, tgb * above
    GLR, tGLR = torch.stack(glr, dim=1), torch.stack(tglr, dim=1)
    GX, tGX = GLR.clone(), tGLR.clone()
    GX[:, 0] -= gb
    tGX[:, 0] += tgb
    if terms is not None:
        terms.append((tGLR, tGX))
    return GLR, GX


# ---- the sweep -----------------------------------------------------------------------------------------------------------------
_K = (0.05, 0.25, 0.4, 0.25, 0.05)


def _reduce_rows(n, odd, mutant):
    Rm = ref.reduce_matrix(n, odd).clone()
    if mutant == "b":                       # the last row's fix-up adds K[4] at n - 2 (odd) or n - 1 (even)
        Rm[-1, n - 2 if odd else n - 1] -= _K[4]
    if mutant == "c":                       # the first row's fix-up adds K[1] at 0 and K[0] at 1
        Rm[0, 0] -= _K[1]
        Rm[0, 1] -= _K[0]
    return Rm


def _reduce_cols(n, n_rows, mutant):
    return ref.reduce_matrix(n, (n if mutant == "a" else n_rows) % 2 == 1)


def _expand(n_out, n_in, mutant):
    E = ref.expand_matrix(n_out, n_in).clone()
    if mutant == "d":                       # c + 1 past the last coarse sample reads nothing instead of the last sample
        for i in range(n_out):
            if i // 2 + 1 > n_in - 1:
                E[i, n_in - 1] -= ref.K2[4] if i % 2 == 0 else ref.K2[3]
    return E


def reduce_t(GG, h, w, mutant=None):
    """Reduce^T of the coarse GG [..., hc, wc] on the fine level h x w"""
    return _reduce_rows(h, h % 2 == 1, mutant).T @ GG @ _reduce_cols(w, h, mutant)


def expand_t(Y, hc, wc, mutant=None):
    """Expand^T of the fine Y [..., h, w] on the coarse level hc x wc"""
    return _expand(Y.shape[-2], hc, mutant).T @ Y @ _expand(Y.shape[-1], wc, mutant)


def sweep_level(GL, GXf, GGc, mutant=None, tin=None):
    """(GG_L, terms) of level L >= 1: GL_L [..., h, w] (None: the base band), GX_{L-1} [..., hf, wf] (on the test side GL_{L-1}),
    GG_{L+1} [..., hc, wc] (None: the base band).  tin: the terms of the three inputs, where they are results themselves (a
    composed chain); None: the inputs are given, their terms are their absolute values."""
    hf, wf = GXf.shape[-2:]
    h, w = (hf + 1) // 2, (wf + 1) // 2
    tGL, tGXf, tGGc = tin if tin is not None else (None if GL is None else GL.abs(), GXf.abs(), None if GGc is None else GGc.abs())
    g, t = -expand_t(GXf, h, w, mutant), expand_t(tGXf, h, w)
    if GL is not None:
        g, t = g + GL, t + tGL
    if GGc is not None:
        g, t = g + reduce_t(GGc, h, w, mutant), t + reduce_t(tGGc, h, w)
    return g, t


def level0(GL0, GG1, mutant=None, tin=None):
    """(g0, terms) = GL_0 + Reduce^T(GG_1)"""
    h, w = GL0.shape[-2:]
    tGL0, tGG1 = tin if tin is not None else (GL0.abs(), GG1.abs())
    return GL0 + reduce_t(GG1, h, w, mutant), tGL0 + reduce_t(tGG1, h, w)


# ---- synthetic maps with every branch planted ----------------------------------------------------------------------------------
# the planted pixels, by index in the flattened band (the first four are map_grad_ref.synthetic_maps's)
PX_D0, PX_DMAX, PX_TCLAMP, PX_TIE, PX_COLLAPSED, PX_LBKG_AT, PX_LBKG_BELOW, PX_RCLAMP = range(8)
N_PLANTED = 8


def collapsed_triple(gain, seed=0):
    """(T, R, S) as fp32-representable floats with T != R adjacent and fp32(T fp32(S gain)) == fp32(R fp32(S gain)): a search
    over random adjacent pairs (the product with a factor whose significand is below 1 merges about every other pair)."""
    g32 = np.float32(gain)
    rng = np.random.default_rng(seed)
    for _ in range(10000):
        S = np.float32(rng.uniform(1.0, 31.0))
        s = np.float32(S * g32)
        T = np.float32(rng.uniform(0.03, 0.06))
        R = np.nextafter(T, np.float32(1.0))
        if T != R and np.float32(T * s) == np.float32(R * s):
            return float(T), float(R), float(S)
    raise AssertionError("no collapsed pair found")


def synthetic_ref_maps(W, H, n_bands, n, nc, k, seed):
    """map_grad_ref.synthetic_maps plus a slope plane `kappa` [n, 2, h, w] per band and four more planted pixels, the same in
    every band, frame and channel (every band has N_PLANTED pixels or more at the shapes of the tests):
      PX_TCLAMP      replanted: only t clamped, the reference's contrast far from it (no cancellation in T' - R'), D below d_max
      PX_COLLAPSED   adjacent contrasts whose products with S gain coincide in fp32, the stored D tiny and positive
      PX_LBKG_AT     L_bkg exactly lbkg_min,  PX_LBKG_BELOW  L_bkg below it
      PX_RCLAMP      only r clamped, D below d_max
    Returns (layers, maps) as synthetic_maps; every value is fp32-representable, so that the fp32 maps the kernels read and the
    float64 maps of the restatement are the same numbers."""
    layers, maps = ref.synthetic_maps(W, H, n_bands, n, nc, k, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    Tc, Rc, Sc = collapsed_triple(k.gain)
    for b, (layer, mp) in enumerate(zip(layers, maps)):
        m = 1.0 if b == 0 else 2.0
        h, w = layer.shape[-2:]
        assert h * w >= N_PLANTED
        mp["kappa"] = (torch.rand((n, 2, h, w), generator=g, dtype=F64) * 1.5 - 0.6).float().double()
        mp["S"] = mp["S"] * 0.25               # (keeps most pixels below the d_max clamp under either parameter set)
        for name in ("lbkg", "S", "ref"):
            mp[name] = mp[name].float().double()
        layer = layer.float().double()
        fl, fr, fS, fL = layer.view(n, nc, -1), mp["ref"].view(n, nc, -1), mp["S"].view(n, 2, -1), mp["lbkg"].view(n, -1)
        fl[:, :, PX_TCLAMP] = 2000.0 * fL[:, None, PX_TCLAMP]
        fr[:, :, PX_TCLAMP] = 300.0 * m
        fS[:, :, PX_TCLAMP] = 0.0078125
        fL[:, PX_COLLAPSED] = 4.0
        fl[:, :, PX_COLLAPSED] = Tc * 4.0 / m
        fr[:, :, PX_COLLAPSED] = Rc
        fS[:, :, PX_COLLAPSED] = Sc
        for px, lb in ((PX_LBKG_AT, float(np.float32(k.lbkg_min))), (PX_LBKG_BELOW, 0.0625)):
            fl[:, :, px] = (torch.tensor(0.03125 * lb, dtype=F64)).float().double()      # contrasts 0.03125 m and 0.0078125 m
            fr[:, :, px] = 0.0078125 * m
            fL[:, px] = lb
        fl[:, :, PX_RCLAMP] = 500.0 * fL[:, None, PX_RCLAMP]
        fr[:, :, PX_RCLAMP] = k.cmax * m
        fS[:, :, PX_RCLAMP] = 0.0078125
        layers[b] = layer.float().double()
    return layers, maps


def stored_maps(layers, maps, k, nc):
    """forward_maps, then what is stored rounded to fp32 (as float64 tensors): the maps a kernel reads."""
    ref.forward_maps(layers, maps, k, nc)
    for mp in maps:
        mp["contrast"] = mp["contrast"].float().double()
        mp["D"] = mp["D"].float().double()
    return maps


# ---- the chain composed ----------------------------------------------------------------------------------------------------------
# (W, H, n_bands) of the GPU test: 7x5 -> 4x3 -> 2x2 (the last coarse sample is also the first); 121x68 ... 4x3 (row and column
# parities disagree in both directions); 259x6 (two blocks along x at level 0); 32x32 (exact block counts, band boundaries)
SHAPES = ((7, 5, 2), (121, 68, 5), (259, 6, 2), (32, 32, 3))


def band_layers(mp, c_b, b, k, side, nc, mutant=None):
    """(GL, GX, terms of GL, terms of GX) [n, nc, h, w] of band b from its stored maps and c_b [n, nc]; side "test": GX is GL"""
    n = c_b.shape[0]
    T, R = mp["contrast"][:, 0::2], mp["contrast"][:, 1::2]
    Dm, S = mp["D"][:, :nc], mp["S"][:, :nc]
    cb = c_b.reshape(n, nc, 1, 1)
    tm = []
    if side == "test":
        gl = [test_layer(cb[:, cc], T[:, cc], R[:, cc], Dm[:, cc], S[:, cc], mp["lbkg"], b, cc, k, tm, mutant) for cc in range(nc)]
        GL, t = torch.stack(gl, dim=1), torch.stack(tm, dim=1)
        return GL, GL, t, t
    GLR, GX = ref_layer(cb, T, R, Dm, S, mp["kappa"][:, :nc], mp["lbkg"], b, k, tm, mutant)
    return GLR, GX, tm[0][0], tm[0][1]


def backbone(maps, coef, k, side, nc):
    """Maps and coefficients [n, nc, n_bands] -> the level-0 gradient, every stage in float64 and the terms carried along:
    dict(per=[band_layers per band], GG, tGG (index L in [1, n_bands]), g0, tg0 [n, nc, H, W])."""
    nb = len(maps)
    per = [band_layers(maps[b], coef[:, :, b], b, k, side, nc) for b in range(nb)]
    GG, tGG = [None] * (nb + 2), [None] * (nb + 2)
    for lv in range(nb, 0, -1):
        GL, tGL = (per[lv][0], per[lv][2]) if lv < nb else (None, None)
        GG[lv], tGG[lv] = sweep_level(GL, per[lv - 1][1], GG[lv + 1], tin=(tGL, per[lv - 1][3], tGG[lv + 1]))
    g0, tg0 = level0(per[0][0], GG[1], tin=(per[0][2], tGG[1]))
    return dict(per=per, GG=GG, tGG=tGG, g0=g0, tg0=tg0)


def chain_cap(n_bands, fast, ref_side, deriv=0.0):
    """The sum of the stage bounds along the deepest path of the chain, relative to the composed terms: the coefficient, a layer
    kernel, one sweep per level and level 0, and for a still the display model's derivative (the project's allowance for
    eotf_grad, tests/test_gpu_video_grad_input.py) with its two products."""
    layer = (REF_LAYER_ULPS if ref_side else LAYER_ULPS) * U + (FAST_SLACK if fast else 0.0)
    return COEF_REL + layer + (n_bands + 1) * SWEEP_ULPS * U + deriv + 2 * U
