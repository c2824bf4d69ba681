"""Test helper (not part of the product): the float64 side of the display-gradient tests.

  CASES / inputs / psi0     the end-to-end cases; content as param_grad_ref.inputs (reference uniform in [0.25, 0.75], test =
                            reference + 0.04 N(0, 1), the left half identical, one flat patch; narrower for PQ)
  jod                       Oracle(dtype=np.float64) under a psi, photometry=orc.Photometry(..., dtype=np.float64)
  central_differences       dJOD/dpsi [5] by central differences of that oracle, step 1e-5 max(|psi_i|, 1)
  intermediate_differences  U_fd = dJOD/d(Y_black, u1, gamma) by central differences through a subclass of orc.Photometry whose
                            forward takes the intermediate variables (u1: scale for sRGB / gamma, Y_peak for PQ / linear)
  disagree                  the yardstick's own error: the central differences against the reference's autograd (the golden),
                            normalised by scale_i, the worst over all cases and entries
  jacobian / scale          J[i][j] = du_j/dpsi_i and the per-entry yardstick scale_i = sum_j |J_ij U_fd,j|
  eotf_block / sens / video_s / sums_of
                            a numpy float64 evaluation of exactly what the sums entry points of include/fvvdp_hip_display.h
                            compute from their fp32 arguments: the temporal transpose from the window list (the folds
                            included), the sensitivity values, the sums and the sums of the absolute elementary terms
Every oracle result is computed once per process and shared."""
import functools
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import fvvdp_oracle as orc          # noqa: E402

NAMES = ("Y_peak", "contrast", "E_ambient", "k_refl", "gamma")
KINDS = {"sRGB": 1, "gamma": 2, "PQ": 3, "linear": 4}          # FVVDP_EOTF_*
SCALED = ("sRGB", "gamma")

# name: (display for the geometry and the defaults of psi, EOTF, psi entries the case fixes, foveated, C, frames, fps, padding);
# frames == 0: a stack of 3 still images
CASES = {
    "still_gamma_stack": ("standard_4k", "gamma", {"contrast": 50.0, "E_ambient": 500.0}, False, 3, 0, 0, "replicate"),
    "rgb_srgb_30": ("standard_4k", "sRGB", {}, False, 3, 6, 30, "replicate"),
    "gray_fov_gamma_60": ("standard_fhd", "gamma", {}, True, 1, 4, 60, "replicate"),
    "hdr_pq_30": ("standard_hdr_pq", "PQ", {"Y_peak": 1500.0, "contrast": 1e6, "E_ambient": 10.0}, False, 1, 3, 30, "replicate"),
    "circular_30": ("standard_4k", "sRGB", {}, False, 1, 12, 30, "circular"),
    "pingpong_rgb": ("standard_4k", "sRGB", {}, False, 3, 5, 30, "pingpong"),
}
GOLDEN_CASES = ("still_gamma_stack", "rgb_srgb_30", "gray_fov_gamma_60", "hdr_pq_30")
H, W = 68, 121
STILL_WEIGHTS = (1.0, -0.5, 2.0)


def psi0(name):
    """The display parameters the case runs at, float64 [5]."""
    display, eotf, fixed = CASES[name][:3]
    ph = orc.Photometry.load(display)
    v = dict(Y_peak=ph.Y_peak, contrast=ph.contrast, E_ambient=ph.E_ambient, k_refl=ph.k_refl, gamma=ph.gamma)
    v.update(fixed)
    return np.array([float(v[n]) for n in NAMES], dtype=np.float64)


# the cases whose content param_grad_ref already has (the same shape, channels, frames and gaze trace): its arrays, as they are
SHARED_INPUTS = {"still_gamma_stack": "still_f32_stack", "gray_fov_gamma_60": "gray_fov_60", "hdr_pq_30": "hdr_pq_30"}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(test, reference) float32 [B, C, F, H, W] (B = 3 and F = 1 for the still stack, else B = 1) and the gaze trace or None."""
    if name in SHARED_INPUTS:
        import param_grad_ref
        return param_grad_ref.inputs(SHARED_INPUTS[name])
    display, eotf, _, fov, C, N, fps, padding = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 211)
    ref = rng.uniform(0.25, 0.75, (1, C, N, H, W))
    test = ref + 0.04 * rng.standard_normal(ref.shape)
    test[..., : W // 2] = ref[..., : W // 2]                         # identical half: D = 0
    y0, x0 = H // 3, W // 2 + W // 8
    for a in (test, ref):
        a[..., y0:y0 + 24, x0:x0 + 24] = 0.5                         # flat patch: M = 0 (and D = 0) inside
    return np.clip(test, 0, 1).astype(np.float32), np.clip(ref, 0, 1).astype(np.float32), None


class _IntermediatePhotometry(orc.Photometry):
    """orc.Photometry with the intermediate variables as its state: (Y_black, u1, gamma), u1 = scale or Y_peak."""

    def __init__(self, eotf, y_black, u1, gamma):
        super().__init__(u1, EOTF=eotf, gamma=gamma, dtype=np.float64)
        self.y_black, self.u1 = y_black, u1

    def get_black_level(self):
        return self.y_black

    def forward(self, V):
        if self.EOTF not in SCALED:                 # Y_peak = u1 enters through the clip only
            return super().forward(V)
        F = np.float64
        V = np.asarray(V, dtype=F)
        oob = bool(np.any(V > 1) or np.any(V < 0))
        V = np.clip(V, 0.0, 1.0)
        f = orc.srgb2lin(V, F) if self.EOTF == "sRGB" else np.power(V, F(self.gamma))
        return (F(self.u1) * f + F(self.y_black)).astype(F), oob


def _predict(name, photometry, k, capture=False):
    display, eotf, _, fov, C, N, fps, padding = CASES[name]
    test, ref, gaze = inputs(name)
    o = orc.Oracle(display, photometry=photometry, foveated=fov, temp_padding=padding, dtype=np.float64)
    if capture:
        o.capture = {}
    j, stats = o.predict(test[k:k + 1], ref[k:k + 1], "BCFHW", fps, fixation_point=gaze)
    return float(j), o


def jod(name, psi, k=0):
    eotf = CASES[name][1]
    v = dict(zip(NAMES, (float(x) for x in psi)))
    ph = orc.Photometry(v["Y_peak"], contrast=v["contrast"], EOTF=eotf, gamma=v["gamma"], E_ambient=v["E_ambient"],
                        k_refl=v["k_refl"], dtype=np.float64)
    return _predict(name, ph, k)[0]


@functools.lru_cache(maxsize=None)
def central_differences(name, k=0):
    """dJOD/dpsi [5] of pair k by central differences of the float64 oracle, step 1e-5 max(|psi_i|, 1)."""
    p = psi0(name)
    out = np.zeros(len(NAMES))
    for i in range(len(NAMES)):
        if NAMES[i] == "gamma" and CASES[name][1] != "gamma":
            continue                                 # no other model reads gamma: exactly 0
        h = 1e-5 * max(abs(p[i]), 1.0)
        pp, pm = p.copy(), p.copy()
        pp[i] += h
        pm[i] -= h
        out[i] = (jod(name, pp, k) - jod(name, pm, k)) / (2 * h)
    return out


def intermediates(name, psi):
    """(Y_black, u1, gamma) of psi."""
    Yp, c, E, kr, g = (float(x) for x in psi)
    yb = E / math.pi * kr + Yp / c
    return np.array([yb, Yp - yb if CASES[name][1] in SCALED else Yp, g])


@functools.lru_cache(maxsize=None)
def intermediate_differences(name, k=0):
    """U_fd [3] = dJOD/d(Y_black, u1, gamma) of pair k by central differences, step 1e-5 max(|u|, 1)."""
    eotf = CASES[name][1]
    u = intermediates(name, psi0(name))
    out = np.zeros(3)
    for j in range(3):
        if j == 2 and eotf != "gamma":
            continue
        h = 1e-5 * max(abs(u[j]), 1.0)
        up, um = u.copy(), u.copy()
        up[j] += h
        um[j] -= h
        out[j] = (_predict(name, _IntermediatePhotometry(eotf, *up), k)[0] -
                  _predict(name, _IntermediatePhotometry(eotf, *um), k)[0]) / (2 * h)
    return out


def jacobian(name, psi):
    """J [5, 3]: d(Y_black, u1, gamma) / dpsi_i."""
    Yp, c, E, kr, g = (float(x) for x in psi)
    dyb = np.array([1.0 / c, -Yp / (c * c), kr / math.pi, E / math.pi, 0.0])
    du1 = np.array([1.0, 0.0, 0.0, 0.0, 0.0]) - (dyb if CASES[name][1] in SCALED else 0.0)
    dg = np.array([0.0, 0.0, 0.0, 0.0, 1.0])
    return np.stack([dyb, du1, dg], axis=1)


def scale(name, k=0):
    """scale_i = sum_j |J_ij U_fd,j| [5]: what an error of entry i is relative to."""
    return np.abs(jacobian(name, psi0(name)) * intermediate_differences(name, k)[None, :]).sum(axis=1)


def weights(name):
    return STILL_WEIGHTS if CASES[name][5] == 0 else (1.0,)


def weighted(name, fn):
    """sum_k w_k fn(name, k) and sum_k |w_k| scale(name, k) over the pairs of the case."""
    w = weights(name)
    return sum(wk * fn(name, k) for k, wk in enumerate(w)), sum(abs(wk) * scale(name, k) for k, wk in enumerate(w))


def normalised(diff, sc):
    """|diff_i| / scale_i; an entry nothing depends on (scale_i == 0) must be exactly 0 and counts as 0."""
    diff, sc = np.asarray(diff, dtype=np.float64), np.asarray(sc, dtype=np.float64)
    assert np.all(diff[sc == 0] == 0), "an entry with no dependence must be exactly zero: %r" % (diff,)
    return np.where(sc > 0, np.abs(diff) / np.where(sc > 0, sc, 1.0), 0.0)


@functools.lru_cache(maxsize=None)
def clamp_counts(name, k=0):
    """(difference-map pixels at the d_max clamp, samples at a display clamp) of pair k in the float64 oracle."""
    display, eotf = CASES[name][:2]
    p = dict(zip(NAMES, psi0(name)))
    ph = orc.Photometry(p["Y_peak"], contrast=p["contrast"], EOTF=eotf, gamma=p["gamma"], E_ambient=p["E_ambient"],
                        k_refl=p["k_refl"], dtype=np.float64)
    _, o = _predict(name, ph, k, capture=True)
    d_clamped = sum(int((np.asarray(D) >= 1e4).sum()) for D in o.capture["D"])
    test, ref, _ = inputs(name)
    s_clamped = 0
    for a in (test[k], ref[k]):
        a = a.astype(np.float64)
        if eotf == "linear":
            s_clamped += int(((a <= 0.005) | (a >= p["Y_peak"])).sum())
        else:
            s_clamped += int(((a <= 0) | (a >= 1)).sum())
            if eotf == "PQ":
                L = orc.pq2lin(a, np.float64)
                s_clamped += int(((L <= 0.005) | (L >= p["Y_peak"])).sum())
    return d_clamped, s_clamped


@functools.lru_cache(maxsize=None)
def disagree():
    """The worst normalised difference between the helper's central differences and the golden over all cases and entries
    (reference-side data only), and the per-case values."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "g2x_display_grad.npz"))
    per_case = {}
    for name in GOLDEN_CASES:
        worst = 0.0
        for k in range(len(weights(name))):
            gold = g[name + "_grad"][k]
            have = ~np.isnan(gold)
            if CASES[name][1] == "PQ":
                assert [n for n, h in zip(NAMES, have) if h] == ["contrast", "E_ambient", "k_refl"]
            else:
                assert have.all()
            diff = np.where(have, central_differences(name, k) - np.where(have, gold, 0.0), 0.0)
            worst = max(worst, float(normalised(diff, scale(name, k)).max()))
            assert abs(jod(name, psi0(name), k) - g[name + "_jod"][k]) < 1e-4
        per_case[name] = worst
    return max(per_case.values()), per_case



# ---- what the sums entry points compute, in float64 from their fp32 arguments --------------------------------------------
def eotf_block(eotf, psi):
    """The fp32 members of the display block as the library receives and completes them: Y_peak, Y_black, gamma as fp32, and
    scale = Y_peak - Y_black in fp32."""
    Yp, c, E, kr, g = (float(x) for x in psi)
    yb = E / math.pi * kr + Yp / c
    yp32, yb32 = np.float32(Yp), np.float32(yb)
    return dict(kind=KINDS[eotf], Y_peak=yp32, Y_black=yb32, gamma=np.float32(g), scale=np.float32(yp32 - yb32))


def pq_luminance(v):
    """pq2lin of clamped fp32 samples in float64, with the constants the kernel has (fp32)."""
    f = np.float32
    m_inv, n_inv = np.float64(f(1.0) / f(78.84375)), np.float64(f(1.0) / f(0.1593017578125))
    c1, c2, c3 = 0.8359375, 18.8515625, 18.6875
    t = np.power(v, m_inv)
    r = np.maximum(t - c1, 0.0) / (c2 - c3 * t)
    return 10000.0 * np.power(r, n_inv)


def sens(V, e):
    """(a1, a2) float64 of fp32 samples V under the block e (eotf_display_sens): the kernel's fp32 constants, float64
    arithmetic."""
    f = np.float32
    V32 = np.asarray(V, dtype=f)
    V = V32.astype(np.float64)
    v = np.clip(V, 0.0, 1.0)
    a1, a2 = np.zeros_like(V), np.zeros_like(V)
    kind = e["kind"]
    if kind == KINDS["sRGB"]:
        hi = np.power((v + np.float64(f(0.055))) * np.float64(f(1.0) / f(1.055)), np.float64(f(2.4)))
        a1 = np.where(np.clip(V32, f(0), f(1)) > f(0.04045), hi, v * np.float64(f(1.0) / f(12.92)))
    elif kind == KINDS["gamma"]:
        pos = v > 0
        sv = np.where(pos, v, 1.0)
        a1 = np.where(pos, np.power(sv, np.float64(e["gamma"])), 0.0)
        a2 = np.where(pos, np.float64(e["scale"]) * a1 * np.log(sv), 0.0)
    elif kind == KINDS["PQ"]:
        a1 = (pq_luminance(v) > np.float64(e["Y_peak"])).astype(np.float64)
    elif kind == KINDS["linear"]:
        a1 = (V > np.float64(e["Y_peak"])).astype(np.float64)
    return a1, a2


def clip_margin(V, e):
    """Smallest relative distance of a sample's luminance from the upper clip (PQ, linear): the indicator a1 of a sample at
    the threshold would depend on the last bit of an fp32 power."""
    V = np.asarray(V, dtype=np.float64)
    if e["kind"] == KINDS["PQ"]:
        L = pq_luminance(np.clip(V, 0.0, 1.0))
    elif e["kind"] == KINDS["linear"]:
        L = V
    else:
        return np.inf
    return float(np.min(np.abs(L / np.float64(e["Y_peak"]) - 1.0)))


def video_s(g0, taps, widx, fl, N):
    """s[j] [N, HW] and the sum of its absolute elementary terms, float64: the temporal transpose of the window list.
    g0 [N, 2, HW] fp32, taps [2, fl] fp32, widx [N + fl - 1] (the head chosen by the padding, then frames 1 .. N - 1)."""
    g0 = np.asarray(g0, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    HW = g0.shape[2]
    s, sa = np.zeros((N, HW)), np.zeros((N, HW))
    for p in range(N + fl - 1):
        A, Aa = np.zeros(HW), np.zeros(HW)
        for k in range(fl):
            t = p - (fl - 1) + k
            if 0 <= t < N:
                for cc in range(2):
                    A += taps[cc, k] * g0[t, cc]
                    Aa += np.abs(taps[cc, k] * g0[t, cc])
        s[int(widx[p])] += A
        sa[int(widx[p])] += Aa
    return s, sa


def sums_of(s, sa, V, wgt, e):
    """(sums [3], sums of the absolute elementary terms [3]) float64.  s, sa [..., HW]; V [C, ..., HW] fp32 samples; wgt [C] fp32."""
    out, outa = np.zeros(3), np.zeros(3)
    for c in range(V.shape[0]):
        a1, a2 = sens(V[c], e)
        w = np.float64(np.float32(wgt[c]))
        for i, a in enumerate((np.ones_like(a1), a1, a2)):
            out[i] += (s * w * a).sum()
            outa[i] += (sa * np.abs(w * a)).sum()
    return out, outa


def window_indices(N, fl, padding):
    """The flat window index list [N + fl - 1] (oldest first) of the oracle's per-frame windows."""
    w = np.asarray(orc.window_frame_indices(N, fl, padding))
    return np.concatenate([w[0], w[1:, -1]]).astype(np.int64)
