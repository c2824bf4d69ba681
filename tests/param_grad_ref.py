"""Test helper (not part of the product): the float64 side of the parameter-gradient tests.

  sums_from_maps        the five sums of include/fvvdp_hip_params.h in float64 numpy from a band's maps (the oracle's capture, or
                        the fp32 maps a GPU pass wrote)
  CASES / inputs        the content of the end-to-end cases: reference uniform in [0.25, 0.75], test = reference + 0.04 N(0, 1),
                        the left half identical (D = 0), one flat patch (both contrasts 0 around its centre: M = 0)
  oracle_case           Oracle(dtype=np.float64) on a case with its capture -> Q_per_ch, sums, pixels per band, clamped pixels
  central_differences   dJOD/dtheta by central differences of that oracle with o.prm overridden, step 1e-5 max(|theta|, 1)
Every oracle result is computed once per process and shared."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import fvvdp_oracle as orc          # noqa: E402

NAMES = ("mask_p", "mask_q_sust", "mask_q_trans", "mask_c", "sensitivity_correction", "beta",
         "beta_sch", "beta_tch", "beta_t", "w_transient", "jod_a", "log_jod_exp")
D_MAX = 1e4


def sums_from_maps(D, T, R, S, prm, cc, d_hi=D_MAX, gain=None, k_mask=None):
    """(s0..s4, sum of the absolute pixel terms of each) of one band plane.  D, T, R, S: arrays of one (band, channel, slot);
    T, R the band contrasts times the band multiplier, S the sensitivity before the gain.  A pixel is live where 0 < D < d_hi.
    gain, k_mask: the fp32 constants a kernel was given, in the place of 10^(sensitivity_correction / 20) and 10^mask_c."""
    D, T, R, S = (np.asarray(x, dtype=np.float64).ravel() for x in (D, T, R, S))
    g = 10.0 ** (prm["sensitivity_correction"] / 20.0) if gain is None else float(gain)
    k = 10.0 ** prm["mask_c"] if k_mask is None else float(k_mask)
    q = prm["mask_q_sust"] if cc == 0 else prm["mask_q_trans"]
    Tp, Rp = T * S * g, R * S * g
    u = np.abs(Tp - Rp)
    M = k * np.minimum(np.abs(Tp), np.abs(Rp))
    pos = D > 0
    live = pos & (D < d_hi)
    with np.errstate(divide="ignore", invalid="ignore"):
        Db = np.where(pos, np.power(np.where(pos, D, 1.0), prm["beta"]), 0.0)
        Dl = np.where(live, Db, 0.0)
        lnu = np.where(u > 0, np.log(np.where(u > 0, u, 1.0)), 0.0)
        lnM = np.where(M > 0, np.log(np.where(M > 0, M, 1.0)), 0.0)
        Mq = np.where(M > 0, np.power(np.where(M > 0, M, 1.0), q), 0.0)
        a = Mq / (1.0 + Mq)
        lnD = np.where(pos, np.log(np.where(pos, D, 1.0)), 0.0)
    terms = [Dl, Dl * lnu, Dl * a * lnM, Dl * a, Db * lnD]
    return np.array([t.sum() for t in terms]), np.array([np.abs(t).sum() for t in terms])


# name: (display, foveated, C, frames, H, W, fps, dtype); frames == 0: a stack of 3 still images
CASES = {
    "still_f32_stack": ("standard_4k", False, 3, 0, 68, 121, 0, np.float32),
    "rgb_u8_30": ("standard_4k", False, 3, 6, 135, 240, 30, np.uint8),
    "gray_fov_60": ("standard_fhd", True, 1, 4, 68, 121, 60, np.float32),
    "hdr_pq_30": ("standard_hdr_pq", False, 1, 3, 68, 121, 30, np.float32),
}
CPU_CASES = ("still_f32_stack", "rgb_u8_30", "gray_fov_60")


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(test, reference) [B, C, F, H, W] (B = 3 and F = 1 for the still stack, else B = 1) and the gaze trace or None."""
    display, fov, C, N, H, W, fps, dt = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 11)
    B, F = (3, 1) if N == 0 else (1, N)
    lo, hi, sd = (0.25, 0.75, 0.04) if name != "hdr_pq_30" else (0.30, 0.55, 0.01)
    ref = rng.uniform(lo, hi, (B, C, F, H, W))
    test = ref + sd * rng.standard_normal(ref.shape)
    test[..., : W // 2] = ref[..., : W // 2]                         # identical half: D = 0
    y0, x0 = H // 3, W // 2 + W // 8
    for a in (test, ref):
        a[..., y0:y0 + 24, x0:x0 + 24] = 0.5 if name != "hdr_pq_30" else 0.4     # flat patch: M = 0 (and D = 0) inside
    if dt == np.uint8:
        test, ref = np.clip(np.rint(test * 255), 0, 255).astype(np.uint8), np.clip(np.rint(ref * 255), 0, 255).astype(np.uint8)
    else:
        test, ref = np.clip(test, 0, 1).astype(np.float32), np.clip(ref, 0, 1).astype(np.float32)
    gaze = None
    if fov:
        gaze = np.stack([np.linspace(W * 0.3, W * 0.7, F), np.linspace(H * 0.6, H * 0.4, F)], 1).astype(np.float32)
    return test, ref, gaze


def _oracle(name, k, prm=None, capture=False):
    display, fov, C, N, H, W, fps, dt = CASES[name]
    test, ref, gaze = inputs(name)
    o = orc.Oracle(display, foveated=fov, dtype=np.float64)
    if prm is not None:
        o.prm = dict(o.prm, **prm)
    if capture:
        o.capture = {}
    jod, stats = o.predict(test[k:k + 1], ref[k:k + 1], "BCFHW", fps, fixation_point=gaze)
    return o, float(jod), stats


def theta0():
    return np.array([orc.load_defaults()["fvvdp_parameters.json"][n] for n in NAMES], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def oracle_case(name, k=0):
    """Pair k of the case -> dict(jod, Q [bands, 2, F], sums [bands, 2, F, 5], npx [bands], channels, clamped)."""
    o, jod, stats = _oracle(name, k, capture=True)
    Q = np.asarray(stats["Q_per_ch"], dtype=np.float64)
    nb, _, F = Q.shape
    channels = 1 if F == 1 else 2
    sums = np.zeros((nb, 2, F, 5))
    npx = np.zeros(nb)
    clamped = 0
    for f in range(F):
        bands = o.capture["bands"][f]
        for cc in range(channels):
            for b in range(nb):
                i = (f * channels + cc) * nb + b
                D, S = o.capture["D"][i], o.capture["S"][i]
                m = 1.0 if b == 0 else 2.0
                sums[b, cc, f] = sums_from_maps(D, bands[b][2 * cc] * m, bands[b][2 * cc + 1] * m, S, o.prm, cc)[0]
                npx[b] = D.size
                clamped += int((D >= D_MAX).sum())
    return dict(jod=jod, Q=Q, sums=sums, npx=npx, channels=channels, clamped=clamped)


@functools.lru_cache(maxsize=None)
def central_differences(name, k=0):
    """dJOD/dtheta [12] of pair k by central differences of the float64 oracle, step 1e-5 max(|theta|, 1)."""
    th = theta0()
    out = np.zeros(len(NAMES))
    for i, n in enumerate(NAMES):
        h = 1e-5 * max(abs(th[i]), 1.0)
        jp = _oracle(name, k, {n: th[i] + h})[1]
        jm = _oracle(name, k, {n: th[i] - h})[1]
        out[i] = (jp - jm) / (2 * h)
    return out


def planar_content(H, W, P, seed):
    """Temporal channels [P, H, W] fp32 (test / reference sustained, then test / reference transient for P = 4) for the sums
    kernel alone: the left half identical (D = 0), a patch where the reference planes are exactly 0 under a faint test
    (reference contrast exactly 0: M = 0 with D > 0), and a patch of full contrast in the test over a flat reference (pixels at the
    d_max clamp)."""
    rng = np.random.default_rng(seed)
    R = np.zeros((P, H, W), dtype=np.float32)
    ref = rng.uniform(20.0, 80.0, (H, W))
    test = ref + 2.0 * rng.standard_normal((H, W))
    y0, x0 = H // 8, W // 2 + 4
    ref[y0:y0 + 20, x0:x0 + 20] = 0.0
    test[y0:y0 + 20, x0:x0 + 20] = rng.uniform(0.0, 0.02, (20, 20))
    y1 = H // 2 + 2
    ref[y1:y1 + 28, x0:x0 + 40] = 50.0
    test[y1:y1 + 28, x0:x0 + 40] = 100.0 * ((np.add.outer(np.arange(28), np.arange(40)) // 6) % 2)
    test[:, : W // 2] = ref[:, : W // 2]
    R[0], R[1] = test, ref
    if P == 4:
        rt = 3.0 * rng.standard_normal((H, W))
        tt = rt + 0.5 * rng.standard_normal((H, W))
        rt[y0:y0 + 20, x0:x0 + 20] = 0.0
        tt[y0:y0 + 20, x0:x0 + 20] = rng.uniform(-0.01, 0.01, (20, 20))
        rt[y1:y1 + 28, x0:x0 + 40] = 0.0
        tt[y1:y1 + 28, x0:x0 + 40] = 60.0 * ((np.arange(40)[None, :] // 6) % 2) - 30.0
        tt[:, : W // 2] = rt[:, : W // 2]
        R[2], R[3] = tt, rt
    return R
