"""Test helper (not part of the product): the float64 side of the tests of the temporal parameters' gradients.

  tap_sums_ref      out[cc][k] = sum_t sum_x (G[t][cc] Y_T[widx[t][fl-1-k]] + G_r[t][cc] Y_R[widx[t][fl-1-k]]) in float64 numpy:
                    what fvvdp_tap_grad computes (include/fvvdp_hip_taps.h), with the windows in the oracle's own form
  windows           the product's flat window index list -> the oracle's [N, fl] form (slot k oldest first)
  CASES / inputs    the end-to-end cases: the video cases of param_grad_ref plus longer clips, the other paddings and 120 fps
  jod_under         the JOD of Oracle(dtype=float64) on a case with sustained_sigma / sustained_beta overridden, or with the
                    taps themselves substituted
  fd_phi / fd_taps  central differences of that JOD in phi (step 1e-6 max(|phi|, 1)) and in every tap
Every oracle result is computed once per process and shared."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import fvvdp_oracle as orc          # noqa: E402
import param_grad_ref as pref                   # noqa: E402

NAMES = ("sustained_sigma", "sustained_beta")
D_MAX = 1e4


def phi0():
    return np.array([orc.load_defaults()["fvvdp_parameters.json"][n] for n in NAMES], dtype=np.float64)


def windows(flat, n, fl, b0=0):
    """The slice of the product's flat list (fl - 1 history entries, then the newest frame of every output) for output frames
    [b0, b0 + n) as the oracle's idx[n, fl]: slot k of output t is entry b0 + t + k, oldest first."""
    flat = np.asarray(flat)
    return np.stack([flat[b0 + t:b0 + t + fl] for t in range(n)], 0)


def tap_sums_ref(G, G_r, Y_T, Y_R, widx):
    """G, G_r [n, 2, ...] (gradient of the JOD for level 0's test / reference planes of n output frames), Y_T, Y_R [frames, ...]
    luminance frames, widx [n, fl] source frame of every window slot, oldest first (slot fl - 1 is the newest frame, weighted by
    tap 0) -> (out [2, fl], sum of the absolute terms [2, fl]) in float64."""
    G, G_r, Y_T, Y_R = (np.asarray(a, dtype=np.float64) for a in (G, G_r, Y_T, Y_R))
    n, fl = widx.shape
    out, mag = np.zeros((2, fl)), np.zeros((2, fl))
    for t in range(n):
        for k in range(fl):
            f = int(widx[t, fl - 1 - k])
            for cc in range(2):
                a, b = G[t, cc] * Y_T[f], G_r[t, cc] * Y_R[f]
                out[cc, k] += a.sum() + b.sum()
                mag[cc, k] += np.abs(a).sum() + np.abs(b).sum()
    return out, mag


# name: (display, foveated, C, frames, H, W, fps, dtype, padding); content as param_grad_ref.inputs
CASES = {
    "rgb_u8_30": pref.CASES["rgb_u8_30"] + ("replicate",),
    "gray_fov_60": pref.CASES["gray_fov_60"] + ("replicate",),
    "hdr_pq_30": pref.CASES["hdr_pq_30"] + ("replicate",),
    "long_30": ("standard_4k", False, 1, 12, 68, 121, 30, np.float32, "replicate"),
    "circular_30": ("standard_4k", False, 1, 5, 68, 121, 30, np.float32, "circular"),
    "pingpong_30": ("standard_4k", False, 3, 5, 68, 121, 30, np.float32, "pingpong"),
    "gray_120": ("standard_fhd", False, 1, 4, 68, 121, 120, np.float32, "replicate"),
}
TAP_CASES = ("long_30", "gray_fov_60")          # dJOD/dtaps end to end: one at 30 fps (N > fl), one foveated at 60 fps


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(test, reference) [1, C, F, H, W] and the gaze trace or None."""
    if name in pref.CASES:
        return pref.inputs(name)
    display, fov, C, N, H, W, fps, dt, pad = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 101)
    ref = rng.uniform(0.25, 0.75, (1, C, N, H, W))
    # the content changes over time (a drifting sinusoid) so that the transient channel is not noise alone
    ph = np.arange(N).reshape(1, 1, N, 1, 1) * 0.9 + np.arange(W).reshape(1, 1, 1, 1, W) * 0.15
    ref = np.clip(ref + 0.15 * np.sin(ph), 0.05, 0.95)
    test = ref + 0.04 * rng.standard_normal(ref.shape)
    test[..., : W // 2] = ref[..., : W // 2]
    test, ref = np.clip(test, 0, 1).astype(np.float32), np.clip(ref, 0, 1).astype(np.float32)
    return test, ref, None


def _oracle(name, prm=None, taps=None, capture=False):
    display, fov, C, N, H, W, fps, dt, pad = CASES[name]
    test, ref, gaze = inputs(name)
    o = orc.Oracle(display, foveated=fov, dtype=np.float64, temp_padding=pad)
    if prm is not None:
        o.prm = dict(o.prm, **prm)
    if capture:
        o.capture = {}
    own = orc.temporal_filters
    if taps is not None:
        orc.temporal_filters = lambda *a, **k: np.asarray(taps, dtype=np.float64)
    try:
        jod, stats = o.predict(test, ref, "BCFHW", fps, fixation_point=gaze)
    finally:
        orc.temporal_filters = own
    return o, float(jod), stats


def jod_under(name, phi=None, taps=None):
    prm = None if phi is None else dict(zip(NAMES, (float(phi[0]), float(phi[1]))))
    return _oracle(name, prm, taps)[1]


@functools.lru_cache(maxsize=None)
def clamped(name):
    """Pixels of the case's difference maps at the d_max clamp."""
    o = _oracle(name, capture=True)[0]
    return int(sum(int((np.asarray(D) >= D_MAX).sum()) for D in o.capture["D"]))


def taps64(name, phi=None):
    fps = CASES[name][6]
    p = phi0() if phi is None else phi
    return orc.temporal_filters(fps, p[0], p[1], orc.filter_len(fps), np.float64)


@functools.lru_cache(maxsize=None)
def fd_phi(name):
    """dJOD/dphi [2] by central differences of the float64 oracle, step 1e-6 max(|phi|, 1)."""
    p = phi0()
    out = np.zeros(2)
    for i in range(2):
        h = 1e-6 * max(abs(p[i]), 1.0)
        e = np.zeros(2)
        e[i] = h
        out[i] = (jod_under(name, p + e) - jod_under(name, p - e)) / (2 * h)
    return out


@functools.lru_cache(maxsize=None)
def fd_taps(name):
    """dJOD/dtaps [2, fl] by central differences of the float64 oracle in every tap (the others held), step 1e-6."""
    T = taps64(name)
    out = np.zeros_like(T)
    h = 1e-6
    for cc in range(2):
        for k in range(T.shape[1]):
            P, M = T.copy(), T.copy()
            P[cc, k] += h
            M[cc, k] -= h
            out[cc, k] = (jod_under(name, taps=P) - jod_under(name, taps=M)) / (2 * h)
    return out


def dtaps_dphi_fd(fps, fl, phi):
    """d taps / d phi [2, fl, 2] by central differences of the oracle's float64 temporal_filters."""
    J = np.zeros((2, fl, 2))
    for i in range(2):
        h = 1e-6 * max(abs(phi[i]), 1.0)
        e = np.zeros(2)
        e[i] = h
        p, m = phi + e, phi - e
        J[:, :, i] = (orc.temporal_filters(fps, p[0], p[1], fl, np.float64) -
                      orc.temporal_filters(fps, m[0], m[1], fl, np.float64)) / (2 * h)
    return J
