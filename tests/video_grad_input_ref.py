"""Float64 reference of fvvdp_video_grad_input (include/fvvdp_hip_video_grad.h), written from the FORWARD's definition and
not from the kernel: the transpose of the sliding-window temporal filter, and the derivative of each closed-form display model.
Shared by tests/test_video_grad_input_cpu.py (which checks it against the dense transpose and the oracle's temporal channels)
and tests/test_gpu_video_grad_input.py (which holds the kernel against it).

Forward, per output frame f and temporal channel cc, `idx` the window index list of N + fl - 1 entries:
    X_cc[f] = sum_k taps[cc][k] Lum[idx[f + fl - 1 - k]],      Lum[j] = sum_c w_c EOTF(V_c[j])
so with g0[f][cc] the gradient with respect to X_cc[f]
    dLum[j] = sum over positions p with idx[p] == j of sum_cc sum_k taps[cc][k] g0[p - (fl - 1) + k][cc]   (frames outside [0, N) dropped)
    grad_c[j] = w_c EOTF'(V_c[j]) dLum[j]
"""
import numpy as np

from fovvideovdp_amd import _native as nat

# PQ constants (SMPTE ST 2084), as oracle/fvvdp_oracle.py:pq2lin
PQ_N, PQ_M = 0.15930175781250000, 78.843750000000000
PQ_C1, PQ_C2, PQ_C3 = 0.83593750000000000, 18.851562500000000, 18.687500000000000
# The forward compares float32 samples with these constants in float32 (a float32 tensor against a Python scalar), so the
# thresholds a float32 sample meets are the float32 roundings
SRGB_KNEE = float(np.float32(0.04045))
L_FLOOR = float(np.float32(0.005))


def forward_matrix(idx, taps, N):
    """The temporal filter as a dense matrix M [N, 2, N]: X[f][cc] = sum_j M[f][cc][j] Lum[j]."""
    taps = np.asarray(taps, dtype=np.float64)
    fl = taps.shape[1]
    assert len(idx) == N + fl - 1
    M = np.zeros((N, 2, N), dtype=np.float64)
    for f in range(N):
        for cc in range(2):
            for k in range(fl):
                M[f, cc, int(idx[f + fl - 1 - k])] += taps[cc, k]
    return M


def dlum(idx, taps, g0, absolute=False):
    """dLum [N, ...] in float64 from g0 [N, 2, ...] by the sum above.  absolute: the same sum over |tap * g0|, the scale of
    the rounding error of any evaluation order."""
    taps = np.asarray(taps, dtype=np.float64)
    g0 = np.asarray(g0, dtype=np.float64)
    N, fl = g0.shape[0], taps.shape[1]
    assert len(idx) == N + fl - 1 and g0.shape[1] == 2
    if absolute:
        taps, g0 = np.abs(taps), np.abs(g0)
    out = np.zeros((N,) + g0.shape[2:], dtype=np.float64)
    for p in range(N + fl - 1):
        A = np.zeros(g0.shape[2:], dtype=np.float64)
        for k in range(fl):
            t = p - (fl - 1) + k
            if 0 <= t < N:
                A += taps[0, k] * g0[t, 0] + taps[1, k] * g0[t, 1]
        out[int(idx[p])] += A
    return out


def pq_inverse(L):
    """The code value in [0, 1] whose PQ luminance is L cd/m^2 (float64)."""
    y = np.power(np.asarray(L, dtype=np.float64) / 10000.0, PQ_N)
    return np.power((PQ_C1 + PQ_C2 * y) / (1.0 + PQ_C3 * y), PQ_M)


def pq_luminance(V):
    """pq2lin of display_model.py in float64, V clipped to [0, 1]."""
    V = np.clip(np.asarray(V, dtype=np.float64), 0.0, 1.0)
    t = np.power(V, 1.0 / PQ_M)
    return 10000.0 * np.power(np.maximum(t - PQ_C1, 0.0) / (PQ_C2 - PQ_C3 * t), 1.0 / PQ_N)


def eotf_grad(V, kind, Y_peak=0.0, Y_black=0.0, gamma=2.2, L_min=0.0, L_max=0.0):
    """dL/dV in float64 of fvvdp_display_photo_eotf.forward / fvvdp_display_photo_absolute.forward (display_model.py) at the
    float32 samples V; the parameters are the float32 values the kernel is given.  A clamp of the forward (V.clamp(0, 1),
    .clip(0.005, Y_peak), .clamp(L_min, L_max)) passes the gradient on where the value lies inside the closed range and gives
    an exact zero outside, as torch.clamp's backward."""
    V = np.asarray(V, dtype=np.float32).astype(np.float64)
    scale = float(np.float32(Y_peak)) - float(np.float32(Y_black))
    inside = (V >= 0.0) & (V <= 1.0)
    with np.errstate(all="ignore"):
        if kind == nat.EOTF_SRGB:
            hi = (2.4 / 1.055) * np.power((V + 0.055) / 1.055, 1.4)
            return np.where(inside, scale * np.where(V > SRGB_KNEE, hi, 1.0 / 12.92), 0.0)
        if kind == nat.EOTF_GAMMA:
            g = float(np.float32(gamma))
            return np.where(inside & (V > 0.0), scale * g * np.power(V, g - 1.0), 0.0)
        if kind == nat.EOTF_PQ:
            Vc = np.clip(V, 0.0, 1.0)
            t = np.power(Vc, 1.0 / PQ_M)
            den = PQ_C2 - PQ_C3 * t
            r = np.maximum(t - PQ_C1, 0.0) / den
            L = 10000.0 * np.power(r, 1.0 / PQ_N)
            d = L / (PQ_N * r) * ((PQ_C2 - PQ_C3 * PQ_C1) / (den * den)) * (t / (PQ_M * Vc))
            ok = inside & (V > 0.0) & (r > 0.0) & (L >= L_FLOOR) & (L <= float(np.float32(Y_peak)))
            return np.where(ok, d, 0.0)
        if kind == nat.EOTF_LINEAR:
            return np.where((V >= L_FLOOR) & (V <= float(np.float32(Y_peak))), 1.0, 0.0)
        if kind == nat.EOTF_ABSOLUTE:
            return np.where((V >= float(np.float32(L_min))) & (V <= float(np.float32(L_max))), 1.0, 0.0)
    raise ValueError("no closed form for display model kind %r" % (kind,))


def grad_input(idx, taps, g0, test, weights, kind, **eotf):
    """(grad, bound_scale) in float64 for g0 [N, 2, HW], test [C, N, HW] float32 and the C luminance weights: the gradient
    w_c EOTF'(V_c[j]) dLum[j] and |w_c EOTF'| times the same sum over |tap * g0|."""
    d = eotf_grad(test, kind, **eotf)
    w = np.asarray(weights, dtype=np.float32).astype(np.float64).reshape(-1, 1, 1)
    return w * d * dlum(idx, taps, g0)[None], np.abs(w * d) * dlum(idx, taps, g0, absolute=True)[None]
