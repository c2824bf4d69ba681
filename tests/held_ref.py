"""Float64 reference of fvvdp_video_grad_input_held (include/fvvdp_hip_held.h), written from the FORWARD's definition and not from
the kernel, beside tests/video_grad_input_ref.py (whose display-model derivatives it uses).

Forward, per display frame v and temporal channel cc, `comp` the composed list of N + fl - 1 entries -- the display-rate window
list sent through the stream's frame map, comp[p] = m[widx[p]], every entry a SOURCE frame in [0, n_source):
    X_cc[v] = sum_k taps[cc][k] Lum[comp[v + fl - 1 - k]],      Lum[j] = sum_c w_c EOTF(V_c[j])
so with g0[v][cc] the gradient with respect to X_cc[v]
    dLum[j] = sum over positions p with comp[p] == j of sum_cc sum_k taps[cc][k] g0[p - (fl - 1) + k][cc]   (frames outside [0, N) dropped)
    grad_c[j] = w_c EOTF'(V_c[j]) dLum[j]
with `out` of n_source rows: a source frame no position shows keeps an exact zero."""
import numpy as np

import video_grad_input_ref as vref


def composed(m, widx):
    """The per-stream list handed to the ingest."""
    return np.asarray(m)[np.asarray(widx)]


def forward_matrix(comp, taps, N, n_source):
    """The temporal filter on the held stream as a dense matrix M [N, 2, n_source]: X[v][cc] = sum_j M[v][cc][j] Lum[j]."""
    taps = np.asarray(taps, dtype=np.float64)
    fl = taps.shape[1]
    assert len(comp) == N + fl - 1
    M = np.zeros((N, 2, n_source), dtype=np.float64)
    for v in range(N):
        for cc in range(2):
            for k in range(fl):
                M[v, cc, int(comp[v + fl - 1 - k])] += taps[cc, k]
    return M


def dlum(comp, taps, g0, n_source, absolute=False):
    """dLum [n_source, ...] in float64 from g0 [N, 2, ...] by the sum above.  absolute: the same sum over |tap * g0|."""
    taps = np.asarray(taps, dtype=np.float64)
    g0 = np.asarray(g0, dtype=np.float64)
    N, fl = g0.shape[0], taps.shape[1]
    assert len(comp) == N + fl - 1 and g0.shape[1] == 2
    assert min(int(c) for c in comp) >= 0 and max(int(c) for c in comp) < n_source
    if absolute:
        taps, g0 = np.abs(taps), np.abs(g0)
    out = np.zeros((n_source,) + g0.shape[2:], dtype=np.float64)
    for p in range(N + fl - 1):
        A = np.zeros(g0.shape[2:], dtype=np.float64)
        for k in range(fl):
            t = p - (fl - 1) + k
            if 0 <= t < N:
                A += taps[0, k] * g0[t, 0] + taps[1, k] * g0[t, 1]
        out[int(comp[p])] += A
    return out


def streaming_counts(m, n_source):
    """K_j: the streaming positions (display frames 1 .. N - 1) that show source frame j."""
    return np.bincount(np.asarray(m)[1:], minlength=n_source)


def head_shown(m, widx, fl, n_source):
    """bool [n_source]: the source frames that a position of the padding head shows."""
    out = np.zeros(n_source, bool)
    out[composed(m, widx)[:fl]] = True
    return out


def grad_input(comp, taps, g0, src, weights, kind, **eotf):
    """(grad, bound_scale) in float64 for g0 [N, 2, HW], src [C, n_source, HW] float32 and the C luminance weights."""
    d = vref.eotf_grad(src, kind, **eotf)
    w = np.asarray(weights, dtype=np.float32).astype(np.float64).reshape(-1, 1, 1)
    n_source = src.shape[1]
    return w * d * dlum(comp, taps, g0, n_source)[None], np.abs(w * d) * dlum(comp, taps, g0, n_source, absolute=True)[None]
