"""Float64 (and, via dtype=, float32) restatement of the resized clips shown through frame maps, in plain numpy: the yardstick of
fvvdp_temporal_channels_resized_held and fvvdp_resize_grad_held (include/fvvdp_hip_resize_held.h).  TEST INFRASTRUCTURE: numpy
only, no GPU.  Built on resize_ref.py (the resize, its adjoint) and held_cases.py (the maps); neither is edited.

Forward:  the streams expanded with numpy's index_select, then resize_ref.resized_temporal_channels -- `forward`.  `forward_steps`
          restates what the KERNEL does instead: it walks the composed list of a stream position by position and takes the
          previous position's luminance whenever the entry repeats; with mutate= it does so wrongly, in the three ways the tests
          must be able to see.
Adjoint:  resize_ref.resize_adjoint applied per SOURCE frame to the run sum of gL over the display frames that show it -- `adjoint`.
"""
import copy

import numpy as np

import resize_ref as rref

F32, F64 = np.float32, np.float64


def run_table(m, F):
    """r [F + 1]: source frame j is shown by display frames [r[j], r[j + 1]) of the non-decreasing map m."""
    m = np.asarray(m)
    return np.searchsorted(m, np.arange(F + 1), side="left").astype(np.int64)


def expand(x, m):
    """index_select along the frames of a clip [C, F, h, w]."""
    return np.ascontiguousarray(np.asarray(x)[:, np.asarray(m)])


def forward(test, ref, m_t, m_r, size, mode, photometry, rgb2y, taps32, idx, dtype=F64):
    """(R, S) of resize_ref.resized_temporal_channels on the expanded streams; idx [N, fl]: the display-rate windows."""
    return rref.resized_temporal_channels(expand(test, m_t), expand(ref, m_r), size, mode, photometry, rgb2y, taps32, idx, dtype)


def forward_steps(test, ref, m_t, m_r, size, mode, photometry, rgb2y, taps32, widx, fl, dtype=F64, mutate=None):
    """R [N, 4, Ho, Wo] as the ingest kernel makes it: per stream the composed list m_s[widx] is walked once, a position whose
    entry equals the previous one takes the previous luminance, any other converts its frame.  mutate:
      "sticky"   the first position of the test's list whose entry CHANGES keeps the previous luminance all the same;
      "list0"    the reference reads the test's list (clamped into the reference's frames)."""
    F = dtype
    ph = copy.copy(photometry)
    ph.dtype = F
    taps = np.asarray(taps32, dtype=np.float32).astype(F)
    widx = np.asarray(widx)
    lists = [np.asarray(m_t)[widx], np.asarray(m_r)[widx]]
    if mutate == "list0":
        lists[1] = np.minimum(lists[0], ref.shape[1] - 1)
    lum = []
    for s, (clip, lst) in enumerate(zip((test, ref), lists)):
        out, sticky = [], mutate == "sticky" and s == 0
        for p, j in enumerate(lst):
            if p > 0 and j == lst[p - 1]:
                out.append(out[-1])
            elif p > 0 and sticky:
                out.append(out[-1])
                sticky = False
            else:
                out.append(rref.luminance(clip[:, int(j)], size, mode, ph, rgb2y, F))
        lum.append(out)
    N = len(widx) - fl + 1
    Wo, Ho = size
    R = np.zeros((N, 4, Ho, Wo), dtype=F)
    for f in range(N):
        R[f] = rref.orc.temporal_channels(np.stack(lum[0][f:f + fl], 0), np.stack(lum[1][f:f + fl], 0), taps, F)
    return R


def run_sums(gL, m, F, dtype=F64, absolute=False, drop_last=False):
    """[F, Ho, Wo]: gL [N, Ho, Wo] summed over each source frame's run, ascending, starting from the run's first frame (an empty
    run: zeros).  absolute: the sum of |gL|.  drop_last: the MUTATION whose run ends one display frame early."""
    r = run_table(m, F)
    g = np.asarray(gL, dtype=dtype)
    if absolute:
        g = np.abs(g)
    out = np.zeros((F,) + g.shape[1:], dtype=dtype)
    for j in range(F):
        lo, hi = int(r[j]), int(r[j + 1]) - (1 if drop_last else 0)
        if hi > lo:
            acc = g[lo].copy()
            for v in range(lo + 1, hi):
                acc = (acc + g[v]).astype(dtype)
            out[j] = acc
    return out


def adjoint(gL, test, m, size, mode, rgb2y, kind, dtype=F64, absolute=False, drop_last=False, **eotf):
    """The gradient [C, F, h, w] of the float clip test [C, F, h, w] shown through m, for the display-rate luminance gradient gL
    [N, Ho, Wo].  absolute: the same sums over the absolute values of their terms (one term per display frame, target sample and
    tap)."""
    F = test.shape[1]
    g = run_sums(gL, m, F, dtype, absolute, drop_last)
    return np.stack([rref.resize_adjoint(g[j], test[:, j], size, mode, rgb2y, kind, dtype=dtype, absolute=absolute, **eotf)
                     for j in range(F)], 1)


def hold_resize(x, m, size, mode):
    """The linear part of the forward, hold then resize: x [C, F, h, w] -> [C, N, Ho, Wo] in float64."""
    return rref.resize(expand(np.asarray(x, dtype=F64), m), size, mode)
