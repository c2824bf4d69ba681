"""fvvdp.predict_held and fvvdp.jod_video_held on the GPU: the forward against predict on the index_select-expanded clips, bit for
bit; the gradient against jod_video's on the expanded clip with a derived bound, with exact zeros where they are due, bit-equal
across backward batches, runs and `wrt`; half precision against the float32 gradient rounded once; and the real reference's
autograd (tests/golden/g26_held_grad.npz) with the existing jod_video on the expanded clip as the yardstick."""
import os
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd.fvvdp import window_frame_indices

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import held_cases as hc                      # noqa: E402
import held_ref as href                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
TORCH = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
_metrics = {}


def metric(name):
    (W, H), C, fps, padding, dtype, ts, rs, N, opt = hc.ALL_CASES[name]
    key = (opt.get("display", "standard_fhd"), bool(opt.get("foveated")), padding)
    if key not in _metrics:
        _metrics[key] = fv.fvvdp(display_name=key[0], foveated=key[1], temp_padding=padding, quiet=True, device=DEV, heatmap=None)
    m = _metrics[key]
    m.batch_frames = opt.get("batch_frames")
    m.grad_batch = None
    return m


def as_input(x, dt, host=False):
    """numpy [C, F, H, W] -> what the case hands over: a numpy array for the integer types, a tensor of the float type."""
    if dt in ("uint8", "uint16"):
        return x if host else torch.from_numpy(x.view(np.int16) if dt == "uint16" else x).to(DEV)
    t = torch.from_numpy(x).to(TORCH[dt])
    return t if host else t.to(DEV)


def case_args(name):
    """(test, reference, kwargs of predict_held, frame axis of the arrays, the two maps)"""
    (W, H), C, fps, padding, dtype, ts, rs, N, opt = hc.ALL_CASES[name]
    dt_t, dt_r = dtype if isinstance(dtype, tuple) else (dtype, dtype)
    t, r = hc.case_inputs(name)
    t, r = as_input(t, dt_t, opt.get("host")), as_input(r, dt_r, opt.get("host"))
    order = opt.get("dim_order", "CFHW")
    if order == "FCHW":
        t, r = t.permute(1, 0, 2, 3).contiguous(), r.permute(1, 0, 2, 3).contiguous()
    kw = dict(dim_order=order, frames_per_second=fps, test_frames=hc.spec_arg(ts, N), reference_frames=hc.spec_arg(rs, N))
    gaze = hc.case_gaze(name)
    if gaze is not None:
        kw["fixation_point"] = gaze
    m_t, _, m_r, _ = hc.case_maps(name)
    return t, r, kw, order.index("F"), m_t, m_r


def expand(x, axis, m):
    if isinstance(x, np.ndarray):
        return np.take(x, m, axis=axis)
    return x.index_select(axis, torch.as_tensor(m, dtype=torch.int64, device=x.device))


def u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def tbits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype is torch.float32 else torch.int16).numpy()


# ---- 1. the forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_predict_held_is_predict_on_the_expanded_clips(name):
    m = metric(name)
    t, r, kw, axis, m_t, m_r = case_args(name)
    q, st = m.predict_held(t, r, **kw)
    pk = {k: v for k, v in kw.items() if k not in ("test_frames", "reference_frames")}
    q0, st0 = m.predict(expand(t, axis, m_t), expand(r, axis, m_r), **pk)
    print("%s: JOD %.6f" % (name, float(q)))
    assert 0 < float(q) < 10
    assert u32(float(q)) == u32(float(q0))
    assert st["Q_per_ch"].shape == st0["Q_per_ch"].shape and np.array_equal(u32(st["Q_per_ch"]), u32(st0["Q_per_ch"]))
    assert st["N_frames"] == len(m_t) == st0["N_frames"] and (st["width"], st["height"]) == (st0["width"], st0["height"])


def test_identity_maps_hand_over_to_predict():
    m = metric("k2")
    _, r = hc.case_inputs("k2")
    r = torch.from_numpy(r).to(DEV)
    t = (r * 0.9).contiguous()
    q, st = m.predict_held(t, r, dim_order="CFHW", frames_per_second=30, test_frames=list(range(r.shape[1])))
    q0, st0 = m.predict(t, r, dim_order="CFHW", frames_per_second=30)
    assert u32(float(q)) == u32(float(q0)) and np.array_equal(u32(st["Q_per_ch"]), u32(st0["Q_per_ch"]))


# ---- 2. the gradient ----------------------------------------------------------------------------------------------------------------
def held_grads(m, t, r, kw, wrt):
    """(JOD, grad of the test or None, grad of the reference or None)"""
    tt = t.detach().clone().requires_grad_(wrt in ("test", "both"))
    rr = r.detach().clone().requires_grad_(wrt in ("reference", "both"))
    q = m.jod_video_held(tt, rr, wrt=wrt, **kw)
    q.backward()
    return q.detach(), tt.grad, rr.grad


def expanded_grads(m, t, r, kw, axis, m_t, m_r, wrt):
    """jod_video's gradients on the expanded clips, per display frame (no sum over the copies)."""
    pk = {k: v for k, v in kw.items() if k not in ("test_frames", "reference_frames")}
    tt = expand(t, axis, m_t).detach().clone().requires_grad_(wrt in ("test", "both"))
    rr = expand(r, axis, m_r).detach().clone().requires_grad_(wrt in ("reference", "both"))
    q = m.jod_video(tt, rr, wrt=wrt, **pk)
    q.backward()
    return q.detach(), tt.grad, rr.grad


def check_against_expanded(name, g, gx, axis, mp, fl, padding):
    """g: the held gradient of one stream, gx: the expanded clip's per display frame (float32 both), mp: the stream's map.
    DERIVED: the level-0 gradients of the two backward passes have equal bits, so on a source frame j that no head position shows
    every g_v is one rounded product chain of one streaming term and g_j the same chain on the sum of n_j such terms:
        |g_j - sum_v g_v| <= (n_j + 2) 2^-24 sum_v |g_v|       (the sums in float64 over the display frames that show j)."""
    g = np.moveaxis(g.detach().cpu().numpy().astype(np.float64), axis, 0)
    gx = np.moveaxis(gx.detach().cpu().numpy().astype(np.float64), axis, 0)
    F, N = g.shape[0], gx.shape[0]
    head = href.head_shown(mp, window_frame_indices(N, fl, padding), fl, F)
    worst, checked, skipped = 0.0, 0, 0
    for j in range(F):
        vs = np.nonzero(mp == j)[0]
        if len(vs) == 0:                                   # a frame no display frame shows: exact zeros
            assert (g[j] == 0).all(), (name, j)
            skipped += 1
            continue
        s, sa = gx[vs].sum(axis=0), np.abs(gx[vs]).sum(axis=0)
        if head[j]:                                        # the numbers are the C-ABI test's; here: zeros where zeros are due
            assert (g[j][sa == 0] == 0).all(), (name, j)
            continue
        bound = (len(vs) + 2) * U * sa
        err = np.abs(g[j] - s)
        assert (err <= bound).all(), (name, j, float((err / np.maximum(bound, 1e-300)).max()))
        if (sa > 0).any():
            worst = max(worst, float((err[sa > 0] / bound[sa > 0]).max()))
        checked += 1
    print("%s: worst |g_j - sum g_v| / bound %.3f over %d frames (%d head-shown, %d never shown)" % (name, worst, checked, int(head.sum()), skipped))
    assert checked >= F // 2 - skipped
    return skipped


@pytest.mark.parametrize("name", hc.GRAD_CASES)
def test_jod_video_held_gradient(name):
    (W, H), C, fps, padding, dtype, ts, rs, N, opt = hc.ALL_CASES[name]
    m = metric(name)
    t, r, kw, axis, m_t, m_r = case_args(name)
    q, g, _ = held_grads(m, t, r, kw, "test")
    qp, _ = m.predict_held(t, r, **kw)
    assert u32(float(q)) == u32(float(qp))
    assert g.shape == t.shape and g.dtype == t.dtype and torch.isfinite(g.float()).all() and (g != 0).any()
    # half precision: the float32 gradient of the upcast input, rounded once
    t32, r32 = t.float(), r.float()
    if t.dtype is not torch.float32:
        q32, g32, _ = held_grads(m, t32, r32, kw, "test")
        assert u32(float(q32)) == u32(float(q))
        assert np.array_equal(tbits(g32.to(t.dtype)), tbits(g))
    else:
        g32 = g
    qx, gx, _ = expanded_grads(m, t32, r32, kw, axis, m_t, m_r, "test")
    assert u32(float(qx)) == u32(float(q))
    check_against_expanded(name, g32, gx, axis, m_t, hc.FL[fps], padding)
    # backward batches of 1, 2 and the default, and a second run: equal bits
    for gb in (1, 2, None, None):
        m.grad_batch = gb
        _, g2, _ = held_grads(m, t, r, kw, "test")
        assert np.array_equal(tbits(g2), tbits(g)), gb
    m.grad_batch = None


@pytest.mark.parametrize("name", ["skipref", "fchw", "k3"])
def test_gradients_with_respect_to_a_held_reference(name):
    (W, H), C, fps, padding, dtype, ts, rs, N, opt = hc.ALL_CASES[name]
    m = metric(name)
    t, r, kw, axis, m_t, m_r = case_args(name)
    t, r = t.float(), r.float()
    q, gt, _ = held_grads(m, t, r, kw, "test")
    qb, gtb, grb = held_grads(m, t, r, kw, "both")
    qr, none, gr = held_grads(m, t, r, kw, "reference")
    assert none is None and u32(float(q)) == u32(float(qb)) == u32(float(qr))
    assert np.array_equal(tbits(gtb), tbits(gt))                     # the test gradient is bit-identical whatever wrt
    assert np.array_equal(tbits(grb), tbits(gr)) and gr.shape == r.shape and (gr != 0).any()
    _, gxt, gxr = expanded_grads(m, t, r, kw, axis, m_t, m_r, "both")
    check_against_expanded(name + "/test", gtb, gxt, axis, m_t, hc.FL[fps], padding)
    skipped = check_against_expanded(name + "/reference", grb, gxr, axis, m_r, hc.FL[fps], padding)
    if name == "skipref":
        assert skipped >= 5                                          # the skipping map's frames: exact zeros, checked above


def test_identical_clips_give_ten_and_zeros():
    m = metric("k2")
    t, _ = hc.case_inputs("k2")
    for k in (2, 3):
        tt = torch.from_numpy(t).to(DEV).requires_grad_(True)
        ref = tt.detach().repeat_interleave(k, dim=1)
        q = m.jod_video_held(tt, ref, dim_order="CFHW", frames_per_second=30, test_frames=k)
        q.backward()
        assert float(q.detach()) == 10.0 and (tt.grad == 0).all() and tt.grad.shape == tt.shape


# ---- 3. the real reference's autograd -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hc.GOLDEN_CASES))
def test_against_the_reference_autograd(name):
    """No tolerance is fixed: the existing jod_video on the expanded clip, its gradient summed over the copies, is measured against
    the same golden in the same test, and the held path may be at most 3 times that figure (the project's standing margin)."""
    m = metric(name)
    t, r, kw, axis, m_t, m_r = case_args(name)
    jod_ref, g_ref = hc.load_golden(name)
    q, g, _ = held_grads(m, t, r, kw, "test")
    _, gx, _ = expanded_grads(m, t, r, kw, axis, m_t, m_r, "test")
    summed = torch.zeros_like(g).index_add_(axis, torch.as_tensor(m_t, dtype=torch.int64, device=g.device), gx)
    scale = float(np.abs(g_ref).max())
    held_fig = float(np.abs(g.cpu().numpy() - g_ref).max()) / scale
    exp_fig = float(np.abs(summed.cpu().numpy() - g_ref).max()) / scale
    print("%s: JOD %.5f (reference %.5f); max|g - g_ref| / max|g_ref|: held %.3e, jod_video on the expanded clip %.3e"
          % (name, float(q), jod_ref, held_fig, exp_fig))
    assert abs(float(q) - jod_ref) <= 1e-3                                          # the project's parity bound
    assert held_fig <= 3 * exp_fig
