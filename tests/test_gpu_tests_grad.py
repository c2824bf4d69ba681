"""fvvdp.jod_tests on the GPU.  Every yardstick is existing code, never jod_tests itself:

    forward            predict_tests(tests, reference) and jod_video(tests[k], reference)              torch.equal
    wrt="tests"        the gradient of w_k * jod_video(tests[k], reference)                            torch.equal
    wrt="reference"    T = 1: the gradient of w_0 * jod_video(..., wrt="reference")                    torch.equal
                       T > 1: g_loop = sum_k (gradient of w_k * jod_video(..., wrt="reference")), the terms added in
                       float64 on the host                                                             REF_SUM_TOL
    C ABI              fvvdp_video_ref_grad_frames on the same maps                                    torch.equal

The T > 1 comparison: both paths evaluate the same per-test layer values and differ only in where the fp32 sum sits -- here
before the sweep, level 0, the temporal transpose and the display derivative, in the loop after them.  Its bound is, per case,
3 x the worst max|g - g_loop| / max|g_loop| measured on an MI355X over T in {2, 3, 4, 5, 9} (the project's convention), under
a cap of 5.3e-5, the tightest clip tolerance of tests/test_gpu_ref_grad.py.  Measured (MI355X, gfx950):
    rgb_4k   (RGB 250x131x5, standard_4k)      T = 2: 0 (one term that is not zero)   3: 1.74e-7   4: 1.74e-7   5: 1.30e-7   9: 2.13e-7
    rgb_pq   (RGB 250x131x5, standard_hdr_pq)  T = 2: 0                               3: 2.10e-7   4: 2.10e-7   5: 4.67e-7   9: 2.06e-7
    gray_4k  (gray 9x5x5, standard_4k)         T = 2: 0                               3: 8.62e-8   4: 8.62e-8   5: 6.88e-8   9: 1.73e-7
so REF_SUM_TOL = 3 x (2.128e-7, 4.665e-7, 1.725e-7).  The kernels repeat bit for bit, so the values do.  (T = 4 adds the test
that is identical to the reference to T = 3: exact zeros, the same figure.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd import grad_passes as gp
from fovvideovdp_amd import tests_grad as tg
from fovvideovdp_amd.synth import synth_video_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_multitest import H0, W0, _as, _degrade          # noqa: E402   the multitest suite's shape and degradations

pytestmark = pytest.mark.gpu

FPS = 30
CAP = 5.3e-5
# case -> (width, height, gray, display).  250x131 RGB: three strips at level 0, odd heights at several levels, a pixel count
# that is no multiple of the vector width.  9x5 gray: every band far below one 256-thread block.
CASES = {"rgb_4k": (W0, H0, False, "standard_4k"), "rgb_pq": (W0, H0, False, "standard_hdr_pq"), "gray_4k": (9, 5, True, "standard_4k")}
REF_SUM_TOL = {"rgb_4k": 6.4e-7, "rgb_pq": 1.4e-6, "gray_4k": 5.2e-7}
TS = [1, 2, 3, 4, 5, 9]
# test k of a case is _degrade(..., k): the generator's noisy test, a blur, the clip one frame late, the reference itself, then
# seeded noise of growing amplitude
IDENTICAL = 3
# seeded, of mixed sign, test 1 with an exact zero
WEIGHTS = np.random.default_rng(20).uniform(0.3, 2.0, 9) * np.array([1, 1, -1, 1, -1, 1, 1, -1, 1])
WEIGHTS[1] = 0.0
WEIGHTS = [float(np.float32(w)) for w in WEIGHTS]

_cache = {}


def _clips(case, dtype="float32"):
    W, H, gray, _ = CASES[case]
    key = ("clips", W, H, gray, dtype)
    if key not in _cache:
        t, r = synth_video_pair(5, H, W, pair=3)
        _cache[key] = ([_as(_degrade(t, r, k), dtype, gray).cuda() for k in range(9)], _as(r, dtype, gray).cuda())
    return _cache[key]


def _vgrad(m, t, r, w, wrt):
    """The gradient of w * jod_video(t, r) with respect to `wrt` ("test" or "reference"), and the JOD."""
    x = (t if wrt == "test" else r).clone().requires_grad_(True)
    jod = m.jod_video(x if wrt == "test" else t, r if wrt == "test" else x, frames_per_second=FPS, wrt=wrt)
    (jod * w).backward()
    return x.grad, jod.detach()


def _base(case):
    """(metric, tests, reference, per test: jod_video's JOD, the gradient of w_k JOD_k for the test and for the reference) of
    a case -- made once, never changed."""
    if ("base", case) not in _cache:
        tests, ref = _clips(case)
        m = fv.fvvdp(display_name=CASES[case][3])
        gt, gr, jod = [], [], []
        for k, t in enumerate(tests):
            g, j = _vgrad(m, t, ref, WEIGHTS[k], "test")
            gt.append(g)
            jod.append(j)
            gr.append(_vgrad(m, t, ref, WEIGHTS[k], "reference")[0])
        _cache[("base", case)] = (m, tests, ref, torch.stack(jod), gt, gr)
    return _cache[("base", case)]


def _run(m, tests, ref, wrt, T=None, weights=None, **kw):
    """jod_tests on fresh leaves and the backward of sum_k w_k JOD_k: (JOD, test gradients, reference gradient)."""
    T = len(tests) if T is None else T
    need_t, need_r = wrt in ("tests", "both"), wrt in ("reference", "both")
    xs = [t.clone().requires_grad_(need_t) for t in tests[:T]]
    y = ref.clone().requires_grad_(need_r)
    jod = m.jod_tests(xs, y, frames_per_second=FPS, wrt=wrt, **kw)
    w = torch.tensor((WEIGHTS if weights is None else weights)[:T], dtype=torch.float32, device=jod.device)
    (jod * w).sum().backward()
    return jod.detach(), [x.grad for x in xs], y.grad


def _g_loop(gr, T):
    acc = np.zeros(gr[0].shape, np.float64)
    for g in gr[:T]:
        acc += g.cpu().numpy().astype(np.float64)
    return acc


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("case", list(CASES))
def test_forward_equals_predict_tests_and_jod_video(case, T):
    m, tests, ref, jod, _, _ = _base(case)
    want, _ = m.predict_tests(tests[:T], ref, frames_per_second=FPS)
    plain = m.jod_tests(tests[:T], ref, frames_per_second=FPS)
    assert plain.grad_fn is None and plain.dtype is torch.float32 and plain.is_cuda and tuple(plain.shape) == (T,)
    assert torch.equal(plain, want) and torch.equal(plain, jod[:T])
    for wrt in tg.WRT:
        xs = [t.clone().requires_grad_(wrt != "reference") for t in tests[:T]]
        y = ref.clone().requires_grad_(wrt != "tests")
        got = m.jod_tests(xs, y, frames_per_second=FPS, wrt=wrt)
        assert got.grad_fn is not None and torch.equal(got.detach(), want), wrt


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("case", list(CASES))
def test_wrt_tests_equals_jod_video(case, T):
    m, tests, ref, jod, gt, _ = _base(case)
    got, grads, gy = _run(m, tests, ref, "tests", T)
    assert gy is None and torch.equal(got, jod[:T])
    for k in range(T):
        assert torch.equal(grads[k], gt[k]), k
        assert torch.isfinite(grads[k]).all()
    assert (gt[0] != 0).any()
    if T >= 2:
        assert (grads[1] == 0).all()                  # the zero weight
    if T > IDENTICAL:
        assert torch.equal(tests[IDENTICAL], ref) and (grads[IDENTICAL] == 0).all()          # the test identical to the reference


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("case", list(CASES))
def test_wrt_reference_against_the_loop(case, T):
    m, tests, ref, jod, _, gr = _base(case)
    got, grads, g = _run(m, tests, ref, "reference", T)
    assert all(x is None for x in grads) and torch.equal(got, jod[:T])
    assert g.dtype is torch.float32 and g.shape == ref.shape and torch.isfinite(g).all()
    if T == 1:
        assert torch.equal(g, gr[0]) and (g != 0).any()
        return
    # two of the per-test terms differ by more than 5 % of the larger one: the sum is one of different things
    far = 0.0
    for i in range(T):
        for j in range(i + 1, T):
            big = max(float(gr[i].abs().max()), float(gr[j].abs().max()))
            if big > 0:
                far = max(far, float((gr[i] - gr[j]).abs().max()) / big)
    assert far > 0.05
    loop = _g_loop(gr, T)
    err = float(np.abs(g.cpu().numpy().astype(np.float64) - loop).max() / np.abs(loop).max())
    print("%s T=%d: max|g - g_loop| / max|g_loop| = %.3e (bound %.3e, cap %.1e)" % (case, T, err, REF_SUM_TOL[case], CAP))
    assert REF_SUM_TOL[case] <= CAP
    assert err <= REF_SUM_TOL[case]


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("case", list(CASES))
def test_wrt_both_equals_the_two_single_sided_calls(case, T):
    m, tests, ref, jod, gt, _ = _base(case)
    _, _, g_ref = _run(m, tests, ref, "reference", T)
    got, grads, g = _run(m, tests, ref, "both", T)
    assert torch.equal(got, jod[:T]) and torch.equal(g, g_ref)
    for k in range(T):
        assert torch.equal(grads[k], gt[k]), k


def test_invariance():
    """Run to run, the backward batch, the launch groups, the map sets per layer call and the layout of the caller's tensors:
    none changes a bit."""
    m, tests, ref, jod, gt, _ = _base("rgb_4k")
    for T in (5, 9):
        _, t0, g0 = _run(m, tests, ref, "both", T)
        _, t1, g1 = _run(m, tests, ref, "both", T)
        assert torch.equal(g0, g1) and all(torch.equal(a, b) for a, b in zip(t0, t1))
        try:
            m.grad_batch = 2                          # three backward batches
            _, tb, gb = _run(m, tests, ref, "both", T)
            assert torch.equal(gb, g0) and all(torch.equal(a, b) for a, b in zip(tb, t0))
            m.grad_batch = None
            for cap in (1, 2, 4):
                tg.GROUP_MAX = cap
                assert torch.equal(_run(m, tests, ref, "reference", T)[2], g0), cap
            tg.GROUP_MAX = 0
            for sets in (1, 2, 3):                    # fewer map sets than tests: several layer calls per batch
                m.tests_grad_sets = sets
                _, ts_, gs = _run(m, tests, ref, "both", T)
                assert torch.equal(gs, g0) and all(torch.equal(a, b) for a, b in zip(ts_, t0)), sets
            m.tests_grad_sets, m.grad_batch = 3, 2
            assert torch.equal(_run(m, tests, ref, "reference", T)[2], g0)
        finally:
            tg.GROUP_MAX = 0
            m.grad_batch = m.tests_grad_sets = None
    # permuted-layout host tensors against the contiguous device ones; a test that does not require grad gets None
    T = 3
    _, t0, g0 = _run(m, tests, ref, "both", T)
    xs = [t[0].permute(1, 2, 3, 0).cpu().contiguous().requires_grad_(k != 1) for k, t in enumerate(tests[:T])]     # FHWC
    y = ref[0].permute(1, 2, 3, 0).cpu().contiguous().requires_grad_(True)
    j = m.jod_tests(xs, y, dim_order="FHWC", frames_per_second=FPS, wrt="both")
    (j * torch.tensor(WEIGHTS[:T], device=j.device)).sum().backward()
    assert torch.equal(j.detach(), jod[:T])
    assert xs[1].grad is None and y.grad.device.type == "cpu" and y.grad.shape == y.shape
    assert torch.equal(y.grad.permute(3, 0, 1, 2)[None].cuda(), g0)
    for k in (0, 2):
        assert torch.equal(xs[k].grad.permute(3, 0, 1, 2)[None].cuda(), t0[k]), k
    # double backward is refused
    yg = ref.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(m.jod_tests(tests[:2], yg, frames_per_second=FPS, wrt="reference").sum(), yg, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


@pytest.mark.parametrize("case", ["rgb_4k", "gray_4k"])
def test_c_abi_with_one_test_equals_the_single_test_entry_point(case):
    """fvvdp_tests_ref_grad_layer + _finish with one test on the maps of a map-writing pass against
    fvvdp_video_ref_grad_frames on the same maps; the outputs are pre-filled with NaN."""
    m, tests, ref, _, _, _ = _base(case)
    lib, t, dev = nat.lib(), tests[0], ref.device
    with torch.cuda.device(dev):
        s = gp.ClipSetup(m, t, FPS, ref)
        N, nb = s.N, s.N
        _, Q = gp.forward_clip(s, None)
        buf = gp.level0_buffers("test", m, s, t, nb, need_t=False, need_r=True)
        buf.maps_pass(lib, m, s, t, ref, None, 0, nb)
        prm = s.params()
        gamma = torch.tensor([WEIGHTS[0]], dtype=torch.float32, device=dev)
        buf.g0_r.fill_(float("nan"))
        gp.level0_backward(buf, s, prm, Q, N, 0, nb, gamma, need_t=False, need_r=True)
        want = buf.g0_r.clone()
        nbytes, work = gp.workspace(lib.fvvdp_tests_ref_grad_workspace, s.W, s.H, s.n_bands, nb, 1)
        work.fill_(float("nan"))
        g0 = torch.full_like(want, float("nan"))
        nat.check(lib.fvvdp_tests_ref_grad_layer(s.W, s.H, s.n_bands, nb, 1, 0, 1, 0, 0, C.byref(prm), C.byref(s.pp), gp._ptr(Q), N, 0,
                                                 gp._ptr(gamma), buf.maps.maps_arr, buf.maps.slopes, gp._ptr(work), nbytes, s.stream))
        nat.check(lib.fvvdp_tests_ref_grad_finish(s.W, s.H, s.n_bands, nb, 1, N, 0, gp._ptr(g0), gp._ptr(work), nbytes, s.stream))
        assert torch.isfinite(g0).all() and torch.isfinite(want).all() and (want != 0).any()
        assert torch.equal(g0, want)


def test_bfloat16_clips():
    """The forward is predict_tests' on the same tensors; the gradients arrive in bfloat16 and are the float32 gradients of the
    same call on the upcast inputs, rounded once."""
    tests, ref = _clips("rgb_4k", "bfloat16")
    T = 3
    m = fv.fvvdp(display_name="standard_4k")
    want, _ = m.predict_tests(tests[:T], ref, frames_per_second=FPS)
    j, gt, gr = _run(m, tests, ref, "both", T)
    assert torch.equal(j, want)
    assert gr.dtype is torch.bfloat16 and all(g.dtype is torch.bfloat16 for g in gt)
    j32, gt32, gr32 = _run(m, [t.float() for t in tests], ref.float(), "both", T)
    assert torch.equal(j32, j) and gr32.dtype is torch.float32
    assert torch.equal(gr, gr32.to(torch.bfloat16)) and (gr != 0).any()
    for k in range(T):
        assert torch.equal(gt[k], gt32[k].to(torch.bfloat16)), k
    # a mixed list: everything is upcast inside autograd's view, each gradient comes back in its tensor's dtype
    xs = [tests[0].clone().requires_grad_(True), tests[1].float().requires_grad_(True)]
    y = ref.clone().requires_grad_(True)
    jm = m.jod_tests(xs, y, frames_per_second=FPS, wrt="both")
    (jm * torch.tensor(WEIGHTS[:2], device=jm.device)).sum().backward()
    assert torch.equal(jm.detach(), j32[:2])
    assert xs[0].grad.dtype is torch.bfloat16 and xs[1].grad.dtype is torch.float32 and y.grad.dtype is torch.bfloat16
    assert torch.equal(xs[0].grad, gt32[0].to(torch.bfloat16)) and torch.equal(xs[1].grad, gt32[1])


def test_five_adam_steps_on_the_reference_raise_the_mean_jod():
    m, tests, ref, _, _, _ = _base("rgb_4k")
    three = [tests[0], tests[1], tests[2]]
    y = ref.clone().requires_grad_(True)
    # Adam's first steps move every sample by about lr whatever the gradient's size.  The tests lie a code value or so (4e-3)
    # from the reference: five steps of a twentieth of a code value stay where the mean JOD is close to linear in the samples
    opt = torch.optim.Adam([y], lr=1.0 / (255 * 20))
    seen = []
    for step in range(6):
        opt.zero_grad()
        mean = m.jod_tests(three, y, frames_per_second=FPS, wrt="reference").mean()
        seen.append(float(mean.detach()))
        if step == 5:
            break
        (-mean).backward()
        opt.step()
        with torch.no_grad():
            y.clamp_(0, 1)
    print("mean JOD over five Adam steps:", " ".join("%.4f" % q for q in seen))
    assert all(b > a for a, b in zip(seen, seen[1:])), seen
