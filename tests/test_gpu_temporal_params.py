"""Gradients with respect to sustained_sigma and sustained_beta on the GPU (calibration_jod_video(temporal=...)): the tap-gradient
kernel alone against float64 numpy, fvvdp_luminance_frames against the oracle, dJOD/dtaps and dJOD/dphi end to end against central
differences of the float64 oracle, the forward bit for bit against predict, theta's gradient with and without phi, the backward
batching, phi's dtype and device, reuse of the native context, degenerate inputs and a short fit."""
import ctypes as C

import numpy as np
import pytest
import torch

import temporal_grad_ref as ref
from temporal_grad_ref import orc

pytestmark = pytest.mark.gpu

# The kernel's bound per entry: C_CHAIN 2^-24 sum |g0 Y|.  A lane adds the products of an entry with fused multiply-adds (the
# product is not rounded: ONE rounding per term) into an fp32 sum that starts at 0 and moves to fp64 after TG_CHAIN = 16 terms (2
# clips x PX pixels x 16 / (2 PX) frames), so the longest chain of fp32 roundings behind an output is 16: the error of such a sum
# is at most gamma_16 = 16 u / (1 - 16 u) times the sum of the absolute terms, u = 2^-24.  The conversion to fp64 is exact; the
# fp64 adds behind an entry (per lane, 6 shuffle steps, 4 waves, the partials of the workgroups, the batches) add at most their
# count x 2^-53, below 2^-24 x 1e-4 for any clip that fits the device.  C_CHAIN = 17 covers gamma_16's second-order term and that.
C_CHAIN = 17
U = 2.0 ** -24

# dJOD/dtaps end to end: max |GPU - per-tap central differences of the float64 oracle| / max |differences|, measured on an MI355X
# (TAPS_MEASURED); the bound is 3 x that, the convention of test_gpu_params.py.  It covers the fp32 maps, Q_per_ch and level-0
# gradients of the GPU path against the float64 oracle.
TAPS_MEASURED = {"long_30": 1.29e-5, "gray_fov_60": 1.05e-6}
# dJOD/dphi: |GPU - central differences of the float64 oracle in phi| relative to sum_{cc,k} |fd_taps[cc][k] dtaps[cc][k]/dphi_i|
# (both factors from the oracle), the worse of the two entries, measured per case on an MI355X; the bound is 3 x that.
PHI_MEASURED = {"rgb_u8_30": 4.41e-7, "gray_fov_60": 1.27e-7, "hdr_pq_30": 1.02e-5, "long_30": 6.76e-6, "circular_30": 1.59e-5,
                "pingpong_30": 4.62e-6, "gray_120": 4.42e-7}


def bound3(measured):
    assert measured is not None, "no MI355X measurement recorded for this case"
    return 3 * measured


@pytest.fixture(scope="module")
def fv():
    import fovvideovdp_amd
    from fovvideovdp_amd import _native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _native.lib()
    return fovvideovdp_amd


DEV = torch.device("cuda:0")
_METRICS = {}


def metric_of(fv, name):
    display, fov, pad = ref.CASES[name][0], ref.CASES[name][1], ref.CASES[name][8]
    if (display, fov, pad) not in _METRICS:
        _METRICS[(display, fov, pad)] = fv.fvvdp(display_name=display, foveated=fov, temp_padding=pad, device=DEV, quiet=True)
    return _METRICS[(display, fov, pad)]


def call(m, name, theta, temporal, **kw):
    test, rf, gaze = ref.inputs(name)
    return m.calibration_jod_video(test, rf, theta, dim_order="BCFHW", frames_per_second=ref.CASES[name][6], fixation_point=gaze,
                                   temporal=temporal, **kw)


# ---- the kernel alone ----------------------------------------------------------------------------------------------------------
def shifted(a, off):
    """A device copy of `a` whose first element sits `off` floats past a 256-byte boundary."""
    buf = torch.empty(a.size + 64, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 256 == 0
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v, buf


def run_kernel(G, G_r, Y_T, Y_R, pos, fl, off=0):
    from fovvideovdp_amd import _native as nat
    lib = nat.lib()
    n, _, H, W = G.shape
    dev = [shifted(np.ascontiguousarray(a, dtype=np.float32), off) for a in (G, G_r, Y_T, Y_R)]
    nbytes = C.c_size_t(0)
    nat.check(lib.fvvdp_tap_grad_workspace(W, H, fl, C.byref(nbytes)))
    work = torch.empty(nbytes.value // 8 + 32, dtype=torch.float64, device=DEV)
    out = torch.full((2, fl), float("nan"), dtype=torch.float64, device=DEV)
    pos = np.ascontiguousarray(pos, dtype=np.int32)
    assert len(pos) == fl - 1 + n
    nat.check(lib.fvvdp_tap_grad(W, H, n, fl, *[C.c_void_p(d[0].data_ptr()) for d in dev], pos.ctypes.data_as(C.POINTER(C.c_int32)),
                                 Y_T.shape[0], C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()), nbytes.value, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def kernel_case(H, W, fl, n, pad, b0, seed, offsets=(0,)):
    from fovvideovdp_amd.fvvdp import window_frame_indices
    rng = np.random.default_rng(seed)
    N = b0 + n
    Y_T = rng.uniform(0.5, 200.0, (N, H, W)).astype(np.float32)
    Y_R = rng.uniform(0.5, 200.0, (N, H, W)).astype(np.float32)
    G = (rng.standard_normal((n, 2, H, W)) * 1e-3).astype(np.float32)             # signed
    G_r = (rng.standard_normal((n, 2, H, W)) * 1e-3).astype(np.float32)
    flat = window_frame_indices(N, fl, pad)
    pos = flat[b0:b0 + fl - 1 + n]
    want, mag = ref.tap_sums_ref(G, G_r, Y_T, Y_R, ref.windows(flat, n, fl, b0))
    worst = 0.0
    for off in offsets:
        got = run_kernel(G, G_r, Y_T, Y_R, pos, fl, off)
        again = run_kernel(G, G_r, Y_T, Y_R, pos, fl, off)
        assert got.tobytes() == again.tobytes()                                  # no atomics: bit-identical from run to run
        err = np.abs(got - want) / (U * mag)
        worst = max(worst, err.max())
        assert np.isfinite(got).all() and err.max() <= C_CHAIN, (H, W, fl, n, pad, b0, off, err.max(), np.argmax(err))
    return worst


@pytest.mark.parametrize("fl", [2, 7, 8, 9, 15, 16, 17, 30, 32, 33, 64])
def test_tap_grad_kernel_every_filter_length(fv, fl):
    """68 x 121 = 8228 pixels (4-pixel lanes, 9 workgroups, the last one partly empty): a batch shorter than the filter from the
    clip's start, and a longer one that starts at b0 = 2."""
    pads = ["replicate", "circular", "pingpong"]
    w = max(kernel_case(68, 121, fl, max(1, min(3, fl - 1)), pads[fl % 3], 0, 100 + fl),
            kernel_case(68, 121, fl, fl + 5, pads[(fl + 1) % 3], 2, 200 + fl))
    print("fl %d: worst error %.2f x 2^-24 sum|g0 Y|" % (fl, w))


@pytest.mark.parametrize("H,W", [(7, 9), (16, 16), (68, 121), (135, 240), (12, 107)])
@pytest.mark.parametrize("fl,pad", [(8, "circular"), (15, "pingpong"), (8, "replicate")])
def test_tap_grad_kernel_pixel_counts_and_paddings(fv, H, W, fl, pad):
    """63 pixels (1-pixel lanes, one partly filled wave), 256 (one wave of 4-pixel lanes), 8228, 32400 (32 workgroups) and
    1284 = 4 * 64 * 5 + 4 (one lane past five full waves); the three paddings; n < fl and n > fl; a batch at b0 > 0."""
    w = max(kernel_case(H, W, fl, fl - 3, pad, 0, H * W + fl), kernel_case(H, W, fl, fl + 4, pad, 3, H * W + fl + 1))
    print("%dx%d fl %d %s: worst error %.2f x 2^-24 sum|g0 Y|" % (H, W, fl, pad, w))


@pytest.mark.parametrize("H,W,fl", [(16, 16, 8), (135, 240, 15), (68, 121, 33)])
def test_tap_grad_kernel_variants_agree(fv, H, W, fl):
    """Pointers one float past a 16-byte boundary force the 1-pixel variant: it and the 4-pixel variant both lie within the same
    bound of the float64 sums (so within twice that of each other)."""
    w = kernel_case(H, W, fl, fl + 2, "replicate", 1, 7 * fl, offsets=(0, 1))
    print("%dx%d fl %d: worst error of both variants %.2f x 2^-24 sum|g0 Y|" % (H, W, fl, w))


# ---- luminance frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("display,dtype,C_ch", [("standard_4k", np.uint8, 3), ("standard_4k", np.uint16, 3), ("standard_4k", np.float32, 3),
                                                ("standard_4k", np.float32, 1), ("standard_hdr_pq", np.float32, 1),
                                                ("standard_hdr_pq", np.uint16, 3)])
def test_luminance_frames_against_the_oracle(fv, display, dtype, C_ch):
    """The per-stage tolerance of the temporal kernel: against the oracle's float64 luminance, relative to
    the luminance, at most 4 x max(the error of the oracle's own fp32 chain, 4 x 2^-24)."""
    m = fv.fvvdp(display_name=display, device=DEV, quiet=True)
    rng = np.random.default_rng(5)
    N, H, W = 5, 37, 53
    u = rng.uniform(0.0, 1.0, (2, 1, C_ch, N, H, W))
    if dtype == np.float32:
        a = u.astype(np.float32)
    else:
        top = 255 if dtype == np.uint8 else 65535
        a = np.rint(u * top).astype(dtype)
    test, rf = a[0], a[1]
    vs = fv.fvvdp_video_source_array(test, rf, 30, dim_order="BCFHW", display_photometry=m.display_photometry,
                                     color_space_name=m.color_space)
    with torch.cuda.device(DEV):
        pl = m._clip_plan(vs)
        frames = np.asarray([3, 0, 4], dtype=np.int32)
        out = torch.full((2, len(frames), H, W), float("nan"), dtype=torch.float32, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        pl.feeder.luminance(frames, out, flag, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    assert int(flag) == 0
    o64 = orc.Oracle(display, dtype=np.float64)
    o32 = orc.Oracle(display, dtype=np.float32)
    worst = e_ref = 0.0
    for s, arr in enumerate((test, rf)):
        for i, f in enumerate(frames):
            L64 = orc.frame_luminance(arr, int(f), o64.photometry, o64.rgb2y, np.float64)[0]
            L32 = orc.frame_luminance(arr, int(f), o32.photometry, o32.rgb2y, np.float32)[0]
            e_ref = max(e_ref, float((np.abs(L32.astype(np.float64) - L64) / L64).max()))
            worst = max(worst, float((np.abs(got[s, i] - L64) / L64).max()))
    bound = 4 * max(e_ref, 4 * U)
    print("%s %s C=%d: luminance error %.3e, the oracle's fp32 chain %.3e, bound %.3e" % (display, dtype.__name__, C_ch, worst, e_ref, bound))
    assert worst <= bound


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.TAP_CASES)
def test_tap_gradient_against_per_tap_central_differences(fv, name):
    from fovvideovdp_amd import param_grad as pg
    m = metric_of(fv, name)
    test, rf, gaze = ref.inputs(name)
    assert ref.clamped(name) == 0
    g = pg.tap_gradient(m, test, rf, m.parameter_tensor(), m.temporal_parameter_tensor(), frames_per_second=ref.CASES[name][6],
                        fixation_point=gaze)
    fd = ref.fd_taps(name)
    assert g.dtype == torch.float64 and tuple(g.shape) == fd.shape
    g = g.cpu().numpy()
    err = np.abs(g - fd).max() / np.abs(fd).max()
    print("%s: dJOD/dtaps max |GPU - differences| / max |differences| = %.3e (largest %.3e)" % (name, err, np.abs(fd).max()))
    for cc in range(2):
        print("  channel %d GPU         %s" % (cc, " ".join("% .4e" % v for v in g[cc])))
        print("  channel %d differences %s" % (cc, " ".join("% .4e" % v for v in fd[cc])))
    assert err <= bound3(TAPS_MEASURED[name])


@pytest.mark.parametrize("name", list(ref.CASES))
def test_phi_gradient_against_central_differences_of_the_float64_oracle(fv, name):
    m = metric_of(fv, name)
    assert ref.clamped(name) == 0                 # differences are meaningless where a pixel crosses the clamp inside the step
    fps = ref.CASES[name][6]
    phi = m.temporal_parameter_tensor().requires_grad_(True)
    assert np.array_equal(phi.detach().numpy(), ref.phi0())
    jod = call(m, name, m.parameter_tensor(), phi)
    assert jod.grad_fn is not None and abs(float(jod.detach()) - ref.jod_under(name)) < 1e-3
    jod.backward()
    g = phi.grad
    assert g.dtype == torch.float64 and g.device.type == "cpu" and g.shape == (2,) and torch.isfinite(g).all()
    fd = ref.fd_phi(name)
    J = ref.dtaps_dphi_fd(fps, orc.filter_len(fps), ref.phi0())
    scale = np.abs(ref.fd_taps(name)[:, :, None] * J).sum(axis=(0, 1))
    err = np.abs(g.numpy() - fd) / scale
    for i, n in enumerate(ref.NAMES):
        print("%-12s %-16s GPU % .9e  differences % .9e  scale %.3e  rel %.2e" % (name, n, g[i], fd[i], scale[i], err[i]))
    print("%s: worst relative error %.3e" % (name, err.max()))
    assert err.max() <= bound3(PHI_MEASURED[name])


def perturbed_theta(theta, seed=3):
    return theta * torch.from_numpy(1.0 + 0.03 * np.random.default_rng(seed).standard_normal(12))


@pytest.mark.parametrize("name", ["rgb_u8_30", "gray_fov_60", "pingpong_30"])
def test_forward_bits(fv, name):
    m = metric_of(fv, name)
    display, fov, pad = ref.CASES[name][0], ref.CASES[name][1], ref.CASES[name][8]
    test, rf, gaze = ref.inputs(name)
    fps = ref.CASES[name][6]
    th0, phi0 = m.parameter_tensor(), m.temporal_parameter_tensor()
    today = m.calibration_jod_video(test, rf, th0, dim_order="BCFHW", frames_per_second=fps, fixation_point=gaze)
    assert torch.equal(call(m, name, th0, None), today) and torch.equal(call(m, name, th0, phi0), today)
    assert torch.equal(call(m, name, th0, phi0.clone().requires_grad_(True)).detach(), today)
    from fovvideovdp_amd import param_grad as pg
    for theta, phi in ((perturbed_theta(th0), phi0 * torch.tensor([1.1, 0.9], dtype=torch.float64)),
                       (th0, (phi0 * torch.tensor([0.85, 1.2], dtype=torch.float64)).float())):
        other = fv.fvvdp(display_name=display, foveated=fov, temp_padding=pad, device=DEV, quiet=True)
        other.set_parameters(theta)
        other.set_temporal_parameters(phi)
        want, st = other.predict(test, rf, dim_order="BCFHW", frames_per_second=fps, fixation_point=gaze)
        vs = fv.fvvdp_video_source_array(test, rf, fps, dim_order="BCFHW", display_photometry=m.display_photometry,
                                         color_space_name=m.color_space)
        with torch.cuda.device(DEV):
            jod, Q = pg._video_pass(m, vs, gaze, pg.theta_values(theta), False, pg.phi_values(phi))[:2]
        assert torch.equal(jod.cpu(), want.cpu()) and not torch.equal(want.cpu(), today.cpu())
        assert Q.cpu().numpy().tobytes() == np.ascontiguousarray(st["Q_per_ch"], dtype=np.float32).tobytes()
        assert torch.equal(call(m, name, theta, phi).cpu(), want.cpu())
        assert torch.equal(call(m, name, theta, phi.clone().requires_grad_(True)).detach().cpu(), want.cpu())
        assert torch.equal(m.parameter_tensor(), th0) and torch.equal(m.temporal_parameter_tensor(), phi0)


@pytest.mark.parametrize("name", ["rgb_u8_30", "gray_fov_60"])
def test_theta_gradient_is_bit_identical_with_and_without_phi(fv, name):
    m = metric_of(fv, name)
    phi0 = m.temporal_parameter_tensor()
    grads = []
    for temporal in (None, phi0, phi0.clone().requires_grad_(True)):
        theta = perturbed_theta(m.parameter_tensor(), 5).requires_grad_(True)
        call(m, name, theta, temporal).backward()
        grads.append(theta.grad.clone())
        if temporal is not None and temporal.requires_grad:
            assert torch.isfinite(temporal.grad).all() and (temporal.grad != 0).all()
    assert grads[0].numpy().tobytes() == grads[1].numpy().tobytes() == grads[2].numpy().tobytes()
    # ... and phi's gradient does not depend on whether theta requires grad
    a = phi0.clone().requires_grad_(True)
    call(m, name, perturbed_theta(m.parameter_tensor(), 5), a).backward()
    assert a.grad.numpy().tobytes() == temporal.grad.numpy().tobytes()


def test_backward_batching_phi_dtype_and_device(fv):
    """phi.grad under grad_batch = 2 against the whole clip: WITHIN THE KERNEL'S BOUND, not bit for bit -- the level-0 gradients and
    the luminance do not depend on the batching, the grouping of the kernel's fp32 sums (and of the fp64 adds) does."""
    from fovvideovdp_amd import param_grad as pg
    name = "long_30"
    m = metric_of(fv, name)
    test, rf, gaze = ref.inputs(name)
    fps = ref.CASES[name][6]
    th, phi0 = m.parameter_tensor(), m.temporal_parameter_tensor()

    def grad(phi):
        phi = phi.clone().requires_grad_(True)
        call(m, name, th, phi).backward()
        return phi.grad

    whole = grad(phi0)
    assert grad(phi0).numpy().tobytes() == whole.numpy().tobytes()                    # from run to run: bit for bit
    taps_whole, mag = pg.tap_gradient(m, test, rf, th, phi0, frames_per_second=fps, with_scale=True)
    assert getattr(m, "grad_batch", None) is None
    m.grad_batch = 2
    try:
        split = grad(phi0)
        taps_split = pg.tap_gradient(m, test, rf, th, phi0, frames_per_second=fps)
    finally:
        m.grad_batch = None
    mag = mag.cpu().numpy()
    d = np.abs(taps_split.cpu().numpy() - taps_whole.cpu().numpy())
    print("dJOD/dtaps, batches of 2 against the whole clip: worst %.2f x 2^-24 sum|g0 Y|" % (d / (U * mag)).max())
    assert (d <= 2 * C_CHAIN * U * mag).all()                                          # each side within the bound of the exact sums
    J = pg.taps_jacobian(float(fps), taps_whole.shape[1], float(phi0[0]), float(phi0[1]))[1].numpy()
    lim = (2 * C_CHAIN * U * mag[:, :, None] * np.abs(J)).sum(axis=(0, 1))
    print("phi.grad whole %s, batches of 2 %s, bound %s" % (whole.tolist(), split.tolist(), lim.tolist()))
    assert (np.abs(split.numpy() - whole.numpy()) <= lim).all()
    # phi as float32, and on the device: the gradient arrives in phi's dtype and on its device
    g32 = grad(phi0.float())
    assert g32.dtype == torch.float32 and g32.device.type == "cpu"
    p32 = phi0.float().double()
    assert torch.allclose(g32.double(), grad(p32), rtol=1e-6, atol=0)
    gd = grad(phi0.to(DEV))
    assert gd.dtype == torch.float64 and gd.device == DEV and gd.cpu().numpy().tobytes() == whole.numpy().tobytes()
    # an upstream gradient scales it
    phi = phi0.clone().requires_grad_(True)
    (call(m, name, th, phi) * -2.5).backward()
    assert torch.allclose(phi.grad, -2.5 * whole, rtol=1e-12, atol=0)


def test_context_is_reused_and_degenerate_inputs(fv):
    name = "long_30"
    m = metric_of(fv, name)
    test, rf, _ = ref.inputs(name)
    th, phi0 = m.parameter_tensor(), m.temporal_parameter_tensor()
    before, _ = m.predict(test, rf, dim_order="BCFHW", frames_per_second=30)
    ctx, filters = m._ctx, len(m._filters)
    assert ctx is not None
    key = ctx.key
    for k in range(3):                                     # a new phi per step: same context, no cache entry per phi
        phi = (phi0 * (1.0 + 0.05 * (k + 1))).requires_grad_(True)
        call(m, name, th, phi).backward()
        assert m._ctx is ctx and ctx.key == key and torch.isfinite(phi.grad).all()
    assert len(m._filters) == filters
    assert torch.equal(m.temporal_parameter_tensor(), phi0)
    after, _ = m.predict(test, rf, dim_order="BCFHW", frames_per_second=30)
    assert m._ctx is ctx and torch.equal(after.cpu(), before.cpu())
    # identical test and reference: exact zeros
    theta, phi = th.clone().requires_grad_(True), phi0.clone().requires_grad_(True)
    jod = m.calibration_jod_video(rf, rf, theta, frames_per_second=30, temporal=phi)
    assert float(jod.detach()) == 10
    jod.backward()
    assert (phi.grad == 0).all() and (theta.grad == 0).all()
    # a single frame has no temporal filter
    with pytest.raises(RuntimeError, match="single frame has no temporal filter"):
        m.calibration_jod_video(test[:, :, :1], rf[:, :, :1], th, frames_per_second=0, temporal=phi0)


def test_a_short_fit_moves_phi_towards_the_phi_that_made_the_targets(fv):
    """Two clips (replicate, 4K display, uint8 RGB and float gray), whose gradients point in different directions of the
    (ln sigma, ln beta) plane; plain Adam on ln phi from phi0 x (1.2, 0.8)."""
    names = ("rgb_u8_30", "long_30")
    phi0 = metric_of(fv, names[0]).temporal_parameter_tensor()
    with torch.no_grad():
        targets = [call(metric_of(fv, n), n, metric_of(fv, n).parameter_tensor(), phi0).double().cpu() for n in names]
    psi = torch.log(phi0 * torch.tensor([1.2, 0.8], dtype=torch.float64)).requires_grad_(True)
    opt = torch.optim.Adam([psi], lr=0.04)
    dist0 = float((psi.detach() - torch.log(phi0)).norm())
    losses = []
    for step in range(10):
        opt.zero_grad()
        phi = torch.exp(psi)
        loss = sum((call(metric_of(fv, n), n, metric_of(fv, n).parameter_tensor(), phi).double().cpu() - t) ** 2
                   for n, t in zip(names, targets))
        loss.backward()
        losses.append(float(loss))
        opt.step()
    dist = float((psi.detach() - torch.log(phi0)).norm())
    print("loss %.3e -> %.3e, |ln phi - ln phi0| %.4f -> %.4f, phi %s" % (losses[0], losses[-1], dist0, dist, torch.exp(psi).tolist()))
    assert losses[-1] < losses[0] and dist < dist0
