"""Gradients with respect to the model parameters on the GPU (fvvdp.calibration_jod_images / calibration_jod_video): the
gradient against central differences of the float64 oracle on all twelve parameters, the forward bit for bit against
predict_images / predict / jod_images / jod_video, reuse of the native context, degenerate inputs, invariance under the backward
batching, the vector's dtype and device, and a short optimisation."""
import numpy as np
import pytest
import torch

import param_grad_ref as ref

pytestmark = pytest.mark.gpu

# Worst |GPU gradient - central differences of the float64 oracle| over the twelve parameters, relative to the sum of the absolute
# per-(band, channel, frame) terms of the entry (param_grad.chain(with_scale=True) on the oracle's arrays), measured per case on
# an MI355X: GRAD_MEASURED.  The bound is 3 x that (the convention of test_gpu_video_grad_input.py): it covers the fp32 maps and
# Q_per_ch of the GPU path against the float64 oracle, not a wrong term, which is off by orders of magnitude.  The worst entry is
# mask_q (sum D^beta a ln M: the largest cancellation among the sums) in every case; the PQ case, whose contrasts are the
# smallest (test - reference = 0.01 of the code range), sits an order of magnitude above the SDR ones.
GRAD_MEASURED = {"still_f32_stack": 1.87e-5, "rgb_u8_30": 1.01e-5, "gray_fov_60": 7.44e-6, "hdr_pq_30": 1.65e-4}
GRAD_BOUND = {k: 3 * v for k, v in GRAD_MEASURED.items()}


@pytest.fixture(scope="module")
def fv():
    import fovvideovdp_amd
    from fovvideovdp_amd import _native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _native.lib()
    return fovvideovdp_amd


_METRICS = {}


def metric_of(fv, name):
    display, fov = ref.CASES[name][:2]
    if (display, fov) not in _METRICS:
        _METRICS[(display, fov)] = fv.fvvdp(display_name=display, foveated=fov, device=torch.device("cuda:0"), quiet=True)
    return _METRICS[(display, fov)]


def call(m, name, theta):
    """The calibration entry point of the case under theta."""
    test, rf, gaze = ref.inputs(name)
    fps = ref.CASES[name][6]
    if ref.CASES[name][3] == 0:
        return m.calibration_jod_images(test[:, :, 0], rf[:, :, 0], theta, dim_order="BCHW")
    return m.calibration_jod_video(test, rf, theta, dim_order="BCFHW", frames_per_second=fps, fixation_point=gaze)


def gradient(m, name, theta, upstream=None):
    theta = theta.clone().requires_grad_(True)
    jod = call(m, name, theta)
    assert jod.grad_fn is not None
    if upstream is None:
        jod.sum().backward()
    else:
        (jod * torch.as_tensor(upstream, dtype=jod.dtype, device=jod.device)).sum().backward()
    return jod.detach(), theta.grad


UPSTREAM = {"still_f32_stack": [1.0, -0.5, 2.0]}


@pytest.mark.parametrize("name", list(ref.CASES))
def test_gradient_against_central_differences_of_the_float64_oracle(fv, name):
    from fovvideovdp_amd import param_grad as pg
    m = metric_of(fv, name)
    pairs = 3 if ref.CASES[name][3] == 0 else 1
    up = UPSTREAM.get(name, [1.0])
    fd, scale = np.zeros(12), np.zeros(12)
    for k in range(pairs):
        c = ref.oracle_case(name, k)
        assert c["clamped"] == 0                  # differences are meaningless where a pixel crosses the clamp inside the step
        _, sc = pg.chain(torch.from_numpy(c["Q"]), torch.from_numpy(c["sums"]), torch.from_numpy(c["npx"]), list(ref.theta0()),
                         c["channels"], c["channels"] == 1, with_scale=True)
        fd += up[k] * ref.central_differences(name, k)
        scale += abs(up[k]) * sc[0].numpy()
    theta = m.parameter_tensor()
    assert np.array_equal(theta.numpy(), ref.theta0())
    jod, g = gradient(m, name, theta, up if pairs > 1 else None)
    assert g.dtype == torch.float64 and g.device.type == "cpu" and g.shape == (12,) and torch.isfinite(g).all()
    for k in range(pairs):
        assert abs(float(jod.reshape(-1)[k]) - ref.oracle_case(name, k)["jod"]) < 1e-3
    g = g.numpy()
    worst, where = 0.0, None
    for i, n in enumerate(ref.NAMES):
        if scale[i] == 0:
            assert g[i] == 0, n
            continue
        err = abs(g[i] - fd[i]) / scale[i]
        print("%-16s %-24s GPU % .9e  differences % .9e  rel %.2e" % (name, n, g[i], fd[i], err))
        if err > worst:
            worst, where = err, (n, g[i], fd[i], scale[i])
    print("%s: worst relative error %.3e at %s" % (name, worst, where))
    assert worst <= GRAD_BOUND[name], where


def perturbed(theta, seed=3):
    rng = np.random.default_rng(seed)
    return theta * torch.from_numpy(1.0 + 0.03 * rng.standard_normal(12))


@pytest.mark.parametrize("name", ["still_f32_stack", "rgb_u8_30", "gray_fov_60"])
def test_forward_is_bit_identical_to_a_metric_that_holds_theta(fv, name):
    from fovvideovdp_amd import param_grad as pg
    m = metric_of(fv, name)
    display, fov = ref.CASES[name][:2]
    test, rf, gaze = ref.inputs(name)
    fps = ref.CASES[name][6]
    still = ref.CASES[name][3] == 0
    for theta in (m.parameter_tensor(), perturbed(m.parameter_tensor()), perturbed(m.parameter_tensor(), 4).float()):
        other = fv.fvvdp(display_name=display, foveated=fov, device=torch.device("cuda:0"), quiet=True)
        other.set_parameters(theta)
        vals = pg.theta_values(theta)
        with torch.cuda.device(m.device):
            if still:
                want, st = other.predict_images(test[:, :, 0], rf[:, :, 0], dim_order="BCHW")
                t, r = torch.from_numpy(test[:, :, 0]), torch.from_numpy(rf[:, :, 0])
                jod, Q, _ = pg._images_forward(m, t, r, None, vals, False)
                want_q = np.ascontiguousarray(st["Q_per_ch"][..., 0].transpose(1, 2, 0))
                diff = other.jod_images(torch.from_numpy(test[:, :, 0]), torch.from_numpy(rf[:, :, 0]), dim_order="BCHW")
            else:
                want, st = other.predict(test, rf, dim_order="BCFHW", frames_per_second=fps, fixation_point=gaze)
                vs = fv.fvvdp_video_source_array(test, rf, fps, dim_order="BCFHW", display_photometry=m.display_photometry,
                                                 color_space_name=m.color_space)
                jod, Q, _, _ = pg._video_forward(m, vs, gaze, vals, False)
                want_q = st["Q_per_ch"]
                diff = None
                if test.dtype == np.float32:
                    diff = other.jod_video(torch.from_numpy(test), torch.from_numpy(rf), dim_order="BCFHW", frames_per_second=fps,
                                           fixation_point=gaze)
        assert torch.equal(jod.cpu(), want.cpu()), (name, jod, want)
        assert Q.cpu().numpy().tobytes() == np.ascontiguousarray(want_q, dtype=np.float32).tobytes()
        plain = call(m, name, theta)
        assert plain.grad_fn is None and torch.equal(plain.cpu(), want.cpu())
        with_grad = call(m, name, theta.clone().requires_grad_(True))
        assert with_grad.grad_fn is not None and torch.equal(with_grad.detach().cpu(), want.cpu())
        if diff is not None:
            assert torch.equal(diff.detach().cpu(), want.cpu())
        assert torch.equal(m.parameter_tensor(), torch.from_numpy(ref.theta0()))


def test_context_is_reused_under_another_theta_and_left_as_it_was(fv):
    name = "rgb_u8_30"
    m = metric_of(fv, name)
    test, rf, _ = ref.inputs(name)
    before, _ = m.predict(test, rf, dim_order="BCFHW", frames_per_second=30)
    ctx = m._ctx
    assert ctx is not None
    key = ctx.key
    theta = perturbed(m.parameter_tensor(), 7)
    a = call(m, name, theta)
    assert m._ctx is ctx and ctx.key == key
    _, g = gradient(m, name, theta)
    assert m._ctx is ctx and ctx.key == key and torch.isfinite(g).all()
    assert not torch.equal(a.cpu(), before.cpu())
    bad = theta.clone()
    bad[1] = -1.0                                   # mask_q_sust: refused by the sums kernel's argument check, mid-call
    with pytest.raises(RuntimeError, match="positive"):
        gradient(m, name, bad)
    assert m._ctx is ctx and torch.equal(m.parameter_tensor(), torch.from_numpy(ref.theta0()))
    after, st = m.predict(test, rf, dim_order="BCFHW", frames_per_second=30)
    assert m._ctx is ctx
    fresh = fv.fvvdp(display_name="standard_4k", device=torch.device("cuda:0"), quiet=True)
    want, wst = fresh.predict(test, rf, dim_order="BCFHW", frames_per_second=30)
    assert torch.equal(after.cpu(), want.cpu()) and torch.equal(before.cpu(), want.cpu())
    assert st["Q_per_ch"].tobytes() == wst["Q_per_ch"].tobytes()


def test_degenerate_inputs(fv):
    m = metric_of(fv, "still_f32_stack")
    test, rf, _ = ref.inputs("still_f32_stack")
    theta = m.parameter_tensor().requires_grad_(True)
    jod = m.calibration_jod_images(rf[:, :, 0], rf[:, :, 0], theta, dim_order="BCHW")
    assert (jod == 10).all()
    jod.sum().backward()
    assert torch.isfinite(theta.grad).all() and (theta.grad == 0).all()
    theta = m.parameter_tensor().requires_grad_(True)
    jod = m.calibration_jod_video(np.repeat(rf[:1], 4, 2), np.repeat(rf[:1], 4, 2), theta, frames_per_second=30)
    assert float(jod.detach()) == 10
    jod.backward()
    assert torch.isfinite(theta.grad).all() and (theta.grad == 0).all()
    # a still image: the transient channel and the pooling over channels and frames do not exist
    _, g = gradient(m, "still_f32_stack", m.parameter_tensor())
    for i, n in enumerate(ref.NAMES):
        if n in ("mask_q_trans", "w_transient", "beta_t", "beta_tch"):
            assert g[i] == 0, n
        else:
            assert g[i] != 0 and torch.isfinite(g[i]), n
    # ... also as a one-frame clip
    theta = m.parameter_tensor().requires_grad_(True)
    one = m.calibration_jod_video(test[:1], rf[:1], theta, frames_per_second=0)
    assert abs(float(one) - float(call(m, "still_f32_stack", m.parameter_tensor())[0])) < 1e-5
    one.backward()
    for i, n in enumerate(ref.NAMES):
        assert (theta.grad[i] == 0) == (n in ("mask_q_trans", "w_transient", "beta_t", "beta_tch")), n


def test_gradient_does_not_depend_on_the_backward_batching_nor_on_the_run(fv):
    for name, frames in (("rgb_u8_30", 6), ("still_f32_stack", 3)):
        m = metric_of(fv, name)
        theta = perturbed(m.parameter_tensor(), 9)
        got = []
        try:
            for gb in (1, 2, frames, frames):
                m.grad_batch = gb
                got.append(gradient(m, name, theta, UPSTREAM.get(name))[1])
        finally:
            m.grad_batch = None
        for g in got[1:]:
            assert torch.equal(g, got[0]), (name, got)


def test_theta_on_the_host_or_the_device_in_float32_or_float64(fv):
    name = "gray_fov_60"
    m = metric_of(fv, name)
    theta = m.parameter_tensor()
    j64, g64 = gradient(m, name, theta)
    jd, gd = gradient(m, name, theta.to("cuda:0"))
    assert gd.device.type == "cuda" and gd.dtype == torch.float64
    assert torch.equal(gd.cpu(), g64) and torch.equal(jd, j64)          # the same values: the same bits
    j32, g32 = gradient(m, name, theta.float())
    assert g32.dtype == torch.float32 and g32.device.type == "cpu"
    _, g32d = gradient(m, name, theta.float().to("cuda:0"))
    assert g32d.dtype == torch.float32 and g32d.device.type == "cuda" and torch.equal(g32d.cpu(), g32)
    # theta rounded to fp32 moves every entry by at most 6e-8 relative; the gradient's own sensitivity to theta is of the order
    # of the gradient per unit of theta, so the two agree to a few fp32 roundings of the largest entry
    tol = 1e-5 * float(g64.abs().max())
    assert torch.allclose(g32.double(), g64, rtol=1e-5, atol=tol), (g32, g64)
    assert abs(float(j32) - float(j64)) < 1e-5


def test_adam_steps_on_two_parameters_lower_the_loss(fv):
    m = metric_of(fv, "still_f32_stack")
    test, rf, _ = ref.inputs("still_f32_stack")
    t, r = torch.from_numpy(test[:, :, 0]).to(m.device), torch.from_numpy(rf[:, :, 0]).to(m.device)
    base = m.parameter_tensor()
    i_c, i_s = ref.NAMES.index("mask_c"), ref.NAMES.index("sensitivity_correction")
    truth = base.clone()
    truth[i_c] -= 0.15
    truth[i_s] += 1.0
    target = m.calibration_jod_images(t, r, truth)
    phi = torch.tensor([float(base[i_c]), float(base[i_s])], dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([phi], lr=0.02)
    mask = torch.zeros(12, 2, dtype=torch.float64)
    mask[i_c, 0] = mask[i_s, 1] = 1.0
    rest = base.clone()
    rest[i_c] = rest[i_s] = 0.0
    losses = []
    for _ in range(8):
        opt.zero_grad()
        theta = rest + mask @ phi
        loss = ((m.calibration_jod_images(t, r, theta) - target) ** 2).mean()
        loss.backward()
        losses.append(float(loss))
        opt.step()
    print("losses", losses)
    assert losses[-1] < losses[0] and all(np.isfinite(losses))
    assert torch.equal(m.parameter_tensor(), base)
