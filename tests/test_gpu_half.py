"""float16 / bfloat16 sources on the GPU.  Converting a half-precision sample to fp32 is exact, so the contract is exact too and
nothing here has a tolerance (the two oracle checks aside, which keep the project's JOD bound):
  forward    predict / predict_images / predict_image_pairs / predict_gazes on half input == the same call on the upcast input,
             bit for bit: JOD, Q_per_ch and the out-of-range flag, in every ingest kernel variant;
  oracle     one clip and one image against oracle/fvvdp_oracle.py on the upcast arrays (|dJOD| <= 1e-3), so
             that the new ingest is pinned to something other than its float sibling;
  gradients  .grad of a half leaf has the leaf's dtype and equals the float32 twin's gradient converted with torch's .to(dtype),
             bit for bit -- one rounding to nearest even, float16 subnormals kept;
  mixed      a half test with a float32 reference: the float32 kernels behind torch's cast node;
  memory     the tensors saved for backward are the half tensors.
Inputs: tests/grad_cases.py and tests/video_grad_cases.py, rounded to the dtype under test; x32 = x16.float() is the twin."""
import os
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_cases as ic                    # noqa: E402
import video_grad_cases as vc              # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HALF = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
F16_MIN_NORMAL = 6.1e-5                    # 2^-14 = 6.104e-5
SCALE = 1024.0


def _metric(display, padding="replicate", opt=None):
    opt = opt or {}
    kw = {}
    if "photometry" in opt:
        kw["display_photometry"] = fv.fvvdp_display_photo_eotf(**opt["photometry"])
    return fv.fvvdp(display_name=display, foveated=bool(opt.get("foveated")), temp_padding=padding, quiet=True, device=DEV, **kw)


_INPUTS = {}


def _clip(name, dtype):
    """(test, reference) [C, N, H, W] device tensors of a video case, rounded to dtype; computed once, never modified."""
    key = ("v", name, dtype)
    if key not in _INPUTS:
        t, r = vc.case_inputs(name)
        _INPUTS[key] = (torch.from_numpy(t).to(DEV).to(dtype), torch.from_numpy(r).to(DEV).to(dtype))
    return _INPUTS[key]


def _image(name, dtype):
    key = ("i", name, dtype)
    if key not in _INPUTS:
        t, r = ic.case_inputs(name)
        _INPUTS[key] = (torch.from_numpy(t).to(DEV).to(dtype), torch.from_numpy(r).to(DEV).to(dtype))
    return _INPUTS[key]


def _video_fix(name):
    return vc.case_gaze(name)


def _same_result(m, a16, b16, a32, b32, dim_order, fps, fix=None):
    """predict on the half pair and on its float32 twin: the whole result row (Q_per_ch | range flag | JOD) must be equal."""
    q16, s16 = m.predict(a16, b16, dim_order=dim_order, frames_per_second=fps, fixation_point=fix, sync=False)
    q32, s32 = m.predict(a32, b32, dim_order=dim_order, frames_per_second=fps, fixation_point=fix, sync=False)
    torch.cuda.synchronize()
    assert torch.equal(s16["result_buffer"].view(torch.int32), s32["result_buffer"].view(torch.int32))
    assert torch.equal(q16, q32) and torch.equal(s16["Q_per_ch"], s32["Q_per_ch"]) and torch.isfinite(q16).all()
    assert 0.0 < float(q16) < 10.0 and int(s16["range_flag"]) == int(s32["range_flag"])
    return float(q16), int(s16["range_flag"])


# ---- 1. forward, bit-identical --------------------------------------------------------------------------------------------
FORWARD_CASES = ["a_gray_30_replicate",         # 68x121, FL 8, PX 4
                 "b_rgb_60_circular",           # FL 16
                 "m_gray_120_pingpong_mod2",    # 69x122, H*W % 4 == 2, FL 32, PX 2
                 "k_gray_30_odd", "n_gray_120_odd",     # 67x121: the per-pixel ring
                 "q_rgb_256",                   # the 64-slot ring
                 "o_gray_240_replicate",        # the two-pass path through luminance_frames_kernel
                 "e_rgb_pq_oob",                # PQ, samples outside [0, 1], the flag set
                 "f_gray_linear",               # linear display, x400
                 "d_rgb_30_pingpong_fov"]       # foveated with a gaze trace


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
@pytest.mark.parametrize("name", FORWARD_CASES)
def test_predict_is_bit_identical_to_the_upcast_input(name, dtype):
    C, N, H, W, fps, padding, display, opt = vc.CASES[name]
    t16, r16 = _clip(name, dtype)
    m = _metric(display, padding, opt)
    q, flag = _same_result(m, t16, r16, t16.float(), r16.float(), "CFHW", fps, _video_fix(name))
    assert flag == (1 if opt.get("oob") else 0)
    print("%s %s: JOD %.6f, flag %d" % (name, dtype, q, flag))


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_predict_with_planes_that_are_only_2_byte_aligned(dtype):
    """RGB at 67x121: the odd channel stride leaves planes 1 and 2 of a half clip 2-byte aligned, whatever the base pointer."""
    g = torch.Generator().manual_seed(11)
    t16 = torch.rand((3, 5, 67, 121), generator=g).to(DEV).to(dtype)
    r16 = (t16.float() * 0.9 + 0.03).to(dtype)
    assert (t16[1].data_ptr() - t16.data_ptr()) % 4 == 2
    for fps in (30, 120):                       # FL 8 and FL 32
        _same_result(_metric("standard_4k"), t16, r16, t16.float(), r16.float(), "CFHW", fps)


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_predict_on_a_non_contiguous_bfhwc_view(dtype):
    t16, r16 = _clip("b_rgb_60_circular", dtype)                    # [C, N, H, W]
    tv = t16.permute(1, 2, 3, 0).contiguous()[None]                  # stored as BFHWC
    rv = r16.permute(1, 2, 3, 0).contiguous()[None]
    assert not tv.permute(0, 4, 1, 2, 3).is_contiguous()
    m = _metric("standard_4k", "circular")
    q, _ = _same_result(m, tv, rv, tv.float(), rv.float(), "BFHWC", 60)
    q2, _ = _same_result(m, t16, r16, t16.float(), r16.float(), "CFHW", 60)
    assert q == q2


# ---- 2. still images ------------------------------------------------------------------------------------------------------
IMAGE_CASES = ["a_gray_fhd", "b_rgb_4k_oob", "c_rgb_hdr_pq", "f_rgb_foveated"]


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
@pytest.mark.parametrize("name", IMAGE_CASES)
def test_predict_images_and_pairs_are_bit_identical(name, dtype):
    C, H, W, display, opt = ic.CASES[name]
    t16, r16 = _image(name, dtype)
    m = _metric(display, opt=opt)
    fix = opt.get("fix")
    # a stack of 3: the case, the case mirrored, the pair swapped
    T = torch.stack([t16, t16.flip(-1), r16])
    R = torch.stack([r16, r16.flip(-1), t16])
    fx = None if fix is None else np.asarray([fix] * 3, dtype=np.float32)
    q16, s16 = m.predict_images(T, R, fixation_point=fx)
    q32, s32 = m.predict_images(T.float(), R.float(), fixation_point=fx)
    assert torch.equal(q16, q32) and np.array_equal(s16["Q_per_ch"], s32["Q_per_ch"])
    assert np.array_equal(s16["range_flags"], s32["range_flags"])
    assert bool(s16["range_flags"][0]) == bool(opt.get("oob")) and len(set(q16.tolist())) >= 2
    # a list mixing a half and a float32 pair (grouped by shape and dtype)
    fl = None if fix is None else [fix, fix]
    out = m.predict_image_pairs([(t16, r16), (t16.flip(-1).float(), r16.flip(-1).float())], dim_order="CHW", fixation_points=fl)
    assert float(out[0][0]) == float(q32[0]) and float(out[1][0]) == float(q32[1])
    assert np.array_equal(out[0][1]["Q_per_ch"], s32["Q_per_ch"][0]) and out[0][1]["out_of_range"] == bool(opt.get("oob"))


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_predict_gazes_is_bit_identical(dtype):
    name = "d_rgb_30_pingpong_fov"
    C, N, H, W, fps, padding, display, opt = vc.CASES[name]
    t16, r16 = _clip(name, dtype)
    m = _metric(display, padding, opt)
    gaze = np.asarray([[20.0, 30.0], [60.5, 34.0], [110.0, 60.0]], dtype=np.float32)
    q16, s16 = m.predict_gazes(t16, r16, gaze, dim_order="CFHW", frames_per_second=fps)
    q32, s32 = m.predict_gazes(t16.float(), r16.float(), gaze, dim_order="CFHW", frames_per_second=fps)
    assert torch.equal(q16, q32) and np.array_equal(s16["Q_per_ch"], s32["Q_per_ch"]) and len(set(q16.tolist())) >= 2


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_calibration_is_bit_identical_with_and_without_temporal(dtype):
    """calibration_jod_images / calibration_jod_video on half sources, and with temporal= (whose luminance pass takes the clip
    upcast): JOD and the gradients for theta and phi equal the float32 twin's exactly."""
    name = "a_gray_30_replicate"
    C, N, H, W, fps, padding, display, opt = vc.CASES[name]
    t16, r16 = _clip(name, dtype)
    m = _metric(display, padding)
    out = []
    for t, r in ((t16.float(), r16.float()), (t16, r16)):
        theta = m.parameter_tensor().requires_grad_(True)
        phi = m.temporal_parameter_tensor().requires_grad_(True)
        jod = m.calibration_jod_video(t, r, theta, dim_order="CFHW", frames_per_second=fps, temporal=phi)
        jod.backward()
        ti, ri = t[:, 0][None], r[:, 0][None]
        th2 = m.parameter_tensor().requires_grad_(True)
        ji = m.calibration_jod_images(ti, ri, th2)
        ji.sum().backward()
        out.append((jod.detach(), theta.grad, phi.grad, ji.detach(), th2.grad))
    for a32, a16 in zip(out[0], out[1]):
        assert torch.equal(a32, a16) and torch.isfinite(a16).all()
    assert (out[1][1] != 0).any() and (out[1][2] != 0).all()


# ---- 3. against the oracle ------------------------------------------------------------------------------------------------
def test_float16_clip_and_image_against_the_oracle():
    from oracle import fvvdp_oracle as orc
    name = "a_gray_30_replicate"
    C, N, H, W, fps, padding, display, opt = vc.CASES[name]
    t16, r16 = _clip(name, torch.float16)
    q, _ = _metric(display, padding).predict(t16, r16, dim_order="CFHW", frames_per_second=fps)
    oq, _ = orc.Oracle(display, temp_padding=padding).predict(t16.float().cpu().numpy(), r16.float().cpu().numpy(), "CFHW", fps)
    print("clip: JOD %.6f, oracle %.6f" % (float(q), float(oq)))
    assert abs(float(q) - float(oq)) <= 1e-3
    name = "a_gray_fhd"
    C, H, W, display, opt = ic.CASES[name]
    t16, r16 = _image(name, torch.float16)
    q, _ = _metric(display).predict_images(t16[None], r16[None])
    oq, _ = orc.Oracle(display).predict(t16.float().cpu().numpy(), r16.float().cpu().numpy(), "CHW")
    print("image: JOD %.6f, oracle %.6f" % (float(q[0]), float(oq)))
    assert abs(float(q[0]) - float(oq)) <= 1e-3


# ---- 4. gradients ---------------------------------------------------------------------------------------------------------
def _leaves(t, r, wrt):
    x = t.clone().requires_grad_(wrt != "reference")
    y = r.clone().requires_grad_(wrt != "test")
    return x, y


def _check_grads(pairs, dtype):
    """pairs: (gradient of the half leaf, gradient of the float32 twin) for every leaf that requires grad."""
    for g16, g32 in pairs:
        assert g16 is not None and g32 is not None
        assert g16.dtype is dtype and g32.dtype is torch.float32 and g16.shape == g32.shape
        want = g32.to(dtype)
        assert torch.equal(g16.view(torch.int16), want.view(torch.int16)), \
            "%d of %d values differ" % (int((g16.view(torch.int16) != want.view(torch.int16)).sum()), g16.numel())
        assert torch.isfinite(g32).all() and (g32 != 0).any()


def _normal_share(g32, dtype, bound):
    """Share of the float32 gradient's entries that are float16 normal numbers; the condition that keeps a float16 comparison from
    being one of zeros and subnormals."""
    share = float((g32.abs() >= F16_MIN_NORMAL).float().mean())
    print("share of |g| >= 6.1e-5: %.4f" % share)
    if dtype is torch.float16 and bound is not None:
        assert share >= bound, share
    return share


IMAGE_GRAD_CASES = ["a_gray_fhd", "b_rgb_4k_oob", "e_rgb_gamma22", "f_rgb_foveated"]


def _image_grads(m, t, r, wrt, fix, scale):
    x, y = _leaves(t[None], r[None], wrt)
    jod = m.jod_images(x, y, fixation_point=fix, wrt=wrt)
    assert jod.dtype is torch.float32
    if scale == 1.0:
        jod.sum().backward()
    else:
        jod.sum().backward(torch.tensor(scale, device=DEV))
    return jod.detach(), {"test": [x.grad], "reference": [y.grad], "both": [x.grad, y.grad]}[wrt]


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
@pytest.mark.parametrize("wrt", ["test", "reference", "both"])
@pytest.mark.parametrize("name", IMAGE_GRAD_CASES)
def test_jod_images_gradient_is_the_float32_gradient_rounded_once(name, wrt, dtype):
    C, H, W, display, opt = ic.CASES[name]
    t16, r16 = _image(name, dtype)
    m = _metric(display, opt=opt)
    fix = opt.get("fix")
    j32, g32 = _image_grads(m, t16.float(), r16.float(), wrt, fix, SCALE)
    if name == "a_gray_fhd" and wrt != "reference":
        _normal_share(g32[0], dtype, 0.95)
    j16, g16 = _image_grads(m, t16, r16, wrt, fix, SCALE)
    assert torch.equal(j16, j32) and len(g16) == len(g32) == (2 if wrt == "both" else 1)
    _check_grads(zip(g16, g32), dtype)
    if opt.get("oob") and wrt != "reference":       # samples the display model clamps: exact zeros
        t = t16.float()
        oob = (t < 0) | (t > 1)
        assert oob.any() and (g16[0][0][oob] == 0).all() and (g16[0][0][~oob] != 0).any()


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_jod_images_unscaled_gradient_keeps_float16_subnormals(dtype):
    """Without loss scaling part of the float16 result is subnormal: it must still be the float32 gradient rounded to nearest
    even, not flushed to zero."""
    C, H, W, display, opt = ic.CASES["a_gray_fhd"]
    t16, r16 = _image("a_gray_fhd", dtype)
    m = _metric(display)
    _, g32 = _image_grads(m, t16.float(), r16.float(), "test", None, 1.0)
    _, g16 = _image_grads(m, t16, r16, "test", None, 1.0)
    _check_grads(zip(g16, g32), dtype)
    a = g32[0].abs()
    sub = (a < F16_MIN_NORMAL) & (a >= 2.0 ** -25)         # rounds to a non-zero float16 subnormal
    print("float16-subnormal share of the unscaled gradient: %.4f" % float(sub.float().mean()))
    if dtype is torch.float16:
        assert sub.any() and (g16[0][sub] != 0).all()
    # the scaled backward is the unscaled one times 1024 in fp32, before the rounding
    _, g32s = _image_grads(m, t16.float(), r16.float(), "test", None, SCALE)
    assert torch.equal(g32s[0], g32[0] * SCALE)


VIDEO_GRAD_CASES = ["a_gray_30_replicate", "c_gray_30_circular", "l_gray_60_circular_odd", "m_gray_120_pingpong_mod2", "q_rgb_256",
                    "e_rgb_pq_oob"]


def _video_grads(m, t, r, fps, wrt, fix, scale):
    x, y = _leaves(t, r, wrt)
    jod = m.jod_video(x, y, dim_order="CFHW", frames_per_second=fps, fixation_point=fix, wrt=wrt)
    assert jod.dtype is torch.float32
    jod.backward(torch.tensor(scale, device=DEV))
    return jod.detach(), [x.grad, y.grad] if wrt == "both" else [x.grad]


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
@pytest.mark.parametrize("wrt", ["test", "both"])
@pytest.mark.parametrize("name", VIDEO_GRAD_CASES)
def test_jod_video_gradient_is_the_float32_gradient_rounded_once(name, wrt, dtype):
    C, N, H, W, fps, padding, display, opt = vc.CASES[name]
    t16, r16 = _clip(name, dtype)
    m = _metric(display, padding, opt)
    j32, g32 = _video_grads(m, t16.float(), r16.float(), fps, wrt, None, SCALE)
    if name == "a_gray_30_replicate":
        _normal_share(g32[0], dtype, 0.90)
    j16, g16 = _video_grads(m, t16, r16, fps, wrt, None, SCALE)
    assert torch.equal(j16, j32)
    _check_grads(zip(g16, g32), dtype)
    if opt.get("oob"):
        t = t16.float()
        oob = (t < 0) | (t > 1)
        assert oob.any() and (g16[0][oob] == 0).all() and (g16[0][~oob] != 0).any()
    if name == "c_gray_30_circular":                # the frame no window shows
        for g in g16:
            assert (g[:, 0] == 0).all() and (g[:, 1:] != 0).any()


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_jod_gazes_gradient_is_the_float32_gradient_rounded_once(dtype):
    name = "d_rgb_30_pingpong_fov"
    C, N, H, W, fps, padding, display, opt = vc.CASES[name]
    t16, r16 = _clip(name, dtype)
    m = _metric(display, padding, opt)
    gaze = np.asarray([[20.0, 30.0], [60.5, 34.0], [110.0, 60.0]], dtype=np.float32)
    out = []
    for t, r in ((t16.float(), r16.float()), (t16, r16)):
        x = t.clone().requires_grad_(True)
        jod = m.jod_gazes(x, r, gaze, dim_order="CFHW", frames_per_second=fps)
        assert jod.dtype is torch.float32 and tuple(jod.shape) == (3,)
        jod.backward(torch.tensor([SCALE, 0.5 * SCALE, 2.0 * SCALE], device=DEV))
        out.append((jod.detach(), x.grad))
    assert torch.equal(out[0][0], out[1][0])
    _check_grads([(out[1][1], out[0][1])], dtype)


# ---- 5. mixed pair ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_mixed_pair_takes_the_float32_kernels_behind_a_cast(dtype):
    C, H, W, display, opt = ic.CASES["a_gray_fhd"]
    t16, r16 = _image("a_gray_fhd", dtype)
    r32 = r16.float()
    m = _metric(display)
    x16 = t16[None].clone().requires_grad_(True)
    j16 = m.jod_images(x16, r32[None])
    j16.sum().backward(torch.tensor(SCALE, device=DEV))
    x32 = t16[None].float().requires_grad_(True)
    j32 = m.jod_images(x32, r32[None])
    j32.sum().backward(torch.tensor(SCALE, device=DEV))
    assert torch.equal(j16, j32) and j16.dtype is torch.float32
    assert "ToCopy" in type(j16.grad_fn.next_functions[0][0]).__name__                 # torch's cast node sits in between
    _check_grads([(x16.grad, x32.grad)], dtype)


# ---- 6. memory ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_the_tensors_saved_for_backward_are_the_half_tensors(dtype):
    C, N, H, W, fps, padding, display, opt = vc.CASES["a_gray_30_replicate"]
    assert (N, H, W) == (12, 68, 121)
    t16, r16 = _clip("a_gray_30_replicate", dtype)
    x = t16[None].clone().requires_grad_(True)                      # contiguous on the device: saved as it is
    jod = _metric(display, padding).jod_video(x, r16[None], dim_order="BCFHW", frames_per_second=fps)
    assert "JodVideoFunction" in type(jod.grad_fn).__name__
    saved = jod.grad_fn.saved_tensors
    assert saved[0].dtype is dtype and saved[1].dtype is dtype and saved[0].data_ptr() == x.data_ptr()
    assert saved[0].numel() * saved[0].element_size() == 2 * N * H * W and saved[2].dtype is torch.float32      # Q_per_ch
