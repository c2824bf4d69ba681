"""Half-precision sources without a GPU: float16 / bfloat16 arrays through the host-side sources, the refusals that name the
dtype, the C ABI of include/fvvdp_hip_half.h and its binding, and the code objects of the new kernel entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd.fvvdp import _image_pair, _image_stack, _sample_type
from fovvideovdp_amd.video_source import fvvdp_video_source_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF = [torch.float16, torch.bfloat16]


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def clip(dtype, C=3, F=4, H=9, W=11, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((1, C, F, H, W), generator=g) * 1.2 - 0.1           # some samples outside [0, 1]
    x[0, 0, 0, 0, :4] = torch.tensor([0.0, 1.0, 3e-6, 6.0e-8])         # float16 subnormals among them
    return x.to(dtype)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("display", ["standard_4k", "standard_hdr_pq"])
def test_array_source_frames_equal_the_float32_source_on_the_upcast_array(dtype, display):
    t16, r16 = clip(dtype, seed=3), clip(dtype, seed=4)
    v16 = fvvdp_video_source_array(t16, r16, 30, display_photometry=display)
    v32 = fvvdp_video_source_array(t16.float(), r16.float(), 30, display_photometry=display)
    assert v16.test_video.dtype is dtype and v16.get_video_size() == v32.get_video_size()
    for f in range(4):
        assert torch.equal(v16.get_test_frame(f), v32.get_test_frame(f))
        assert torch.equal(v16.get_reference_frame(f), v32.get_reference_frame(f))
        assert v16.get_test_frame(f).dtype is torch.float32


def test_numpy_float16_is_carried_as_float16():
    a = clip(torch.float16)[0].numpy()                                  # [C, F, H, W] float16
    assert a.dtype == np.float16
    v16 = fvvdp_video_source_array(a, a[:, ::-1].copy(), 30, dim_order="CFHW")
    v32 = fvvdp_video_source_array(a.astype(np.float32), a[:, ::-1].astype(np.float32), 30, dim_order="CFHW")
    assert v16.test_video.dtype is torch.float16
    assert torch.equal(v16.get_test_frame(1), v32.get_test_frame(1))
    t, r = _image_stack(a[:, 0][None], a[:, 1][None], "BCHW")
    assert t.dtype is torch.float16 and tuple(t.shape) == (1, 3, 9, 11)


@pytest.mark.parametrize("dtype", HALF)
def test_image_stack_and_pair_keep_half_tensors(dtype):
    x = clip(dtype)[0, :, 0]                                            # [C, H, W]
    t, r = _image_stack(torch.stack([x, x]), torch.stack([x, x]), "BCHW")
    assert t.dtype is dtype and r.dtype is dtype and tuple(t.shape) == (2, 3, 9, 11)
    t, r = _image_pair(x.permute(1, 2, 0), x.permute(1, 2, 0), "HWC")
    assert t.dtype is dtype and tuple(t.shape) == (3, 9, 11) and torch.equal(t, x)
    assert _sample_type(dtype) == ((nat.FVVDP_F16 if dtype is torch.float16 else nat.FVVDP_BF16), 0)
    assert _sample_type(torch.float32) == (nat.FVVDP_F32, 0) and (nat.FVVDP_F16, nat.FVVDP_BF16) == (3, 4)


def test_float64_is_refused_as_before():
    x = torch.rand((1, 3, 2, 8, 8), dtype=torch.float64)
    vs = fvvdp_video_source_array(x, x, 30)
    with pytest.raises(RuntimeError, match="Only uint8, uint16 and float32 is currently supported"):
        vs.get_test_frame(0)
    with pytest.raises(RuntimeError, match="Only uint8, uint16 and float32 is currently supported"):
        _sample_type(torch.float64)
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    with pytest.raises(RuntimeError, match="Only uint8, uint16 and float32 is currently supported"):
        m._image_eotf(torch.float64)
    with pytest.raises(RuntimeError, match="float32, float16 or bfloat16 test and reference images .got torch.float64"):
        m.jod_images(x[:, :, 0], x[:, :, 0])


@pytest.mark.parametrize("dtype", HALF)
def test_refusals_name_the_dtype(dtype):
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    x = torch.rand((2, 3, 16, 24)).to(dtype)
    psi = m.display_parameter_tensor()
    with pytest.raises(RuntimeError, match=r"display_jod_images needs float32 test and reference \(got %s and %s\)" % (dtype, dtype)):
        m.display_jod_images(x, x, psi)
    v = torch.rand((1, 3, 4, 16, 24)).to(dtype)
    with pytest.raises(RuntimeError, match=r"display_jod_video needs float32 test and reference \(got %s and torch.float32\)" % dtype):
        m.display_jod_video(v, v.float(), psi, frames_per_second=30)
    p = fv.pu_psnr(device="cuda:0")                                     # (the constructor touches no device)
    with pytest.raises(RuntimeError, match="pu_psnr takes uint8, uint16 and float32 sources, not %s" % dtype):
        p.predict(v, v, frames_per_second=30)
    with pytest.raises(RuntimeError, match="pu_psnr takes uint8, uint16 and float32 sources, not %s" % dtype):
        p.predict(v.float(), v, frames_per_second=30)


def test_mixed_pairs_are_upcast_inside_autograd():
    from fovvideovdp_amd.image_grad import float_pair
    t = torch.rand((1, 1, 8, 8)).half().requires_grad_(True)
    r = torch.rand((1, 1, 8, 8))
    a, b = float_pair("jod_images", "images", t, r)
    assert a.dtype is torch.float32 and b is r and a.grad_fn is not None          # torch's own cast node
    a.sum().backward()
    assert t.grad.dtype is torch.float16
    a, b = float_pair("jod_images", "images", t, r.half())
    assert a is t and b.dtype is torch.float16                                      # equal dtypes pass as they are
    with pytest.raises(RuntimeError, match=r"jod_video needs float32, float16 or bfloat16 .* clips \(got torch.uint8 and torch.float16\)"):
        float_pair("jod_video", "clips", torch.zeros(2, dtype=torch.uint8), t)


def test_half_header_is_exported_and_bound():
    nat.build()
    names = declared("fvvdp_hip_half.h")
    assert names == ["fvvdp_images_grad_st", "fvvdp_images_ref_grad_st", "fvvdp_video_grad_input_st"]
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert sorted(nat.HALF_SYMBOLS) == names
    lib = nat.lib()
    untyped = {"fvvdp_images_grad_st": nat.GRAD_SYMBOLS["fvvdp_images_grad"], "fvvdp_images_ref_grad_st":
               nat.REF_GRAD_SYMBOLS["fvvdp_images_ref_grad"], "fvvdp_video_grad_input_st": nat.VIDEO_GRAD_SYMBOLS["fvvdp_video_grad_input"]}
    for name in names:
        args = list(getattr(lib, name).argtypes)
        assert len(args) == len(untyped[name][1]) + 1 and args.count(ctypes.c_int) == untyped[name][1].count(ctypes.c_int) + 1, name
    txt = open(os.path.join(ROOT, "include", "fvvdp_hip.h")).read()
    assert re.search(r"FVVDP_F32 = 2, FVVDP_F16 = 3, FVVDP_BF16 = 4", txt)
    # the untyped headers keep their function lists
    assert declared("fvvdp_hip_grad.h") == ["fvvdp_images_grad", "fvvdp_images_grad_workspace"]
    assert len(declared("fvvdp_hip_video_grad.h")) == 3 and len(declared("fvvdp_hip_ref_grad.h")) == 4


def test_st_entry_points_check_the_sample_type_without_a_device():
    nat.build()
    lib = nat.lib()
    prm, pp, e = nat.Params(), nat.PoolParams(), nat.Eotf()
    pp.beta_sch = pp.beta_tch = pp.beta_t = pp.beta_jod = prm.beta = 1.0
    e.kind = nat.EOTF_SRGB
    p = ctypes.c_void_p(256)
    maps = (nat.BandMaps * 4)(*[nat.BandMaps(256, 256, 256, 256) for _ in range(4)])
    one = (ctypes.c_void_p * 1)(258)                                   # 2-byte aligned, not 4
    w = np.ones(3, dtype=np.float32)
    ff = np.zeros(8, dtype=np.int32)
    fp = np.arange(8, dtype=np.int32)
    taps = np.ones((2, 8), dtype=np.float32)
    i32 = ctypes.POINTER(ctypes.c_int32)

    def img(dtype):
        return lib.fvvdp_images_grad_st(64, 48, 4, 1, ctypes.byref(prm), ctypes.byref(pp), p, 1, 0, p, maps, one, dtype, 1, 64 * 48,
                                        ctypes.byref(e), nat.fptr(w), one, p, 1 << 30, None)

    def vid(dtype, ptr=258):
        return lib.fvvdp_video_grad_input_st(64, 48, 9, p, ff.ctypes.data_as(i32), fp.ctypes.data_as(i32), nat.fptr(taps), 8,
                                             ctypes.c_void_p(ptr), ctypes.c_void_p(ptr), dtype, 1, 0, 64 * 48, ctypes.byref(e),
                                             nat.fptr(w), p, 1 << 30, None)

    for bad in (nat.FVVDP_U8, nat.FVVDP_U16, 5, -1):
        assert img(bad) == -1 and b"float32, float16 and bfloat16" in lib.fvvdp_last_error(), bad
        assert vid(bad) == -1 and b"float32, float16 and bfloat16" in lib.fvvdp_last_error(), bad
    # float32 samples must be 4-byte aligned, 16-bit samples 2-byte
    assert img(nat.FVVDP_F32) == -1 and b"aligned to 4 bytes" in lib.fvvdp_last_error()
    assert vid(nat.FVVDP_F32) == -1 and b"aligned to 4 bytes" in lib.fvvdp_last_error()
    assert vid(nat.FVVDP_F16, 257) == -1 and b"2 bytes" in lib.fvvdp_last_error()


def test_half_kernels_do_not_spill_and_the_old_names_keep_their_counts():
    """The new entry points have names of their own (temporal_vec_half_kernel, temporal_ring_half_kernel, ...), so the counts the
    other tests make by name stay; the register-ring ones meet the bar of their float siblings: nothing spilled, no scratch."""
    import codeobj
    nat.build()
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    names = list(md)
    nice = codeobj.demangle(names)
    count = {}
    for m, n in zip(names, nice):
        base = n.split("(")[0]
        fam = base.split("<")[0].split()[-1]
        count[fam] = count.get(fam, 0) + 1
        if "_half_kernel" in fam:
            x = md[m]
            assert (x["sgpr_spill_count"], x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), n
            assert re.search(r"[<,] ?[34](, 1)?>$", base) or fam == "video_input_half_kernel", n      # SRC_F16 = 3, SRC_BF16 = 4
    # per sample type: 8 / 16 / 32 / 64-slot vector rings, 8 / 16 / 32-slot per-pixel rings, 4- and 1-pixel still ingest, one image
    # backward kernel, 8 transposes (4 ring sizes x {vector, per-pixel})
    assert count["temporal_vec_half_kernel"] == 8 and count["temporal_ring_half_kernel"] == 6
    assert count["still_ingest_half_kernel"] == 4 and count["grad_input_half_kernel"] == 2
    assert count["video_input_half_kernel"] == 16
    assert count["luminance_frames_kernel"] == 5 and count["temporal_generic_kernel"] == 10
    # the old names, as test_host_cpu / test_image_batch_cpu / test_video_grad_cpu count them
    assert count["temporal_vec_kernel"] == 12 and count["temporal_ring_kernel"] == 9
    assert count["still_ingest_kernel"] == 5 and count["grad_input_kernel"] == 1 and count["video_input_kernel"] == 8
