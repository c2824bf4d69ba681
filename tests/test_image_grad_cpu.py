"""Still-image gradients without a GPU: the third C header and its binding, the code objects of the new kernels, and the
refusals of fvvdp.jod_images that come before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KERNELS = ("grad_coef_kernel", "adj_layer_kernel", "adj_sweep_kernel", "grad_input_kernel")


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def test_grad_header_is_exported_and_bound():
    nat.build()
    names = declared("fvvdp_hip_grad.h")
    assert names == ["fvvdp_images_grad", "fvvdp_images_grad_workspace"]
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert sorted(nat.GRAD_SYMBOLS) == names
    assert not set(names) & (set(nat.SYMBOLS) | set(nat.IMAGE_SYMBOLS))
    assert len(declared("fvvdp_hip.h")) == 24 and len(declared("fvvdp_hip_images.h")) == 3
    lib = nat.lib()
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    assert not hasattr(L, "fvvdp_fail_from")          # the library's internal error hook stays out of the C ABI


def test_grad_argument_checks_need_no_device():
    lib = nat.lib()
    nbytes = ctypes.c_size_t(0)
    assert lib.fvvdp_images_grad_workspace(64, 48, 4, 2, None) == -1
    assert lib.fvvdp_images_grad_workspace(64, 48, 0, 2, ctypes.byref(nbytes)) == -1
    assert lib.fvvdp_images_grad_workspace(64, 48, 4, 0, ctypes.byref(nbytes)) == -1
    assert lib.fvvdp_images_grad_workspace(64, 48, 4, 2, ctypes.byref(nbytes)) == 0
    # coefficients + layer gradients of levels 0..3 + sweep gradients of levels 1..4, each part 256-byte aligned
    sizes = [(64, 48), (32, 24), (16, 12), (8, 6), (4, 3)]
    al = lambda x: (x + 63) // 64 * 64
    expect = al(2 * 4) + sum(al(2 * w * h) for w, h in sizes[:4]) + sum(al(2 * w * h) for w, h in sizes[1:])
    assert nbytes.value == 4 * expect
    assert lib.fvvdp_images_grad(64, 48, 4, 1, None, None, None, 1, 0, None, None, None, 3, 0, None, None, None, None, 0,
                                 None) == -1
    assert b"null" in lib.fvvdp_last_error()
    # a complete argument list with a bad shape / display model / workspace is refused before any launch
    prm, pp = nat.Params(), nat.PoolParams(1, 1, 1, 1, -0.016, 0.6)
    prm.beta = 1.5
    maps = (nat.BandMaps * 4)()
    for b in range(4):
        maps[b].d_D = maps[b].d_contrast = maps[b].d_lbkg = maps[b].d_S = 256
    ptr = (ctypes.c_void_p * 1)(256)
    e = nat.Eotf()
    e.kind = nat.EOTF_SRGB
    w = np.array([0.2126, 0.7152, 0.0722], np.float32)

    def call(C=3, n_bands=4, kind=nat.EOTF_SRGB, work=1 << 30, q_col0=0):
        e.kind = kind
        return lib.fvvdp_images_grad(64, 48, n_bands, 1, ctypes.byref(prm), ctypes.byref(pp), ctypes.c_void_p(256), 1, q_col0,
                                     ctypes.c_void_p(256), maps, ptr, C, 64 * 48, ctypes.byref(e), nat.fptr(w), ptr,
                                     ctypes.c_void_p(256), work, None)

    assert call(C=2) == -1 and b"colour channels" in lib.fvvdp_last_error()
    assert call(n_bands=17) == -1
    assert call(kind=nat.EOTF_LUT) == -1 and b"closed-form" in lib.fvvdp_last_error()
    assert call(kind=nat.EOTF_NONE) == -1
    assert call(work=16) == -1 and b"workspace" in lib.fvvdp_last_error()
    assert call(q_col0=1) == -1 and b"Q columns" in lib.fvvdp_last_error()


def test_new_kernels_do_not_spill():
    import codeobj
    nat.build()
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    names = list(md)
    nice = codeobj.demangle(names)
    found = {k: 0 for k in NEW_KERNELS}
    hot = ("band_kernel<", "band2_kernel<", "band2_fov_kernel<", "temporal_vec_kernel<", "temporal_ring_kernel<",
           "temporal_yuv_kernel<", "temporal_yuv_vec_kernel<", "still_ingest_kernel<", "pool_jod_cols_kernel", "pu21_sse_kernel<")
    for m, n in zip(names, nice):
        base = n.split("(")[0]
        if base in found:
            found[base] += 1
            x = md[m]
            assert (x["sgpr_spill_count"], x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), n
            assert not any(h in n for h in hot), n
    assert found == {k: 1 for k in NEW_KERNELS}


def test_jod_images_refusals_without_device():
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    x = torch.rand((1, 3, 32, 48))
    r = torch.rand((1, 3, 32, 48))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.jod_images(x.clone().requires_grad_(True), r)
    with pytest.raises(RuntimeError, match="gradients with respect to the reference are not supported"):
        m.jod_images(x.clone().requires_grad_(True), r.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="F axis"):
        m.jod_images(torch.rand((1, 3, 2, 32, 48)), torch.rand((1, 3, 2, 32, 48)), dim_order="BCFHW")
    with pytest.raises(RuntimeError, match="float32"):
        m.jod_images(x.double(), r.double())
    with pytest.raises(RuntimeError, match="float32"):
        m.jod_images((x * 255).to(torch.uint8), (r * 255).to(torch.uint8))


def test_jod_images_refuses_user_photometry():
    class MyDisplay(fv.fvvdp_display_photometry):
        def forward(self, V):
            return 100.0 * V + 0.5

        def get_peak_luminance(self):
            return 100.5

        def get_black_level(self):
            return 0.5

    m = fv.fvvdp(display_name="standard_4k", display_photometry=MyDisplay(), device="cpu", quiet=True)
    with pytest.raises(RuntimeError, match="closed form"):
        m.jod_images(torch.rand((1, 3, 32, 48)), torch.rand((1, 3, 32, 48)))


def test_predict_refusal_keeps_its_wording():
    from fovvideovdp_amd.fvvdp import _refuse_grad
    x = torch.zeros((1, 3, 32, 48), requires_grad=True)
    with pytest.raises(RuntimeError, match=r"^Gradients through the metric are not supported on the HIP path.*jod_images"):
        _refuse_grad(x)
