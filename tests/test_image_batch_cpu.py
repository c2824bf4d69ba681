"""Batched still images without a GPU: the second C header and its binding, the code objects of the new kernels, and the
host-side parsing / refusal rules of fvvdp.predict_images / predict_image_pairs."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd.fvvdp import _image_pair, _image_stack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def test_images_header_is_exported_and_bound():
    nat.build()
    names = declared("fvvdp_hip_images.h")
    assert names == ["fvvdp_images_channels", "fvvdp_images_forward_pool", "fvvdp_pool_jod_columns"]
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert sorted(nat.IMAGE_SYMBOLS) == names
    assert len(declared("fvvdp_hip.h")) == 24 and not set(names) & set(nat.SYMBOLS)
    lib = nat.lib()
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    # argument checks run before anything touches a device
    assert lib.fvvdp_images_channels(None, None, None, 1, 0, 3, 0, None, None, 0, None, None) == -1
    pp = nat.PoolParams(1, 1, 1, 1, 1, 1)
    assert lib.fvvdp_pool_jod_columns(None, 4, 2, 1, 1, ctypes.byref(pp), None, None) == -1
    assert lib.fvvdp_images_forward_pool(None, 1, None, 1, 0, None, None, None, None, None, None) == -1


def test_new_kernels_do_not_spill_and_existing_counts_stay():
    import codeobj
    nat.build()
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    names = list(md)
    nice = codeobj.demangle(names)
    hot = ("temporal_vec_kernel<", "band2_kernel<", "band2_fov_kernel<", "band_kernel<", "temporal_ring_kernel<",
           "temporal_yuv_kernel<", "temporal_yuv_vec_kernel<", "pu21_sse_kernel<")
    still = [(m, n) for m, n in zip(names, nice) if "still_ingest_kernel<" in n or "pool_jod_cols_kernel" in n]
    assert len(still) == 6                      # uint8 / float x {1, 4} pixels per lane, uint16 x 1, the column pooling
    for m, n in still:
        x = md[m]
        assert (x["sgpr_spill_count"], x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), n
        assert not any(h in n for h in hot), n
    counts = {h: sum(1 for n in nice if h in n) for h in hot}
    # the instantiation counts test_hot_kernels_do_not_spill relies on (the batched path reuses band_kernel / band2_kernel)
    assert sum(1 for n in nice if "band2_kernel<" in n or "band2_fov_kernel<" in n) == 4
    assert counts["temporal_vec_kernel<"] == 12 and counts["temporal_ring_kernel<"] == 9


def test_stack_parsing():
    a = np.zeros((5, 32, 48, 3), np.uint8)
    t, r = _image_stack(a, a, "BHWC")
    assert tuple(t.shape) == (5, 3, 32, 48) and t.dtype is torch.uint8
    t, r = _image_stack(np.zeros((2, 1, 1, 16, 16), np.uint16), np.zeros((2, 1, 1, 16, 16), np.uint16), "BCFHW")
    assert tuple(t.shape) == (2, 1, 16, 16) and t.dtype is torch.int16
    t, r = _image_stack(np.zeros((4, 16, 16), np.float32), np.zeros((4, 16, 16), np.float32), "BHW")
    assert tuple(t.shape) == (4, 1, 16, 16)
    with pytest.raises(RuntimeError, match="B axis"):
        _image_stack(a[0], a[0], "HWC")
    with pytest.raises(RuntimeError, match="F axis"):
        _image_stack(np.zeros((1, 3, 2, 8, 8)), np.zeros((1, 3, 2, 8, 8)), "BCFHW")
    with pytest.raises(RuntimeError, match="same shape"):
        _image_stack(a, a[:, :16], "BHWC")
    with pytest.raises(RuntimeError, match="colour channels"):
        _image_stack(a[..., :2], a[..., :2], "BHWC")
    with pytest.raises(RuntimeError):
        _image_stack(a, a, "BHW")
    t, r = _image_pair(np.zeros((8, 12, 3), np.uint8), np.zeros((8, 12, 3), np.uint8), "HWC")
    assert tuple(t.shape) == (3, 8, 12)
    with pytest.raises(RuntimeError, match="one image pair"):
        _image_pair(a, a, "BHWC")


def test_refusals_without_gpu():
    m = fv.fvvdp(display_name="standard_fhd", device=torch.device("cpu"))
    a = np.zeros((2, 64, 64), np.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict_images(a, a, dim_order="BHW")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict_image_pairs([(a[0], a[0])], dim_order="HW")
    g = fv.fvvdp(display_name="standard_fhd", device=torch.device("cuda:0"))
    x = torch.zeros((2, 64, 64), requires_grad=True)
    with pytest.raises(RuntimeError, match="Gradients"):
        g.predict_images(x, x.detach(), dim_order="BHW")
    with pytest.raises(RuntimeError, match="Gradients"):
        g.predict_image_pairs([(x[0], x[0].detach())], dim_order="HW")


def test_grouping_keeps_input_order(monkeypatch):
    """predict_image_pairs groups by (shape, dtypes), runs each group once and hands the results back in input order."""
    m = fv.fvvdp(display_name="standard_fhd", device=torch.device("cuda:0"))
    calls = []

    def fake_group(ts, rs, fix, sync, labels=None):
        calls.append([tuple(t.shape) + (str(t.dtype), str(r.dtype)) for t, r in zip(ts, rs)])
        tags = [float(t.reshape(-1)[0]) for t in ts]
        return torch.tensor(tags), {"Q_per_ch": np.array(tags)[:, None, None, None], "range_flags": np.zeros(len(ts), bool),
                                    "rho_band": None, "width": ts[0].shape[2], "height": ts[0].shape[1], "frames_per_second": 0}

    monkeypatch.setattr(m, "_predict_image_group", fake_group)
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    pairs = []
    for i, (shape, dt) in enumerate([((8, 8), np.uint8), ((9, 8), np.uint8), ((8, 8), np.float32), ((8, 8), np.uint8),
                                     ((9, 8), np.uint8), ((8, 8), np.uint16)]):
        t = np.full(shape, i, dtype=dt)
        pairs.append((t, t.copy()))
    res = m.predict_image_pairs(pairs, dim_order="HW")
    assert [float(q) for q, _ in res] == [0, 1, 2, 3, 4, 5]
    assert [s["Q_per_ch"].reshape(-1)[0] for _, s in res] == [0, 1, 2, 3, 4, 5]
    assert len(calls) == 4 and len(calls[0]) == 2 and calls[0][0][:3] == (1, 8, 8)
    assert all(s["N_frames"] == 1 and s["Q_per_ch"].shape == (1, 1, 1) for _, s in res)
