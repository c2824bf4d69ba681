"""Held-frame clips without a GPU: the header and its binding, the argument checks of its two entry points, every refusal of
fvvdp.predict_held / fvvdp.jod_video_held that comes before any device work, the normalisation of the frame maps with the composed
lists and the source-keyed fold list, the float64 restatement (tests/held_ref.py) against the dense transpose and the inner-product
identity, the case table's cap on head-shown frames, the code objects of the new kernels, and the golden."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd import held
from fovvideovdp_amd.fvvdp import window_frame_indices
from fovvideovdp_amd.grad_passes import _fold_arrays, fold_list, held_fold_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import held_cases as hc                      # noqa: E402
import held_ref as href                      # noqa: E402

NEW_KERNELS = ["void held_vec_kernel<%d, %d, %d>" % (fl, 4 if fl == 8 else 2, st) for fl in (8, 16, 32) for st in range(5)] + \
    ["void held_ring_kernel<%d, %d, %d>" % (fl, 2 if fl == 32 else 4, st) for fl in (8, 16, 32) for st in range(5)] + \
    ["void video_input_held_kernel<%d, %d, %d>" % (fl, px, st) for fl in (8, 16, 32) for px in ((4 if fl <= 16 else 2), 1)
     for st in (2, 3, 4)]


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def test_held_header_is_exported_and_bound():
    nat.build()
    names = declared("fvvdp_hip_held.h")
    assert names == ["fvvdp_temporal_channels_held", "fvvdp_video_grad_input_held"]
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert sorted(nat.HELD_SYMBOLS) == names
    lib = nat.lib()
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    assert not hasattr(L, "fvvdp_ctx_ingest_begin")                               # the context's side of the ingest stays internal
    assert not any("held" in n for n in declared("fvvdp_hip.h"))                # nothing is added to fvvdp_hip.h
    txt = open(os.path.join(ROOT, "include", "fvvdp_hip_held.h")).read()
    assert int(re.search(r"#define FVVDP_HELD_MAX_TAPS (\d+)", txt).group(1)) == nat.HELD_MAX_TAPS == 32
    assert ctypes.sizeof(nat.HeldStream) == 32
    assert nat.held_map_bytes(1) == 256 and nat.held_map_bytes(64) == 256 and nat.held_map_bytes(65) == 512
    assert callable(fv.fvvdp.predict_held) and callable(fv.fvvdp.jod_video_held)


def test_argument_checks_need_no_device():
    lib = nat.lib()
    p = ctypes.c_void_p
    i32p = ctypes.POINTER(ctypes.c_int32)
    e = nat.Eotf()
    w = np.ones(3, np.float32)
    W, H, N, F = 16, 8, 12, 6
    HW = W * H
    taps = np.ones((2, 40), np.float32)

    # the backward
    def bwd(g0=256, m=None, ff=None, fp=None, fl=8, src=512, grad=1024, dtype=nat.FVVDP_F32, C=3, cs=F * HW, fs=HW, kind=nat.EOTF_SRGB,
            head=4096, hb=1 << 30, width=W, n_display=N, n_source=F):
        e.kind = kind
        m = np.asarray((np.arange(n_display) // 2) if m is None else m, np.int32)
        if ff is None:
            ff, fp = held_fold_arrays(m, window_frame_indices(n_display, fl, "replicate"), fl) if 1 <= fl <= 32 else (np.zeros(64, np.int32),) * 2
        ff, fp = np.ascontiguousarray(ff, np.int32), np.ascontiguousarray(fp, np.int32)
        return lib.fvvdp_video_grad_input_held(width, H, n_display, n_source, p(g0), m.ctypes.data_as(i32p), ff.ctypes.data_as(i32p),
                                               fp.ctypes.data_as(i32p), nat.fptr(taps), fl, p(src), p(grad), dtype, C, cs, fs,
                                               ctypes.byref(e), nat.fptr(w), p(head), hb, None)

    err = lib.fvvdp_last_error
    assert lib.fvvdp_video_grad_input_held(W, H, N, F, None, None, None, None, None, 8, None, None, 2, 3, 0, 0, None, None, None, 0,
                                           None) == -1 and b"null" in err()
    assert bwd(width=0) == -1 and b"bad shape" in err()
    assert bwd(n_source=0) == -1 and b"bad shape" in err()
    for bad in (nat.FVVDP_U8, nat.FVVDP_U16, 5):
        assert bwd(dtype=bad) == -1 and b"float32, float16 and bfloat16" in err()
    assert bwd(fl=0) == -1 and b"filter length" in err()
    assert bwd(fl=33) == nat.FVVDP_EUNSUPPORTED and b"up to 32 taps" in err()
    assert bwd(C=2) == -1 and b"1 or 3 colour channels" in err()
    assert bwd(fs=HW - 1) == -1 and b"frame_stride" in err()
    assert bwd(cs=HW - 1) == -1 and b"chan_stride" in err()
    assert bwd(kind=nat.EOTF_LUT) == -1 and b"closed-form" in err()
    assert bwd(m=np.arange(N)) == -1 and b"frame map entry 6 names source frame 6 outside [0, 6)" in err()
    assert bwd(m=[-1] + [0] * (N - 1)) == -1 and b"outside [0, 6)" in err()
    assert bwd(m=[0, 1, 0] + [2] * (N - 3)) == -1 and b"non-decreasing (entry 2: 0 after 1)" in err()
    ff, fp = held_fold_arrays(np.arange(N) // 2, window_frame_indices(N, 8, "circular"), 8)
    assert bwd(ff=ff[::-1], fp=fp) == -1 and b"sorted by frame" in err()
    assert bwd(ff=np.full(8, 6), fp=np.arange(8)) == -1 and b"fold list entry 0 names source frame 6" in err()
    assert bwd(ff=np.zeros(8), fp=np.zeros(8)) == -1 and b"listed twice" in err()
    assert bwd(head=4097) == -1 and b"256-byte aligned" in err()
    assert bwd(hb=256 + 8 * HW * 4 - 1) == -1 and b"side buffer of" in err()
    assert bwd(src=514) == -1 and b"aligned to 4 bytes" in err()
    assert bwd(dtype=nat.FVVDP_F16, grad=1025) == -1 and b"2 bytes" in err()

    # the ingest: everything that is checked before the context is looked at (a context needs a device)
    idx = np.zeros(64, np.int32)

    def ing(ctx=256, t=None, r=None, dtype=nat.FVVDP_F32, C=3, kind=nat.EOTF_SRGB, fl=8, it=idx, ir=idx, n_out=4, lut=None):
        e.kind, e.d_lut = kind, lut
        t = t or nat.HeldStream(512, F * HW, HW, F)
        r = r or nat.HeldStream(1024, N * HW, HW, N)
        return lib.fvvdp_temporal_channels_held(p(ctx), ctypes.byref(t), ctypes.byref(r), dtype, C, ctypes.byref(e), nat.fptr(w),
                                                it.ctypes.data_as(i32p), ir.ctypes.data_as(i32p), nat.fptr(taps), fl, n_out, 0, None, None)

    assert ing(ctx=None) == -1 and b"null" in err()
    assert ing(dtype=5) == -1 and b"Only uint8, uint16 and float32" in err()
    assert ing(C=2) == -1 and b"1 or 3 colour channels" in err()
    assert ing(fl=0) == -1 and b"filter length" in err()
    assert ing(fl=33) == nat.FVVDP_EUNSUPPORTED and b"up to 32 taps" in err()
    assert ing(kind=nat.EOTF_LUT) == -1 and b"needs an integer source and a table" in err()
    assert ing(dtype=nat.FVVDP_U8) == -1 and b"uint8 sources need FVVDP_EOTF_LUT" in err()
    assert ing(n_out=0) == -1 and b"at least one output frame" in err()
    bad = idx.copy()
    bad[5] = F
    assert ing(it=bad) == -1 and b"list entry 5 names frame 6 outside the test's [0, 6)" in err()
    bad[5] = N
    assert ing(ir=bad) == -1 and b"list entry 5 names frame 12 outside the reference's [0, 12)" in err()
    assert ing(it=-np.ones(64, np.int32)) == -1 and b"outside the test's" in err()


def test_refusals_without_device():
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    t, r = torch.rand(1, 3, 4, 17, 30), torch.rand(1, 3, 8, 17, 30)
    for call, name in ((m.predict_held, "predict_held"), (m.jod_video_held, "jod_video_held")):
        kw = dict(frames_per_second=30, test_frames=2)
        for bad in (2.0, np.float32(2), True):
            with pytest.raises(ValueError, match="test_frames must be an int k >= 1 or a 1-D integer sequence"):
                call(t, r, frames_per_second=30, test_frames=bad)
        with pytest.raises(ValueError, match="must hold integers"):
            call(t, r, frames_per_second=30, test_frames=[0.0, 0.0, 1.0, 1.0, 2.0, 2.0, 3.0, 3.0])
        with pytest.raises(ValueError, match="must hold integers"):
            call(t, r, frames_per_second=30, reference_frames=torch.arange(8).float())
        with pytest.raises(ValueError, match=r"test_frames must be non-decreasing \(entry 2: 0 after 1\)"):
            call(t, r, frames_per_second=30, test_frames=[0, 1, 0, 1, 2, 2, 3, 3])
        with pytest.raises(ValueError, match=r"test_frames names frame 4 outside the test's \[0, 4\)"):
            call(t, r, frames_per_second=30, test_frames=[0, 0, 1, 1, 2, 2, 3, 4])
        with pytest.raises(ValueError, match=r"reference_frames names frame -1 outside"):
            call(t, r, frames_per_second=30, test_frames=2, reference_frames=[-1, 0, 1, 2, 3, 4, 5, 6])
        with pytest.raises(ValueError, match="1-D sequence"):
            call(t, r, frames_per_second=30, test_frames=[[0, 0, 1, 1], [2, 2, 3, 3]])
        with pytest.raises(ValueError, match="test_frames=0: a frame is held for k >= 1"):
            call(t, r, frames_per_second=30, test_frames=0)
        with pytest.raises(ValueError, match="reference_frames=-2"):
            call(t, r, frames_per_second=30, test_frames=2, reference_frames=-2)
        with pytest.raises(ValueError, match="the test is shown for 12 display frames and the reference for 8"):
            call(t, r, frames_per_second=30, test_frames=3)
        with pytest.raises(ValueError, match="the test is shown for 7 display frames and the reference for 8"):      # a wrong-length map
            call(t, r, frames_per_second=30, test_frames=[0, 0, 1, 1, 2, 2, 3])
        with pytest.raises(ValueError, match="at least 2 display frames, got 1"):
            call(t[:, :, :1], r[:, :, :1], frames_per_second=30)
        with pytest.raises(RuntimeError, match="display rate too high: its temporal filter has 33 taps"):
            call(t, r, frames_per_second=130, test_frames=2)
        with pytest.raises(RuntimeError, match="frames_per_second"):
            call(t, r, test_frames=2)
        with pytest.raises(RuntimeError, match=r"differ in their channel counts \(3 and 1\)"):
            call(t, r[:, :1], **kw)
        with pytest.raises(RuntimeError, match="differ in their frame sizes"):
            call(t, r[..., :29], **kw)
        with pytest.raises(RuntimeError, match="either 1 or 3 colour channels"):
            call(t[:, :2], r[:, :2], **kw)
        with pytest.raises(RuntimeError, match="one clip per call"):
            call(torch.rand(2, 3, 4, 17, 30), torch.rand(2, 3, 8, 17, 30), **kw)
        with pytest.raises(RuntimeError, match="exactly as many dimensions"):
            call(t, r, dim_order="CFHW", **kw)
        with pytest.raises(RuntimeError, match="an F axis"):
            call(t[0, :, 0], r[0, :, 0], dim_order="CHW", **kw)
        vs = fv.fvvdp_video_source_array(r, r, 30, display_photometry="standard_4k") if hasattr(fv, "fvvdp_video_source_array") else None
        if vs is not None:
            with pytest.raises(RuntimeError, match="video source object"):
                call(vs, r, **kw)
        with pytest.raises(RuntimeError, match="samples; the test is float64"):
            call(t.double(), r, **kw)
        # everything accepted: the first device work is refused on a CPU metric
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(t, r, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(t, r, frames_per_second=120, test_frames=np.arange(8) // 2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):                    # both maps the identity: predict / jod_video
            call(r, r.clone(), frames_per_second=30)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(r, r.clone(), frames_per_second=30, test_frames=list(range(8)), reference_frames=torch.arange(8))
    hm = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True, heatmap="raw")
    for call in (hm.predict_held, hm.jod_video_held):
        with pytest.raises(RuntimeError, match="makes no heat maps"):
            call(t, r, frames_per_second=30, test_frames=2)
    # what jod_video refuses
    with pytest.raises(RuntimeError, match="samples; the test is uint8"):
        m.jod_video_held((t * 255).to(torch.uint8), r, frames_per_second=30, test_frames=2)
    with pytest.raises(RuntimeError, match="gradients with respect to the reference are not supported"):
        m.jod_video_held(t, r.clone().requires_grad_(True), frames_per_second=30, test_frames=2)
    with pytest.raises(RuntimeError, match='wrt="reference" treats the test as a constant'):
        m.jod_video_held(t.clone().requires_grad_(True), r, frames_per_second=30, test_frames=2, wrt="reference")
    with pytest.raises(ValueError, match="wrt must be"):
        m.jod_video_held(t, r, frames_per_second=30, test_frames=2, wrt="tests")
    with pytest.raises(RuntimeError, match="forward-only"):
        m.predict_held(t.clone().requires_grad_(True), r, frames_per_second=30, test_frames=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                         # predict_held takes integer samples
        m.predict_held((t * 255).to(torch.uint8), (r.numpy() * 65535).astype(np.uint16), frames_per_second=30, test_frames=2)


def test_refuses_user_photometry():
    class MyDisplay(fv.fvvdp_display_photometry):
        def forward(self, V):
            return 100.0 * V + 0.5

        def get_peak_luminance(self):
            return 100.5

        def get_black_level(self):
            return 0.5

    m = fv.fvvdp(display_name="standard_4k", display_photometry=MyDisplay(), device="cpu", quiet=True)
    for call in (m.predict_held, m.jod_video_held):
        with pytest.raises(RuntimeError, match="needs a display model with a closed form"):
            call(torch.rand(3, 4, 17, 30), torch.rand(3, 8, 17, 30), dim_order="CFHW", frames_per_second=30, test_frames=2)


# ---- frame maps ---------------------------------------------------------------------------------------------------------------------
def test_map_normalisation():
    for F, k in ((4, 1), (4, 2), (5, 3), (1, 7)):
        m = held.frame_map("test", k, F)
        assert m.dtype == np.int32 and np.array_equal(m, np.repeat(np.arange(F), k))
        for seq in (list(m), tuple(m), np.asarray(m, np.int64), np.asarray(m, np.uint8), torch.as_tensor(m), torch.as_tensor(m).long()):
            m2 = held.frame_map("test", seq, F)
            assert m2.dtype == np.int32 and np.array_equal(m2, m)
        assert np.array_equal(held.frame_map("test", np.int64(k), F), m)
    assert held._is_identity(held.frame_map("test", 1, 6), 6) and not held._is_identity(held.frame_map("test", 2, 3), 6)
    assert not held._is_identity(np.arange(5), 6)                                  # the identity on a prefix skips the last frame
    m_t, m_r = held.frame_maps(4, hc.skipping(8), 2, 11)
    assert len(m_t) == len(m_r) == 8
    m_t, m_r = held.frame_maps(2, 1, 1, 2)                                         # N = 2: the shortest clip
    assert list(m_t) == [0, 0] and list(m_r) == [0, 1]
    assert list(hc.pulldown(10)) == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3] and list(hc.skipping(6)) == [0, 1, 3, 4, 6, 7]


@pytest.mark.parametrize("padding", hc.PADDINGS)
def test_composed_lists_and_fold_list(padding):
    for fl in (1, 8, 15, 30):
        for N in (2, fl + 1, 2 * fl + 3):
            widx = window_frame_indices(N, fl, padding)
            for kind in hc.MAP_KINDS + ("identity",):
                m, F = hc.c_abi_map(kind, N)
                comp = href.composed(m, widx)
                # the list IS the expanded clip's list read through the map: index_select then window == window then map
                assert len(comp) == N + fl - 1 and all(comp[p] == m[widx[p]] for p in range(N + fl - 1))
                assert np.array_equal(comp[fl:], m[1:])                              # streaming positions: display frames 1 .. N - 1
                ff, fp = held_fold_arrays(m, widx, fl)
                assert sorted(fp) == list(range(fl))                                  # every head position exactly once
                assert all(ff[i] == comp[fp[i]] for i in range(fl))
                assert all((ff[i], fp[i]) < (ff[i + 1], fp[i + 1]) for i in range(fl - 1))      # sorted by frame, then position
                if kind == "identity":
                    f0, p0 = _fold_arrays(fold_list(widx, fl, N))
                    assert np.array_equal(ff, f0) and np.array_equal(fp, p0)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding", hc.PADDINGS)
def test_reference_is_the_transpose_of_the_forward(padding):
    rng = np.random.default_rng(5)
    for fl, N in ((1, 2), (6, 5), (8, 19), (15, 16), (30, 33)):
        widx = window_frame_indices(N, fl, padding)
        taps = rng.standard_normal((2, fl))
        for kind in hc.MAP_KINDS:
            m, F = hc.c_abi_map(kind, N)
            comp = href.composed(m, widx)
            M = href.forward_matrix(comp, taps, N, F)
            # the forward on the held stream is the dense forward on the expanded clip
            Mx = href.vref.forward_matrix(widx, taps, N)
            E = np.zeros((N, F))
            E[np.arange(N), m] = 1.0                                                  # index_select as a matrix
            assert np.abs(M - Mx @ E).max() <= 1e-13
            g0 = rng.standard_normal((N, 2, 7))
            want = np.einsum("vcj,vcx->jx", M, g0)
            got = href.dlum(comp, taps, g0, F)
            assert got.shape == (F, 7) and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
            shown = np.zeros(F, bool)
            shown[comp] = True
            assert (got[~shown] == 0).all()
            # <M x, y> = <x, M^T y>
            x = rng.standard_normal((F, 7))
            lhs = float((np.einsum("vcj,jx->vcx", M, x) * g0).sum())
            rhs = float((x * got).sum())
            assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0)
            S = href.dlum(comp, taps, g0, F, absolute=True)
            assert (S >= np.abs(got) - 1e-12).all() and (S[~shown] == 0).all()
            K = href.streaming_counts(m, F)
            assert K.sum() == N - 1 and len(K) == F


def test_head_shown_frames_stay_within_the_cap():
    """The derived bound of the end-to-end gradient test covers the source frames that no padding-head position shows; the case
    table keeps the others to half of either stream's frames at most."""
    for name, c in hc.ALL_CASES.items():
        (W, H), C, fps, padding, dtype, ts, rs, N, opt = c
        fl = hc.FL[fps]
        if padding != "replicate":
            assert N >= 2 * fl + 3, name
        widx = window_frame_indices(N, fl, padding)
        m_t, F_t, m_r, F_r = hc.case_maps(name)
        assert len(m_t) == len(m_r) == N and 12 <= N <= 70 or name.startswith("g_")
        for m, F in ((m_t, F_t), (m_r, F_r)):
            n = int(href.head_shown(m, widx, fl, F).sum())
            assert 1 <= n <= F // 2 or (F == 1), (name, n, F)
        t, r = hc.case_inputs(name)
        assert t.shape == (C, F_t, H, W) and r.shape == (C, F_r, H, W)
    assert {hc.ALL_CASES[n][2] for n in hc.CASES} == {30, 60, 120} and {hc.ALL_CASES[n][3] for n in hc.CASES} == set(hc.PADDINGS)
    assert {(c[0][0] * c[0][1]) % 4 for c in hc.CASES.values()} == {0, 2, 3}


def test_golden_loads():
    path = os.path.join(hc.GOLDEN, hc.GOLDEN_FILE)
    largest_g25 = max(os.path.getsize(os.path.join(hc.GOLDEN, f)) for f in os.listdir(hc.GOLDEN) if f.startswith("g25_"))
    assert os.path.getsize(path) <= largest_g25
    assert set(np.load(path).files) == {n + s for n in hc.GOLDEN_CASES for s in ("_jod", "_grad")}       # outputs only
    for name in hc.GOLDEN_CASES:
        (W, H), C = hc.GOLDEN_CASES[name][:2]
        jod, g = hc.load_golden(name)
        assert g.shape == (C, hc.case_maps(name)[1], H, W) and np.isfinite(g).all() and 0 < jod < 10 and g.any()


def test_new_kernels_do_not_spill():
    import codeobj
    nat.build()
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    names = list(md)
    nice = codeobj.demangle(names)
    found = {k: 0 for k in NEW_KERNELS}
    for mname, n in zip(names, nice):
        base = n.split("(")[0]
        if base in found:
            found[base] += 1
            x = md[mname]
            assert (x["sgpr_spill_count"], x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), n
        assert "held" not in base or base in found, n                # no instantiation beyond the list
    assert found == {k: 1 for k in found}
    # none of the names the other tests count by substring
    for n in NEW_KERNELS:
        assert "_half_kernel" not in n
        assert not any(s in n for s in ("temporal_vec_kernel<", "band2_kernel<", "band_kernel<", "temporal_ring_kernel<",
                                        "temporal_yuv_kernel<", "temporal_yuv_vec_kernel<", "video_input_kernel<",
                                        "yuvplanes_ring_kernel<", "video_lum_input_kernel<", "resized_ring_kernel<"))
