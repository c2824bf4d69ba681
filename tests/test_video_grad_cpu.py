"""Video gradients without a GPU: the fourth C header and its binding, the argument checks of its entry points, the code
objects of the new kernels, the host's fold list, and the refusals of fvvdp.jod_video that come before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd.fvvdp import window_frame_indices
from fovvideovdp_amd.video_grad import _fold_arrays, fold_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KERNELS = ("video_coef_kernel", "video_layer_kernel", "video_level0_kernel")
INPUT_KERNELS = ["void video_input_kernel<%d, %d>" % (fl, px) for fl, px in
                 ((8, 4), (8, 1), (16, 4), (16, 1), (32, 2), (32, 1), (64, 2), (64, 1))]


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def test_video_grad_header_is_exported_and_bound():
    nat.build()
    names = declared("fvvdp_hip_video_grad.h")
    assert names == ["fvvdp_video_grad_frames", "fvvdp_video_grad_input", "fvvdp_video_grad_workspace"]
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert sorted(nat.VIDEO_GRAD_SYMBOLS) == names
    assert not set(names) & (set(nat.SYMBOLS) | set(nat.IMAGE_SYMBOLS) | set(nat.GRAD_SYMBOLS))
    assert len(declared("fvvdp_hip.h")) == 24 and len(declared("fvvdp_hip_images.h")) == 3
    assert declared("fvvdp_hip_grad.h") == ["fvvdp_images_grad", "fvvdp_images_grad_workspace"]
    lib = nat.lib()
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    assert not hasattr(L, "grad_sweep_launch") and not hasattr(L, "fvvdp_fail_from")     # internal helpers stay internal
    txt = open(os.path.join(ROOT, "include", "fvvdp_hip_video_grad.h")).read()
    assert int(re.search(r"#define FVVDP_VIDEO_GRAD_MAX_TAPS (\d+)", txt).group(1)) == nat.VIDEO_GRAD_MAX_TAPS


def test_workspace_matches_its_documented_layout():
    lib = nat.lib()
    nbytes = ctypes.c_size_t(0)
    assert lib.fvvdp_video_grad_workspace(64, 48, 4, 3, None) == -1
    assert lib.fvvdp_video_grad_workspace(64, 48, 0, 3, ctypes.byref(nbytes)) == -1
    assert lib.fvvdp_video_grad_workspace(64, 48, 17, 3, ctypes.byref(nbytes)) == -1
    assert lib.fvvdp_video_grad_workspace(64, 48, 4, 0, ctypes.byref(nbytes)) == -1
    assert lib.fvvdp_video_grad_workspace(0, 48, 4, 3, ctypes.byref(nbytes)) == -1
    assert lib.fvvdp_video_grad_workspace(64, 48, 4, 3, ctypes.byref(nbytes)) == 0
    # coefficients [n][2][bands] + layer gradients of levels 0..3 + sweep gradients of levels 1..4, two planes per frame,
    # each part 256-byte aligned
    sizes = [(64, 48), (32, 24), (16, 12), (8, 6), (4, 3)]
    al = lambda x: (x + 63) // 64 * 64
    expect = al(3 * 2 * 4) + sum(al(3 * 2 * w * h) for w, h in sizes[:4]) + sum(al(3 * 2 * w * h) for w, h in sizes[1:])
    assert nbytes.value == 4 * expect


def test_frames_argument_checks_need_no_device():
    lib = nat.lib()
    assert lib.fvvdp_video_grad_frames(64, 48, 4, 2, None, None, None, 5, 0, None, None, None, None, 0, None) == -1
    assert b"null" in lib.fvvdp_last_error()
    prm, pp = nat.Params(), nat.PoolParams(1, 0.67, 1, 0.25, -0.016, 0.6)
    prm.beta = 0.96
    maps = (nat.BandMaps * 4)()
    for b in range(4):
        maps[b].d_D = maps[b].d_contrast = maps[b].d_lbkg = maps[b].d_S = 256
    p = ctypes.c_void_p(256)

    def call(n_bands=4, n=2, n_frames=5, f0=0, work=1 << 30, work_ptr=256, mp=maps, pool=pp):
        return lib.fvvdp_video_grad_frames(64, 48, n_bands, n, ctypes.byref(prm), ctypes.byref(pool), p, n_frames, f0, p, mp, p,
                                           ctypes.c_void_p(work_ptr), work, None)

    assert call(n_bands=17) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert call(n=0) == -1
    assert call(f0=4) == -1 and b"outside the clip" in lib.fvvdp_last_error()
    assert call(f0=-1) == -1
    assert call(n_frames=1) == -1
    assert call(work=16) == -1 and b"workspace" in lib.fvvdp_last_error()
    assert call(work_ptr=260) == -1 and b"aligned" in lib.fvvdp_last_error()
    assert call(pool=nat.PoolParams(1, 0.67, 0, 0.25, -0.016, 0.6)) == -1 and b"exponents" in lib.fvvdp_last_error()
    holes = (nat.BandMaps * 4)()
    for b in range(4):
        holes[b].d_D = holes[b].d_contrast = holes[b].d_lbkg = 256
    assert call(mp=holes) == -1 and b"every map" in lib.fvvdp_last_error()


def test_input_argument_checks_need_no_device():
    lib = nat.lib()
    i32p = ctypes.POINTER(ctypes.c_int32)
    assert lib.fvvdp_video_grad_input(64, 48, 5, None, None, None, None, 8, None, None, 3, 0, 0, None, None, None, 0, None) == -1
    assert b"null" in lib.fvvdp_last_error()
    e = nat.Eotf()
    w = np.array([0.2126, 0.7152, 0.0722], np.float32)
    p = ctypes.c_void_p(256)
    HW = 64 * 48

    def call(fl=8, N=5, C=3, kind=nat.EOTF_SRGB, head=1 << 30, ff=None, fp=None, frame_stride=HW, chan_stride=5 * HW, width=64):
        e.kind = kind
        n = max(1, min(fl, 256))
        ff = np.zeros(n, np.int32) if ff is None else np.asarray(ff, np.int32)
        fp = np.arange(n, dtype=np.int32) if fp is None else np.asarray(fp, np.int32)
        taps = np.ones((2, n), np.float32)
        return lib.fvvdp_video_grad_input(width, 48, N, p, ff.ctypes.data_as(i32p), fp.ctypes.data_as(i32p), nat.fptr(taps), fl, p, p,
                                          C, chan_stride, frame_stride, ctypes.byref(e), nat.fptr(w), p, head, None)

    assert call(width=0) == -1 and b"bad shape" in lib.fvvdp_last_error()
    assert call(N=0) == -1
    assert call(fl=0) == -1 and b"filter length" in lib.fvvdp_last_error()
    assert call(fl=257) == -1 and b"filter length" in lib.fvvdp_last_error()
    assert call(fl=65) == nat.FVVDP_EUNSUPPORTED and b"64" in lib.fvvdp_last_error()       # the ring's reach, said in the header
    assert call(C=2) == -1 and b"colour channels" in lib.fvvdp_last_error()
    assert call(kind=nat.EOTF_LUT) == -1 and b"closed-form" in lib.fvvdp_last_error()
    assert call(kind=nat.EOTF_NONE) == -1
    assert call(head=8 * HW * 4 - 1) == -1 and b"side buffer" in lib.fvvdp_last_error()
    assert call(frame_stride=HW - 1) == -1 and b"frame_stride" in lib.fvvdp_last_error()
    assert call(chan_stride=HW - 1) == -1 and b"chan_stride" in lib.fvvdp_last_error()
    # the fold list: frames inside the clip, every head position once, sorted
    assert call(ff=[0] * 7 + [5]) == -1 and b"outside [0, 5)" in lib.fvvdp_last_error()
    assert call(ff=[-1] + [0] * 7) == -1 and b"outside [0, 5)" in lib.fvvdp_last_error()
    assert call(fp=[0, 1, 2, 3, 4, 5, 6, 8]) == -1 and b"head position" in lib.fvvdp_last_error()
    assert call(fp=[0, 1, 2, 3, 4, 5, 6, 6]) == -1 and b"listed twice" in lib.fvvdp_last_error()
    assert call(ff=[1] + [0] * 7) == -1 and b"sorted" in lib.fvvdp_last_error()
    assert call(fp=[1, 0, 2, 3, 4, 5, 6, 7]) == -1 and b"sorted" in lib.fvvdp_last_error()


def test_new_kernels_do_not_spill():
    import codeobj
    nat.build()
    md = codeobj.kernel_metadata(nat.LIB_PATH)
    names = list(md)
    nice = codeobj.demangle(names)
    found = {k: 0 for k in NEW_KERNELS + tuple(INPUT_KERNELS)}
    for m, n in zip(names, nice):
        base = n.split("(")[0]
        if base in found:
            found[base] += 1
            x = md[m]
            assert (x["sgpr_spill_count"], x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), n
    assert found == {k: 1 for k in found}
    # the shared helpers moved to a header of their own: the four kernels of the image backward are still defined once
    for k in ("grad_coef_kernel", "adj_layer_kernel", "adj_sweep_kernel", "grad_input_kernel"):
        assert sum(1 for n in nice if n.split("(")[0] == k) == 1, k


@pytest.mark.parametrize("N,fl", [(2, 30), (10, 15), (12, 8), (9, 8), (8, 8), (3, 1), (5, 64)])
@pytest.mark.parametrize("padding", ["replicate", "circular", "pingpong"])
def test_fold_list_is_the_transpose_of_the_window_list(N, fl, padding):
    idx = window_frame_indices(N, fl, padding)
    folds = fold_list(idx, fl, N)
    # brute force: every (output frame t, tap k) pair reads list position t + fl - 1 - k; transposed per source frame
    reads = {j: [] for j in range(N)}
    for t in range(N):
        for k in range(fl):
            p = t + fl - 1 - k
            reads[int(idx[p])].append(p)
    for j in range(N):
        positions = sorted(set(reads[j]))
        head = [p for p in positions if p < fl]
        stream = [p for p in positions if p >= fl]
        assert folds[j] == head, (j, folds[j], head)
        assert stream == ([j + fl - 1] if j >= 1 else []), (j, stream)
    ff, fp = _fold_arrays(folds)
    assert len(ff) == fl and sorted(fp.tolist()) == list(range(fl))
    assert all((ff[i], fp[i]) < (ff[i + 1], fp[i + 1]) for i in range(fl - 1))
    if padding == "circular" and N > fl + 1:          # the head is frames N - 1 - fl .. N - 2: frame 0 only for N = fl + 1
        assert folds[0] == []                         # no window shows frame 0: its gradient is zero
    if padding == "circular" and (N, fl) == (10, 15):
        assert max(len(f) for f in folds) == 2        # the head wraps round the clip
    if padding == "replicate":
        assert folds[0] == list(range(fl))


def test_jod_video_refusals_without_device():
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    x = torch.rand((1, 3, 4, 32, 48))
    r = torch.rand((1, 3, 4, 32, 48))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.jod_video(x.clone().requires_grad_(True), r, frames_per_second=30)
    with pytest.raises(RuntimeError, match="gradients with respect to the reference are not supported"):
        m.jod_video(x.clone().requires_grad_(True), r.clone().requires_grad_(True), frames_per_second=30)
    with pytest.raises(RuntimeError, match="jod_images"):
        m.jod_video(x[:, :, :1], r[:, :, :1], frames_per_second=30)
    with pytest.raises(RuntimeError, match="jod_images"):
        m.jod_video(x[:, :, 0], r[:, :, 0], dim_order="BCHW", frames_per_second=30)
    with pytest.raises(RuntimeError, match="B must be 1"):
        m.jod_video(torch.rand((2, 3, 4, 32, 48)), torch.rand((2, 3, 4, 32, 48)), frames_per_second=30)
    with pytest.raises(RuntimeError, match="float32"):
        m.jod_video(x.double(), r.double(), frames_per_second=30)
    with pytest.raises(RuntimeError, match="float32"):
        m.jod_video((x * 255).to(torch.uint8), (r * 255).to(torch.uint8), frames_per_second=30)
    with pytest.raises(RuntimeError, match="frames_per_second"):
        m.jod_video(x, r)
    with pytest.raises(RuntimeError, match="frame rate too high"):
        m.jod_video(x, r, frames_per_second=300)
    with pytest.raises(RuntimeError, match="colour channels"):
        m.jod_video(x[:, :2], r[:, :2], frames_per_second=30)
    with pytest.raises(RuntimeError, match="same shape"):
        m.jod_video(x, r[..., :40], frames_per_second=30)


def test_jod_video_refuses_user_photometry():
    class MyDisplay(fv.fvvdp_display_photometry):
        def forward(self, V):
            return 100.0 * V + 0.5

        def get_peak_luminance(self):
            return 100.5

        def get_black_level(self):
            return 0.5

    m = fv.fvvdp(display_name="standard_4k", display_photometry=MyDisplay(), device="cpu", quiet=True)
    with pytest.raises(RuntimeError, match="closed form"):
        m.jod_video(torch.rand((1, 3, 4, 32, 48)), torch.rand((1, 3, 4, 32, 48)), frames_per_second=30)


def test_jod_images_and_predict_refusals_are_unchanged():
    from fovvideovdp_amd.fvvdp import _refuse_grad
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    with pytest.raises(RuntimeError, match="F axis"):
        m.jod_images(torch.rand((1, 3, 2, 32, 48)), torch.rand((1, 3, 2, 32, 48)), dim_order="BCFHW")
    x = torch.zeros((1, 3, 4, 32, 48), requires_grad=True)
    with pytest.raises(RuntimeError, match=r"^Gradients through the metric are not supported on the HIP path.*jod_images.*jod_video"):
        _refuse_grad(x)
