"""Resized clips shown through frame maps, without a GPU: the header and its binding, the argument checks of its two entry points,
the refusals of fvvdp.predict_resized / fvvdp.jod_video_resized with test_frames= / reference_frames= that come before any device
work (and the unchanged ones with both left at 1), the float64 restatement (tests/resize_held_ref.py) against the inner-product
identity and torch autograd, the three mutations the GPU tests' bounds must see, and the code objects of the new kernels."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd.fvvdp import window_frame_indices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import held_cases as hc                      # noqa: E402
import resize_cases as rc                    # noqa: E402
import resize_held_cases as rhc              # noqa: E402
import resize_held_ref as rhr                # noqa: E402
import resize_ref as rref                    # noqa: E402
import yuv_channels_ref as yref              # noqa: E402

U24 = 2.0 ** -24
WEIGHT_ULPS = 4              # test_resize_cpu.test_axis_matrices_are_torchs
NEW_KERNELS = ["void resized_hold_ring_kernel<%d, %d, %d>" % (fl, 2 if fl <= 16 and m <= 1 else 1, m) for fl in (8, 16, 32) for m in range(4)] + \
    ["void resize_adjoint_run_d_kernel<%d>" % m for m in range(5)]


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fvvdp_[a-z0-9_]+)\s*\(", txt)))


def test_resize_held_header_is_exported_and_bound():
    nat.build()
    names = declared("fvvdp_hip_resize_held.h")
    assert names == ["fvvdp_resize_grad_held", "fvvdp_temporal_channels_resized_held"]
    L = ctypes.CDLL(nat.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
    assert sorted(nat.RESIZE_HELD_SYMBOLS) == names
    lib = nat.lib()
    for name in names:
        assert getattr(lib, name).argtypes is not None, name
    assert not hasattr(L, "fvvdp_ctx_ingest_begin") and not hasattr(L, "resize_launch_gather")      # internal helpers stay internal
    exports = open(os.path.join(ROOT, "fovvideovdp_amd", "csrc", "exports.map")).read()
    assert "global: fvvdp_*;" in exports and all(n in exports for n in names)
    assert nat.resize_grad_held_table_bytes(60, 34, 5) == 1024 and nat.resize_grad_held_table_bytes(60, 34, 3) == 768
    assert nat.resize_grad_held_table_bytes(1920, 1080, 30) == 24320
    txt = open(os.path.join(ROOT, "include", "fvvdp_hip_resize_held.h")).read()
    assert "#define FVVDP_RESIZE_GRAD_HELD_TABLE_BYTES(width, height, n_source)" in txt
    # the unit is built without contraction of multiplies and adds, as resize_launch.hip
    src = open(os.path.join(ROOT, "fovvideovdp_amd", "_native.py")).read()
    assert re.search(r'"resize_held_launch\.hip"\), \["-ffp-contract=off"\]', src)
    import inspect
    for fn in (fv.fvvdp.predict_resized, fv.fvvdp.jod_video_resized):
        p = inspect.signature(fn).parameters
        assert p["test_frames"].default == 1 and p["reference_frames"].default == 1


def test_argument_checks_need_no_device():
    lib = nat.lib()
    p = ctypes.c_void_p
    i32p = ctypes.POINTER(ctypes.c_int32)
    e = nat.Eotf()
    w = np.ones(3, np.float32)
    Wo, Ho, N, F = 120, 68, 6, 3
    err = lib.fvvdp_last_error

    def stream(data=256, dtype=nat.FVVDP_F32, C=3, width=60, height=34, n=F):
        hw = width * height
        return nat.ResizeStream(data, dtype, C, width, height, hw, n * hw)

    def adj(gL=256, m=None, t=None, g=512, mode=1, kind=nat.EOTF_SRGB, width=Wo, n_display=N, n_source=F, work=1024, bytes_=1 << 30):
        e.kind = kind
        m = np.asarray((np.arange(n_display) // 2) if m is None else m, np.int32)
        return lib.fvvdp_resize_grad_held(width, Ho, n_display, n_source, p(gL), m.ctypes.data_as(i32p), ctypes.byref(t or stream()), p(g),
                                          mode, ctypes.byref(e), nat.fptr(w), p(work), bytes_, None)

    assert lib.fvvdp_resize_grad_held(Wo, Ho, N, F, None, None, None, None, 1, None, None, None, 0, None) == -1 and b"null" in err()
    assert adj(n_source=0) == -1 and b"bad shape" in err()
    assert adj(n_display=0, m=[0]) == -1 and b"bad shape" in err()
    assert adj(width=0) == -1 and b"bad shape" in err()
    assert adj(m=np.arange(N)) == -1 and b"frame map entry 3 names source frame 3 outside [0, 3)" in err()
    assert adj(m=[-1, 0, 0, 1, 1, 2]) == -1 and b"outside [0, 3)" in err()
    assert adj(m=[0, 1, 0, 1, 2, 2]) == -1 and b"non-decreasing (entry 2: 0 after 1)" in err()
    assert adj(mode=4) == -1 and b"unknown resize mode" in err()
    assert adj(kind=nat.EOTF_LUT) == -1 and b"closed-form" in err()
    assert adj(t=stream(dtype=nat.FVVDP_U8)) == -1 and b"the test must be float32 (" in err()
    assert adj(t=stream(width=32769, height=1)) == -1 and b"frame size out of range (1..32768 per axis): 32769x1 (test)" in err()
    assert adj(gL=258) == -1 and b"aligned to 4 bytes" in err()
    assert adj(work=1025) == -1 and b"256-byte aligned" in err()
    one = nat.resize_grad_held_table_bytes(60, 34, F) + 4 * 3 * Wo * Ho
    assert adj(bytes_=one - 1) == -1 and b"needed for one frame" in err()

    taps = np.ones((2, 40), np.float32)
    idx = np.zeros(64, np.int32)

    def ing(ctx=256, t=None, r=None, nt=F, nr=N, mode=1, kind=nat.EOTF_SRGB, fl=8, it=idx, ir=idx, n_out=4):
        e.kind = kind
        return lib.fvvdp_temporal_channels_resized_held(p(ctx), ctypes.byref(t or stream()), ctypes.byref(r or stream(dtype=nat.FVVDP_U8, n=N)),
                                                        nt, nr, mode, ctypes.byref(e), nat.fptr(w), it.ctypes.data_as(i32p),
                                                        ir.ctypes.data_as(i32p), nat.fptr(taps), fl, n_out, 0, None)

    assert ing(ctx=None) == -1 and b"null" in err()
    assert ing(mode=7) == -1 and b"unknown resize mode" in err()
    assert ing(fl=0) == -1 and b"filter length" in err()
    assert ing(fl=33) == nat.FVVDP_EUNSUPPORTED and b"up to 32 taps" in err()
    assert ing(kind=nat.EOTF_LUT) == -1 and b"closed-form" in err()
    assert ing(r=stream(dtype=nat.FVVDP_U16)) == -1 and b"the reference must be float32 or uint8" in err()
    assert ing(r=stream(C=1)) == -1 and b"differ in their channel counts (3 and 1)" in err()
    assert ing(nt=0) == -1 and b"at least one frame (test: 0, reference: 6)" in err()
    assert ing(n_out=0) == -1 and b"at least one output frame" in err()
    bad = idx.copy()
    bad[5] = F
    assert ing(it=bad) == -1 and b"list entry 5 names frame 3 outside the test's [0, 3)" in err()
    bad[5] = N
    assert ing(ir=bad) == -1 and b"list entry 5 names frame 6 outside the reference's [0, 6)" in err()
    assert ing(it=-np.ones(64, np.int32)) == -1 and b"outside the test's" in err()


def test_refusals_without_device():
    m = fv.fvvdp(display_name="standard_4k", device="cpu", quiet=True)
    t, r = torch.rand(1, 3, 4, 17, 30), torch.rand(1, 3, 8, 34, 60)
    for call, name in ((m.predict_resized, "predict_resized"), (m.jod_video_resized, "jod_video_resized")):
        # both keywords left at 1: today's refusals, in today's words
        with pytest.raises(RuntimeError, match=r"%s: test and reference differ in their frame counts \(4 and 8\)" % name):
            call(t, r, frames_per_second=30)
        with pytest.raises(RuntimeError, match=r"differ in their frame counts \(4 and 8\)"):
            call(t, r, frames_per_second=30, test_frames=1, reference_frames=np.int64(1))
        with pytest.raises(RuntimeError, match="needs clips: an F axis of at least 2 frames"):
            call(t[:, :, :1], r[:, :, :1], frames_per_second=30)
        # the maps: held.frame_map's ValueErrors, before the device is looked at
        for bad in (2.0, np.float32(2), True):
            with pytest.raises(ValueError, match="test_frames must be an int k >= 1 or a 1-D integer sequence"):
                call(t, r, frames_per_second=30, test_frames=bad)
        with pytest.raises(ValueError, match="must hold integers"):
            call(t, r, frames_per_second=30, test_frames=[0.0, 0.0, 1.0, 1.0, 2.0, 2.0, 3.0, 3.0])
        with pytest.raises(ValueError, match=r"test_frames must be non-decreasing \(entry 2: 0 after 1\)"):
            call(t, r, frames_per_second=30, test_frames=[0, 1, 0, 1, 2, 2, 3, 3])
        with pytest.raises(ValueError, match=r"test_frames names frame 4 outside the test's \[0, 4\)"):
            call(t, r, frames_per_second=30, test_frames=[0, 0, 1, 1, 2, 2, 3, 4])
        with pytest.raises(ValueError, match=r"reference_frames names frame -1 outside"):
            call(t, r, frames_per_second=30, test_frames=2, reference_frames=[-1, 0, 1, 2, 3, 4, 5, 6])
        with pytest.raises(ValueError, match="test_frames=0: a frame is held for k >= 1"):
            call(t, r, frames_per_second=30, test_frames=0)
        with pytest.raises(ValueError, match="the test is shown for 12 display frames and the reference for 8"):
            call(t, r, frames_per_second=30, test_frames=3)
        with pytest.raises(ValueError, match="the test is shown for 7 display frames and the reference for 8"):      # a wrong-length map
            call(t, r, frames_per_second=30, test_frames=[0, 0, 1, 1, 2, 2, 3])
        with pytest.raises(ValueError, match="at least 2 display frames, got 1"):
            call(t[:, :, :1], r[:, :, :1], frames_per_second=30, test_frames=[0])
        # what predict_resized refuses, with maps as without
        kw = dict(frames_per_second=30, test_frames=2)
        with pytest.raises(RuntimeError, match="Unknown resize method"):
            call(t, r, full_screen_resize="lanczos", **kw)
        with pytest.raises(RuntimeError, match=r"differ in their channel counts \(3 and 1\)"):
            call(t, r[:, :1], **kw)
        with pytest.raises(RuntimeError, match="frame rate too high: its temporal filter has 33 taps"):
            call(t, r, frames_per_second=130, test_frames=2)
        with pytest.raises(RuntimeError, match="takes float32 .*samples; the test is float64"):
            call(t.double(), r, **kw)
        with pytest.raises(RuntimeError, match="samples; the reference is float16"):
            call(t, r.half(), **kw)
        with pytest.raises(RuntimeError, match="needs clips"):
            call(t[0, :, 0], r[0, :, 0], dim_order="CHW", **kw)
        # everything accepted: the first device work is refused on a CPU metric
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(t, r, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):                    # a single frame held for the whole clip
            call(t[:, :, :1], r, frames_per_second=30, test_frames=8)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(t, r, frames_per_second=120, test_frames=np.arange(8) // 2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):                    # identity maps on equal counts: today's path
            call(r[..., :17, :30], r.clone(), frames_per_second=30, test_frames=list(range(8)), reference_frames=torch.arange(8))
    with pytest.raises(RuntimeError, match="gradients with respect to the reference are not supported"):
        m.jod_video_resized(t, r.clone().requires_grad_(True), frames_per_second=30, test_frames=2)
    with pytest.raises(RuntimeError, match="samples; the test is uint8"):
        m.jod_video_resized((t * 255).to(torch.uint8), r, frames_per_second=30, test_frames=2)
    with pytest.raises(RuntimeError, match="forward-only"):
        m.predict_resized(t.clone().requires_grad_(True), r, frames_per_second=30, test_frames=2)

    class MyDisplay(fv.fvvdp_display_photometry):
        def forward(self, V):
            return 100.0 * V + 0.5

        def get_peak_luminance(self):
            return 100.5

        def get_black_level(self):
            return 0.5

    user = fv.fvvdp(display_name="standard_4k", display_photometry=MyDisplay(), device="cpu", quiet=True)
    with pytest.raises(RuntimeError, match="needs a display model with a closed form"):
        user.predict_resized(t, r, frames_per_second=30, test_frames=2)


def test_rotation_covers_the_matrix():
    R = rhc.rotation()
    assert {c["maps"] for c in R} == set(rhc.MAPS) and {(c["mode"], c["fps"]) for c in R} == {(m, f) for m in rref.MODES for f in rc.FPS}
    for fps in rc.FPS:
        held_t = [c for c in R if c["fps"] == fps and rhc.MAPS[c["maps"]][0] != "identity"]
        held_r = [c for c in R if c["fps"] == fps and rhc.MAPS[c["maps"]][1] != "identity"]
        assert held_t and held_r
    # circular padding sends the list back to frame 0 behind a held frame: the index changes, so the step must convert
    assert any(c["padding"] == "circular" and rhc.MAPS[c["maps"]][0] != "identity" for c in R)
    for c in R:
        N = rc.RING[c["fps"]] + 3
        m_t, F_t, m_r, F_r = rhc.case_maps(c["maps"], N)
        assert len(m_t) == len(m_r) == N and m_t.max() < F_t and m_r.max() < F_r
    m_t, F_t, m_r, F_r = rhc.case_maps("both", 11)
    assert F_t != F_r and not np.array_equal(m_t, m_r)
    m_t, F_t, _, _ = rhc.case_maps("skipping", 11)
    shown = np.zeros(F_t, bool)
    shown[m_t] = True
    assert (~shown).sum() >= 3 and not shown[-1]
    assert list(rhr.run_table([0, 0, 1, 3, 3, 3], 5)) == [0, 2, 3, 3, 6, 6]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def _small(c, N=6):
    test, ref, m_t, m_r = rhc.inputs(c, N)
    return test, ref, m_t, m_r, N


@pytest.mark.parametrize("mode", rref.MODES)
def test_adjoint_satisfies_the_inner_product_identity(mode):
    """<A x, y> = <x, A^T y> for A = resize o hold, with the whole restated adjoint (linear display model, samples clear of the
    clip, weights of one): to 1e-12, the bound test_resize_cpu.py uses for the resize alone."""
    for k, (source, target) in enumerate([(s, t) for s in rc.SOURCES for t in rc.TARGETS]):
        kind = list(rhc.MAPS)[k % len(rhc.MAPS)]
        N = 7
        m, F = hc.c_abi_map(rhc.MAPS[kind][0] if rhc.MAPS[kind][0] != "identity" else "hold3", N)
        rng = np.random.default_rng(source[0] * target[0] + N)
        x = rng.uniform(0.3, 0.7, (3, F, source[1], source[0]))
        y = rng.standard_normal((N, target[1], target[0]))
        lhs = float((rhr.hold_resize(x, m, target, mode) * y[None]).sum())
        adj = rhr.adjoint(y, x, m, target, mode, np.ones(3), rref.eotf_args(rref.yref.orc.Photometry(1000, EOTF="linear"))[0], Y_peak=1000.0)
        rhs = float((x * adj).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (mode, source, target, kind)
        shown = np.zeros(F, bool)
        shown[m] = True
        assert (adj[:, ~shown] == 0).all()


@pytest.mark.parametrize("mode", rref.MODES)
def test_adjoint_is_torchs_autograd(mode):
    """index_select -> interpolate -> clip under torch autograd in float32 against the float64 adjoint of the run sums.  A source
    sample sums K T terms, K the display frames that show its frame and T the target samples that reach it: the term-count bound
    of test_resize_cpu.test_adjoint_is_torchs_autograd with K T in the place of T."""
    zeros = 0
    for k, (source, target) in enumerate([(s, t) for s in rc.SOURCES[:4] for t in rc.TARGETS]):
        N = 6
        m, F = hc.c_abi_map(("hold2", "pulldown", "skip", "hold4")[k % 4], N)
        x, _ = rc.draw_clip([4, *source, *target], 3, F, source, target, mode)
        rng = np.random.default_rng(source[1] * target[0])
        G = (rng.uniform(0.25, 2.0, (3, N, target[1], target[0])) * rng.choice([-1.0, 1.0], (3, N, target[1], target[0]))).astype(np.float32)
        xt = torch.from_numpy(x.copy()).requires_grad_(True)
        xe = xt.index_select(1, torch.from_numpy(m.astype(np.int64)))
        y = torch.nn.functional.interpolate(xe.permute(1, 0, 2, 3), size=(target[1], target[0]), mode=mode,
                                            **({} if mode in ("nearest", "area") else {"align_corners": False}))
        (y.clip(0, 1).permute(1, 0, 2, 3) * torch.from_numpy(G)).sum().backward()
        want = xt.grad.numpy()
        Ty = int((rref.axis_matrix(source[1], target[1], mode) != 0).sum(axis=0).max())
        Tx = int((rref.axis_matrix(source[0], target[0], mode) != 0).sum(axis=0).max())
        Sy, Sx = (rref.axis_support(source[i], target[i], mode).astype(np.float64) for i in (1, 0))
        r = rhr.run_table(m, F)
        for j in range(F):
            K = int(r[j + 1] - r[j])
            Gs = G[:, r[j]:r[j + 1]].astype(np.float64).sum(axis=1) if K else np.zeros_like(G[:, 0], dtype=np.float64)
            Ga = np.abs(G[:, r[j]:r[j + 1]]).astype(np.float64).sum(axis=1) if K else np.zeros_like(G[:, 0], dtype=np.float64)
            got = rref.clip_adjoint(Gs, x[:, j], target, mode)
            scale = rref.clip_adjoint(Ga, x[:, j], target, mode, absolute=True)
            v = rref.resize(x[:, j].astype(np.float64), target, mode)
            taps = np.matmul(np.matmul(Sy.T, Ga * ((v >= 0) & (v <= 1))), Sx)
            assert (np.abs(got - want[:, j]) <= (max(K, 1) * Ty * Tx + 4) * U24 * scale + WEIGHT_ULPS * U24 * sum(source) * taps).all(), (mode, source, j)
            assert (want[:, j][scale == 0] == 0).all() and (got[scale == 0] == 0).all()
            zeros += int((scale == 0).sum())
            if K == 0:
                assert (want[:, j] == 0).all()
    assert zeros > 0


def test_forward_steps_is_the_expanded_forward():
    """What the kernel does -- walk each stream's composed list and take the previous luminance where the entry repeats -- gives the
    expanded clips' level 0 exactly, in float64 and in float32."""
    for c in rhc.rotation()[::4]:
        test, ref, m_t, m_r, N = _small(c, 9)
        m = fv.fvvdp(temp_padding=c["padding"], quiet=True, device="cpu", display_name="standard_fhd")
        fl, taps = m._temporal_taps(c["fps"])
        widx = window_frame_indices(N, fl, c["padding"])
        idx = np.stack([widx[f:f + fl] for f in range(N)])
        ph = yref.photometry_for("standard_fhd")
        w = np.asarray(yref.orc.load_defaults()["color_spaces.json"]["sRGB"]["RGB2Y"], np.float32)
        for dt in (np.float64, np.float32):
            want, _ = rhr.forward(test, ref, m_t, m_r, c["target"], c["mode"], ph, w, taps, idx, dt)
            got = rhr.forward_steps(test, ref, m_t, m_r, c["target"], c["mode"], ph, w, taps, widx, fl, dt)
            assert np.array_equal(got, want), rhc.case_id(c)


# ---- the bounds see a wrong kernel ----------------------------------------------------------------------------------------------------
def test_bounds_see_a_wrong_kernel():
    """Each of three mutated float32 restatements exceeds what the GPU tests assert: equal bits for the ingest (any difference from
    the expanded forward shows), and for the adjoint 4 x the float32 restatement's own error relative to the sum of a sample's
    absolute terms (yuv_channels_ref.error_bound)."""
    c = next(x for x in rhc.rotation() if x["maps"] == "both")
    test, ref, m_t, m_r, N = _small(c, 9)
    m = fv.fvvdp(temp_padding=c["padding"], quiet=True, device="cpu", display_name="standard_fhd")
    fl, taps = m._temporal_taps(c["fps"])
    widx = window_frame_indices(N, fl, c["padding"])
    ph = yref.photometry_for("standard_fhd")
    w = np.asarray(yref.orc.load_defaults()["color_spaces.json"]["sRGB"]["RGB2Y"], np.float32)
    a = (test, ref, m_t, m_r, c["target"], c["mode"], ph, w, taps, widx, fl, np.float32)
    good = rhr.forward_steps(*a)
    for mutation in ("sticky", "list0"):          # a reuse across a change of index; stream 1 reading stream 0's list
        bad = rhr.forward_steps(*a, mutate=mutation)
        assert not np.array_equal(bad, good), mutation
        assert np.abs(bad - good).max() > 1e-3 * np.abs(good).max(), mutation         # (and not by a last bit)
    # a run sum that drops its last display frame
    c = next(x for x in rhc.rotation() if x["maps"] == "k2" and x["mode"] == "bilinear")
    test, _, m_t, _, N = _small(c, 6)
    kind, kw = rref.eotf_args(ph)
    gL = rhc.gl_for(c, N)
    args = (gL, test, m_t, c["target"], c["mode"], w, kind)
    g64 = rhr.adjoint(*args, dtype=np.float64, **kw)
    g32 = rhr.adjoint(*args, dtype=np.float32, **kw)
    S = rhr.adjoint(*args, dtype=np.float64, absolute=True, **kw)
    bad = rhr.adjoint(*args, dtype=np.float32, drop_last=True, **kw)
    nz = S != 0
    e_ref = float((np.abs(g32.astype(np.float64) - g64)[nz] / S[nz]).max())
    err = float((np.abs(bad.astype(np.float64) - g64)[nz] / S[nz]).max())
    assert e_ref <= 1e-5 and err > 100 * yref.error_bound(e_ref), (e_ref, err)


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
            # nothing private, no register of either kind spilled: stricter than the ring kernels these were made from
            assert (x["sgpr_spill_count"], x["vgpr_spill_count"], x["private_segment_fixed_size"]) == (0, 0, 0), n
        assert "hold_ring" not in base and "run_d_kernel" not in base or base in found, n       # no instantiation beyond the list
    assert found == {k: 1 for k in found}
    # none of the names the other tests count by substring
    for n in NEW_KERNELS:
        assert "held" not in n
        assert not any(s in n for s in ("temporal_vec_kernel<", "band2_kernel<", "band_kernel<", "temporal_ring_kernel<",
                                        "temporal_yuv_kernel<", "temporal_yuv_vec_kernel<", "video_input_kernel<",
                                        "yuvplanes_ring_kernel<", "video_lum_input_kernel<", "resized_ring_kernel<",
                                        "resize_adjoint_d_kernel<", "resize_adjoint_gather_kernel<", "still_ingest_kernel<"))
