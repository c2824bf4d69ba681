"""fvvdp.predict_tests_foveated on the GPU.  The yardstick is the existing path, never the new one:

    loop[k] = predict(tests[k], reference, fixation_point=gaze)          on the same metric object

and the contract is bit identity: every comparison below is torch.equal / np.array_equal, on Q_JOD and on Q_per_ch."""
import ctypes
import logging
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd.multitest import quad_plan
from fovvideovdp_amd.synth import synth_video_pair

pytestmark = pytest.mark.gpu

FPS = 30
# 250x131: three strips at level 0 (coarse width 125 > 122), odd heights at several levels (131, 33, 17, 9, 5: both parities of the
# reduce), 32750 pixels = no multiple of the temporal kernels' vector width (their per-pixel fallback runs)
H0, W0 = 131, 250


def _degrade(t, r, k):
    """Test k of a uint8 pair [1, C, N, H, W] (the kinds of tests/test_gpu_multitest.py): the generator's noisy test, a blur, the
    clip one frame late, the reference itself, then seeded noise of growing amplitude."""
    kind = k % 4 if k < 4 else 4
    if kind == 0:
        return t.clone()
    if kind == 1:
        x = r[0].permute(1, 0, 2, 3).to(torch.float32)
        x = F.avg_pool2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), 3, stride=1)
        return x.round().clamp(0, 255).to(torch.uint8).permute(1, 0, 2, 3)[None].contiguous()
    if kind == 2:
        return torch.roll(r, 1, dims=2).contiguous()
    if kind == 3:
        return r.clone()
    g = torch.Generator().manual_seed(100 + k)
    noise = torch.randint(-3 * k, 3 * k + 1, r.shape, generator=g)
    return (r.to(torch.int64) + noise).clamp(0, 255).to(torch.uint8)


def _as(x, dtype, gray=False):
    """A uint8 clip as the sample type `dtype`: the same picture on that type's scale."""
    if gray:
        x = x.to(torch.float32).mean(dim=1, keepdim=True).round().to(torch.uint8)
    if dtype == "uint8":
        return x.contiguous()
    if dtype == "uint16":
        return (x.numpy().astype(np.uint16) * 257)
    f = (x.to(torch.float32) / 255).contiguous()
    return f.to({"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}[dtype])


_pairs = {}


def _clips(N, H, W, T, dtype="uint8", gray=False):
    key = (N, H, W)
    if key not in _pairs:
        _pairs[key] = synth_video_pair(N, H, W, pair=3)
    t, r = _pairs[key]
    tests = [_as(_degrade(t, r, k), dtype, gray) for k in range(T)]
    ref = _as(r, dtype, gray)
    if dtype != "uint16":
        tests, ref = [x.cuda() for x in tests], ref.cuda()
    return tests, ref


def _gaze(kind, N, H=H0, W=W0):
    """fixed: a frame corner.  moving [N, 2]: a corner, the opposite corner, a point 500 pixels outside the frame (the eccentricity
    clamp), the centre, then points in between."""
    if kind == "fixed":
        return np.float32([W - 1, 0])
    pts = [(0, 0), (W - 1, H - 1), (W + 499, H // 2), (W // 2, H // 2), (0.31 * W, 0.77 * H), (0.9 * W, 0.2 * H), (W // 3, -500)]
    return np.ascontiguousarray(np.float32([pts[f % len(pts)] for f in range(N)]))


def _loop(m, tests, ref, gaze, fps=FPS, **kw):
    jod, Q = [], []
    for t in tests:
        q, st = m.predict(t, ref, frames_per_second=fps, fixation_point=gaze, **kw)
        jod.append(q.clone())
        Q.append(st["Q_per_ch"].copy())
    return torch.stack(jod), np.stack(Q)


def _same(q, st, jod, Q, shared=True):
    assert q.dtype is torch.float32 and q.is_cuda and tuple(q.shape) == (len(jod),)
    assert st["Q_per_ch"].shape == Q.shape and st["Q_per_ch"].dtype == np.float32
    print("max |dQ| %.3g, max |dJOD| %.3g" % (float(np.abs(st["Q_per_ch"] - Q).max()), float((q - jod).abs().max())))
    assert np.array_equal(st["Q_per_ch"], Q)
    assert torch.equal(q, jod)
    assert st["shared_pass"] is shared


_base = {}


def _base_case(kind="moving"):
    """(metric, 8 tests, reference, gaze, the loop of predict calls) of the 250x131 x 5 uint8 RGB case under the fixed or the moving
    gaze -- made once, never changed."""
    if "clips" not in _base:
        _base["clips"] = _clips(5, H0, W0, 8) + (fv.fvvdp(display_name="standard_4k", foveated=True),)
    tests, ref, m = _base["clips"]
    if kind not in _base:
        gaze = _gaze(kind, 5)
        _base[kind] = (m, tests, ref, gaze) + _loop(m, tests, ref, gaze)
    return _base[kind]


@pytest.mark.parametrize("kind", ["fixed", "moving"])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 8])
def test_rows_equal_predict(T, kind):
    """Odd T: the last test shares the reference's quad; even T: the reference stands alone in its quad; T = 8: two launch groups."""
    m, tests, ref, gaze, jod, Q = _base_case(kind)
    q, st = m.predict_tests_foveated(tests[:T], ref, frames_per_second=FPS, fixation_point=gaze)
    _same(q, st, jod[:T], Q[:T])
    assert st["N_frames"] == 5 and st["width"] == W0 and st["height"] == H0 and st["frames_per_second"] == FPS
    assert len(st["rho_band"]) == Q.shape[1] + 1


def test_tests_and_gaze_both_matter():
    _, _, _, _, jod_f, Q_f = _base_case("fixed")
    _, _, _, _, jod_m, Q_m = _base_case("moving")
    assert len(set(float(v) for v in jod_m)) >= 2 and len(set(float(v) for v in jod_f)) >= 2
    differ = [k for k in range(8) if k != 3 and not np.array_equal(Q_f[k], Q_m[k])]       # (test 3 is the reference: Q = 0 anyhow)
    assert len(differ) >= 2 and not torch.equal(jod_f, jod_m)


def test_the_default_gaze_is_the_centre():
    m, tests, ref, _, _, _ = _base_case()
    jod, Q = _loop(m, tests[:2], ref, None)
    q, st = m.predict_tests_foveated(tests[:2], ref, frames_per_second=FPS)
    _same(q, st, jod, Q)
    q, st = m.predict_tests_foveated(tests[:2], ref, frames_per_second=FPS, fixation_point=[W0 // 2, H0 // 2])
    _same(q, st, jod, Q)


@pytest.mark.parametrize("name,H,W,gray,dtype", [("gray5x9", 5, 9, True, "float32"), ("rgb135x240", 135, 240, False, "uint8")])
def test_two_chunks_and_two_strips(name, H, W, gray, dtype):
    """5x9: the smallest frame whose level 0 is walked in two chunks; 135x240: two strips at level 0."""
    tests, ref = _clips(4, H, W, 3, dtype, gray)
    gaze = _gaze("moving", 4, H, W)
    m = fv.fvvdp(display_name="standard_4k", foveated=True)
    jod, Q = _loop(m, tests, ref, gaze)
    for T in (2, 3):
        q, st = m.predict_tests_foveated(tests[:T], ref, frames_per_second=FPS, fixation_point=gaze)
        _same(q, st, jod[:T], Q[:T])


@pytest.mark.parametrize("cap", [2, 3])
def test_group_caps_give_the_same_bits(cap, monkeypatch):
    """FVVDP_TESTS_GROUP (read when a context is created): cap 2, every launch reads the reference's quad and one other."""
    _, tests, ref, gaze, jod, Q = _base_case()
    monkeypatch.setenv("FVVDP_TESTS_GROUP", str(cap))
    m = fv.fvvdp(display_name="standard_4k", foveated=True)
    for T in (7, 8):
        q, st = m.predict_tests_foveated(tests[:T], ref, frames_per_second=FPS, fixation_point=gaze)
        _same(q, st, jod[:T], Q[:T])


@pytest.mark.parametrize("T,cap", [(1, 3), (2, 3), (5, 3), (8, 3), (7, 2)])
def test_launched_groups_are_the_host_plan(T, cap, monkeypatch, capfd):
    """The groups the library launches (its FVVDP_DEBUG_VARIANT lines) are multitest.quad_plan's, on every band."""
    _, tests, ref, gaze, jod, Q = _base_case()
    monkeypatch.setenv("FVVDP_DEBUG_VARIANT", "1")
    monkeypatch.setenv("FVVDP_TESTS_GROUP", str(cap))
    m = fv.fvvdp(display_name="standard_4k", foveated=True)
    capfd.readouterr()
    q, st = m.predict_tests_foveated(tests[:T], ref, frames_per_second=FPS, fixation_point=gaze)
    err = capfd.readouterr().err
    _same(q, st, jod[:T], Q[:T])
    got = re.findall(r"level (\d+): multitest_fov_kernel<(\d+), (true|false)>, n (\d+), quads (\d+)\.\., .*lut_lds 1, store_ref (\d)", err)
    qp = quad_plan(T, 5, cap)
    want = [(str(b), str(len(g["quads"])), "true" if (T - 1) in g["tests"] and T % 2 else "false", "5",
             str(g["quads"][1] if len(g["quads"]) > 1 else 0), "1" if qp.ref_quad in g["store"] else "0")
            for b in range(Q.shape[1]) for g in qp.groups]
    assert got == want
    assert "band_kernel<" not in err and "multitest_kernel<" not in err


def test_batches_shorter_than_the_clip():
    """batch_frames = 2 on 5 frames: three batches, the last one short -- every batch takes its own rows of the gaze trace."""
    _, tests, ref, gaze, _, _ = _base_case()
    m = fv.fvvdp(display_name="standard_4k", foveated=True, batch_frames=2)
    jod, Q = _loop(m, tests[:5], ref, gaze)
    for T in (4, 5):
        q, st = m.predict_tests_foveated(tests[:T], ref, frames_per_second=FPS, fixation_point=gaze)
        _same(q, st, jod[:T], Q[:T])


def test_several_passes_when_the_scratch_budget_is_short():
    """A budget of two quads: five tests go in two passes (three tests, then two), each with the reference; one quad: one test
    per pass."""
    m, tests, ref, gaze, jod, Q = _base_case()
    per_frame = W0 * H0 * 4 * 4 * 1.34
    try:
        for quads in (2, 1):
            m.tests_scratch_bytes = quads * 5 * per_frame + 1
            q, st = m.predict_tests_foveated(tests[:5], ref, frames_per_second=FPS, fixation_point=gaze)
            _same(q, st, jod[:5], Q[:5])
    finally:
        m.tests_scratch_bytes = None


@pytest.mark.parametrize("dtype,gray", [("uint16", False), ("float16", False), ("bfloat16", False), ("uint8", True)])
def test_sample_types_and_channels(dtype, gray):
    tests, ref = _clips(4, H0, W0, 3, dtype, gray)
    gaze = _gaze("moving", 4)
    m = fv.fvvdp(display_name="standard_4k", foveated=True)
    jod, Q = _loop(m, tests, ref, gaze)
    q, st = m.predict_tests_foveated(tests, ref, frames_per_second=FPS, fixation_point=gaze)
    _same(q, st, jod, Q)


def test_a_display_whose_clamps_can_bind():
    tests, ref = _clips(4, H0, W0, 2, "float32")
    gaze = _gaze("moving", 4)
    m = fv.fvvdp(display_name="standard_hdr_pq", foveated=True)
    jod, Q = _loop(m, tests, ref, gaze)
    q, st = m.predict_tests_foveated(tests, ref, frames_per_second=FPS, fixation_point=gaze)
    _same(q, st, jod, Q)


@pytest.mark.parametrize("padding", ["replicate", "circular", "pingpong"])
def test_temporal_padding(padding):
    _, tests, ref, gaze, _, _ = _base_case()
    m = fv.fvvdp(display_name="standard_4k", foveated=True, temp_padding=padding)
    jod, Q = _loop(m, tests[:2], ref, gaze)
    q, st = m.predict_tests_foveated(tests[:2], ref, frames_per_second=FPS, fixation_point=gaze)
    _same(q, st, jod, Q)


def test_sixteen_taps():
    tests, ref = _clips(6, H0, W0, 3)
    gaze = _gaze("moving", 6)
    m = fv.fvvdp(display_name="standard_4k", foveated=True)
    jod, Q = _loop(m, tests, ref, gaze, fps=60)
    assert 9 <= m.filter_len <= 16                                     # the 16-slot ring of the temporal kernels
    q, st = m.predict_tests_foveated(tests, ref, frames_per_second=60, fixation_point=gaze)
    _same(q, st, jod, Q)


def test_dim_order_and_host_arrays():
    m, tests, ref, gaze, jod, Q = _base_case()
    tt = [t[0].permute(1, 2, 3, 0).cpu().numpy() for t in tests[:3]]             # FHWC on the host
    q, st = m.predict_tests_foveated(tuple(tt), ref[0].permute(1, 2, 3, 0).cpu().numpy(), dim_order="FHWC", frames_per_second=FPS,
                                     fixation_point=torch.from_numpy(gaze))
    _same(q, st, jod[:3], Q[:3])


def test_a_row_does_not_depend_on_the_other_tests():
    m, tests, ref, gaze, jod, Q = _base_case()
    order = [2, 0, 3, 1]
    q, st = m.predict_tests_foveated([tests[k] for k in order], ref, frames_per_second=FPS, fixation_point=gaze)
    _same(q, st, jod[order], Q[order])
    q, st = m.predict_tests_foveated([tests[5], tests[6], tests[2], tests[7]], ref, frames_per_second=FPS, fixation_point=gaze)
    assert torch.equal(q[2], jod[2]) and np.array_equal(st["Q_per_ch"][2], Q[2])


def test_a_test_identical_to_the_reference():
    m, tests, ref, gaze, jod, Q = _base_case()
    assert torch.equal(tests[3], ref)
    for group in ([tests[3]], [tests[0], tests[3]], [tests[0], tests[1], tests[3]]):      # beside the reference, and in another quad
        q, st = m.predict_tests_foveated(group, ref, frames_per_second=FPS, fixation_point=gaze)
        assert float(q[-1]) == 10.0
        assert torch.equal(q[-1], jod[3]) and np.array_equal(st["Q_per_ch"][-1], Q[3])


def test_a_second_run_and_no_residue_of_other_calls():
    """The same call twice, and again after a non-foveated predict and a predict_gazes call of the same frame size."""
    m, tests, ref, gaze, jod, Q = _base_case()
    for _ in range(2):
        q, st = m.predict_tests_foveated(tests[:5], ref, frames_per_second=FPS, fixation_point=gaze)
        _same(q, st, jod[:5], Q[:5])
    plain = fv.fvvdp(display_name="standard_4k")
    plain.predict(tests[0], ref, frames_per_second=FPS)
    m.predict_gazes(tests[1], ref, np.stack([gaze[::-1], gaze]), frames_per_second=FPS)
    q, st = m.predict_tests_foveated(tests[:5], ref, frames_per_second=FPS, fixation_point=gaze)
    _same(q, st, jod[:5], Q[:5])


def _call_stats(m):
    out = (ctypes.c_int64 * 3)()
    nat.check(nat.lib().fvvdp_ctx_call_stats(m._ctx.handle, out))
    return [int(v) for v in out]


def test_second_call_neither_allocates_nor_synchronises_in_the_library(monkeypatch):
    _, tests, ref, gaze, jod, Q = _base_case()
    m = fv.fvvdp(display_name="standard_4k", foveated=True, batch_frames=3)
    m.predict_tests_foveated(tests[:5], ref, frames_per_second=FPS, fixation_point=gaze)      # warm-up: the context, the LUT slices
    s0 = _call_stats(m)
    syncs = []
    real = torch.cuda.Stream.synchronize
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (syncs.append(1), real(self))[1])
    q, st = m.predict_tests_foveated(tests[:5], ref, frames_per_second=FPS, fixation_point=gaze)
    assert _call_stats(m) == s0                                        # syncs, allocations, frees inside the library: none added
    assert len(syncs) == 1                                             # the one result copy
    assert tuple(q.shape) == (5,)


def test_out_of_range_warning_once(caplog):
    tests, ref = _clips(4, H0, W0, 3, "float32")
    tests = [t.clone() for t in tests]
    tests[1][0, 1, 2, 7, 9] = 1.5
    m = fv.fvvdp(display_name="standard_4k", foveated=True)
    with caplog.at_level(logging.WARNING):
        m.predict_tests_foveated(tests, ref, frames_per_second=FPS)
    assert sum("outside the valid range" in rec.getMessage() for rec in caplog.records) == 1


def test_a_display_without_lds_slices_takes_the_loop(monkeypatch, capfd):
    """standard_hmd: every band's slice of the CSF table spans 8-9 rho intervals and does not fit the LDS.  The call is the loop of
    predict calls: same bits, shared_pass False, no launch of the new kernel."""
    tests, ref = _clips(4, 135, 240, 3)
    gaze = _gaze("moving", 4, 135, 240)
    monkeypatch.setenv("FVVDP_DEBUG_VARIANT", "1")
    m = fv.fvvdp(display_name="standard_hmd", foveated=True)
    jod, Q = _loop(m, tests, ref, gaze)
    capfd.readouterr()
    q, st = m.predict_tests_foveated(tests, ref, frames_per_second=FPS, fixation_point=gaze)
    err = capfd.readouterr().err
    _same(q, st, jod, Q, shared=False)
    assert "multitest_fov_kernel<" not in err and "band_kernel<4, false, 2>" in err
    assert st["N_frames"] == 4 and st["width"] == 240 and st["height"] == 135 and st["frames_per_second"] == FPS


def test_argument_checks_that_need_a_context():
    lib, dev = nat.lib(), torch.device("cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    W, H, n, T = 121, 68, 3, 3
    m = fv.fvvdp(display_name="standard_4k", foveated=True)
    n_bands, rho = m._band_count(W, H)
    nbytes = ctypes.c_size_t()
    nat.check(lib.fvvdp_tests_workspace(W, H, n_bands, T, n, ctypes.byref(nbytes)))
    work = torch.zeros(nbytes.value // 4 + 64, device=dev)
    Q = torch.zeros((T, n_bands, 2, n), device=dev)
    qp, wp = ctypes.c_void_p(Q.data_ptr()), ctypes.c_void_p(work.data_ptr())
    fix = np.float32([[10, 20], [30, 40], [500, -500]])
    geom = m._geom_struct()
    gp = ctypes.byref(geom)

    def call(ctx, n_=n, T_=T, q=qp, w=wp, wb=nbytes.value, col0=0, f=nat.fptr(fix), g=gp):
        return lib.fvvdp_bands_forward_tests_fov(ctx.handle, n_, T_, q, n, col0, f, g, w, wb, stream), lib.fvvdp_last_error().decode()

    ctx = m._context(W, H, n_bands, 4, 2 * n, rho)                     # 2 quads of 3 frames: T <= 3
    covered = ctypes.c_int(-1)
    nat.check(lib.fvvdp_tests_fov_covered(ctx.handle, gp, ctypes.byref(covered), stream))
    assert covered.value == 1
    assert call(ctx)[0] == 0
    for kw, word in ((dict(T_=0), "n_tests"), (dict(n_=0), "n must"), (dict(T_=4), "frame slots"), (dict(q=None), "null"),
                     (dict(w=None), "null"), (dict(f=None), "null"), (dict(g=None), "geometry"),
                     (dict(w=ctypes.c_void_p(work.data_ptr() + 64)), "aligned"),
                     (dict(wb=nbytes.value - 4), "too small"), (dict(col0=1), "columns")):
        rc, msg = call(ctx, **kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    still = m._context(W, H, n_bands, 2, 2 * n, rho)                   # replaces the video context
    rc, msg = call(still)
    assert rc == -1 and "still-image" in msg
    assert lib.fvvdp_tests_fov_covered(still.handle, gp, ctypes.byref(covered), stream) == -1
    plain = fv.fvvdp(display_name="standard_4k")
    pctx = plain._context(W, H, n_bands, 4, 2 * n, rho)
    rc, msg = call(pctx)
    assert rc == -1 and "not foveated" in msg
    assert lib.fvvdp_tests_fov_covered(pctx.handle, gp, ctypes.byref(covered), stream) == -1
    # a display whose slices do not fit the LDS: the query says so and the pass refuses with the code for "use the general call"
    hmd = fv.fvvdp(display_name="standard_hmd", foveated=True)
    nb_h, rho_h = hmd._band_count(W, H)
    hctx = hmd._context(W, H, nb_h, 4, 2 * n, rho_h)
    hgeom = hmd._geom_struct()
    nat.check(lib.fvvdp_tests_fov_covered(hctx.handle, ctypes.byref(hgeom), ctypes.byref(covered), stream))
    assert covered.value == 0
    nat.check(lib.fvvdp_tests_workspace(W, H, nb_h, T, n, ctypes.byref(nbytes)))
    work_h = torch.zeros(nbytes.value // 4, device=dev)
    Q_h = torch.zeros((T, nb_h, 2, n), device=dev)
    rc, msg = call(hctx, q=ctypes.c_void_p(Q_h.data_ptr()), w=ctypes.c_void_p(work_h.data_ptr()), wb=nbytes.value, g=ctypes.byref(hgeom))
    assert rc == nat.FVVDP_EUNSUPPORTED and "LDS" in msg
    torch.cuda.synchronize()
    assert float(Q_h.abs().max()) == 0.0                               # refused before the first launch
