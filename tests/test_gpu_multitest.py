"""fvvdp.predict_tests on the GPU.  The yardstick is the existing path, never the new one:

    loop[k] = predict(tests[k], reference)          on the same metric object

and the contract is bit identity: every comparison below is torch.equal / np.array_equal, on Q_JOD and on Q_per_ch."""
import ctypes
import logging

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd.synth import synth_video_pair

pytestmark = pytest.mark.gpu

FPS = 30
# 250x131: three strips at level 0 (coarse width 125 > 122), odd heights at several levels (131, 33, 17, 9, 5: the row-parity
# quirk of the reduce), 32750 pixels = no multiple of the temporal kernels' vector width (their per-pixel fallback runs)
H0, W0 = 131, 250


def _degrade(t, r, k):
    """Test k of a uint8 pair [1, C, N, H, W]: the generator's noisy test, a blur, the clip one frame late, the reference itself,
    then seeded noise of growing amplitude."""
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


def _loop(m, tests, ref, fps=FPS):
    jod, Q = [], []
    for t in tests:
        q, st = m.predict(t, ref, frames_per_second=fps)
        jod.append(q.clone())
        Q.append(st["Q_per_ch"].copy())
    return torch.stack(jod), np.stack(Q)


def _same(q, st, jod, Q):
    assert q.dtype is torch.float32 and q.is_cuda and tuple(q.shape) == (len(jod),)
    assert st["Q_per_ch"].shape == Q.shape and st["Q_per_ch"].dtype == np.float32
    print("max |dQ| %.3g, max |dJOD| %.3g" % (float(np.abs(st["Q_per_ch"] - Q).max()), float((q - jod).abs().max())))
    assert np.array_equal(st["Q_per_ch"], Q)
    assert torch.equal(q, jod)


_base = {}


def _base_case():
    """(metric, 8 tests, reference, the loop of predict calls) of the 250x131 x 5 uint8 RGB case -- made once, never changed."""
    if not _base:
        tests, ref = _clips(5, H0, W0, 8)
        m = fv.fvvdp(display_name="standard_4k")
        _base["v"] = (m, tests, ref) + _loop(m, tests, ref)
    return _base["v"]


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 8])
def test_rows_equal_predict(T):
    """Odd T: the last test shares the reference's quad; even T: the reference stands alone in its quad; T = 8: two launch groups."""
    m, tests, ref, jod, Q = _base_case()
    q, st = m.predict_tests(tests[:T], ref, frames_per_second=FPS)
    _same(q, st, jod[:T], Q[:T])
    assert st["N_frames"] == 5 and st["width"] == W0 and st["height"] == H0 and st["frames_per_second"] == FPS
    assert len(st["rho_band"]) == Q.shape[1] + 1


def test_groups_of_two_quads_give_the_same_bits(monkeypatch):
    """FVVDP_TESTS_GROUP=2: every launch reads the reference's quad and one other (multitest_kernel<2, .>), four groups at T = 8."""
    _, tests, ref, jod, Q = _base_case()
    monkeypatch.setenv("FVVDP_TESTS_GROUP", "2")
    m = fv.fvvdp(display_name="standard_4k")
    for T in (7, 8):
        q, st = m.predict_tests(tests[:T], ref, frames_per_second=FPS)
        _same(q, st, jod[:T], Q[:T])


@pytest.mark.parametrize("T,cap", [(1, 3), (2, 3), (5, 3), (8, 3), (7, 2)])
def test_launched_groups_are_the_host_plan(T, cap, monkeypatch, capfd):
    """The groups the library launches (its FVVDP_DEBUG_VARIANT lines) are multitest.quad_plan's, level by level."""
    import re
    from fovvideovdp_amd.multitest import quad_plan
    _, tests, ref, jod, Q = _base_case()
    monkeypatch.setenv("FVVDP_DEBUG_VARIANT", "1")
    monkeypatch.setenv("FVVDP_TESTS_GROUP", str(cap))
    m = fv.fvvdp(display_name="standard_4k")
    capfd.readouterr()
    q, st = m.predict_tests(tests[:T], ref, frames_per_second=FPS)
    err = capfd.readouterr().err
    _same(q, st, jod[:T], Q[:T])
    got = re.findall(r"level (\d+): multitest_kernel<(\d+), (true|false)>, n (\d+), quads (\d+)\.\., .*store_ref (\d)", err)
    qp = quad_plan(T, 5, cap)
    want = [(str(b), str(len(g["quads"])), "true" if (T - 1) in g["tests"] and T % 2 else "false", "5",
             str(g["quads"][1] if len(g["quads"]) > 1 else 0), "1" if qp.ref_quad in g["store"] else "0")
            for b in range(Q.shape[1]) for g in qp.groups]
    assert got == want


def test_one_level_pass_equals_the_two_level_path():
    """1024x520: levels 0 and 1 hold >= 0.5 Mpixel, predict takes band2_kernel for them and the vector temporal kernels.  The
    pass walks the two levels one by one in band2_kernel's strips, chunks and lane order (multitest_kernel.hpp): level 0 with
    54 owned lanes per strip, level 1 with one sum per column and the two-parity lane tree."""
    tests, ref = _clips(3, 520, 1024, 3)
    m = fv.fvvdp(display_name="standard_4k")
    jod, Q = _loop(m, tests, ref)
    q, st = m.predict_tests(tests, ref, frames_per_second=FPS)
    _same(q, st, jod, Q)


def test_one_level_pass_equals_the_one_level_path_at_that_size(monkeypatch):
    """The same clips with predict held to one level per launch (FVVDP_BAND_FUSE=0, read when the context is made): the pass
    follows the switch and its rows are that predict's bit for bit.  The two predicts differ from each other (the grouping of
    the fp32 partial sums: printed), which is why the pass has to follow."""
    tests, ref = _clips(3, 520, 1024, 3)
    monkeypatch.setenv("FVVDP_BAND_FUSE", "0")
    m = fv.fvvdp(display_name="standard_4k")
    jod, Q = _loop(m, tests, ref)
    q, st = m.predict_tests(tests, ref, frames_per_second=FPS)
    _same(q, st, jod, Q)
    monkeypatch.delenv("FVVDP_BAND_FUSE")
    two = fv.fvvdp(display_name="standard_4k")
    jod2, Q2 = _loop(two, tests, ref)
    ne = Q2 != Q
    print("two-level against one-level predict: %d of %d Q entries differ, bands %s, max relative %.3g" % (
        int(ne.sum()), Q.size, sorted(set(np.nonzero(ne)[1].tolist())), float((np.abs(Q2 - Q) / np.maximum(np.abs(Q), 1e-30)).max())))
    assert not ne[:, 2:].any()                                         # the levels both paths walk with the one-level kernel


def test_batches_shorter_than_the_clip():
    """batch_frames = 2 on 5 frames: three batches, the last one short; quad q of a batch of n frames lies in slots [q n, q n + n)."""
    _, tests, ref, _, _ = _base_case()
    m = fv.fvvdp(display_name="standard_4k", batch_frames=2)
    jod, Q = _loop(m, tests[:5], ref)
    for T in (4, 5):
        q, st = m.predict_tests(tests[:T], ref, frames_per_second=FPS)
        _same(q, st, jod[:T], Q[:T])


def test_several_passes_when_the_scratch_budget_is_short():
    """A budget of two quads: five tests go in two passes (three tests, then two), each with the reference; one quad: one test
    per pass.  The batch stays predict's, so the rows keep their bits."""
    m, tests, ref, jod, Q = _base_case()
    per_frame = W0 * H0 * 4 * 4 * 1.34
    try:
        for quads in (2, 1):
            m.tests_scratch_bytes = quads * 5 * per_frame + 1
            q, st = m.predict_tests(tests[:5], ref, frames_per_second=FPS)
            _same(q, st, jod[:5], Q[:5])
    finally:
        m.tests_scratch_bytes = None


@pytest.mark.parametrize("dtype,gray", [("float32", False), ("uint16", False), ("float16", False), ("bfloat16", False), ("uint8", True),
                                        ("float32", True)])
def test_sample_types_and_channels(dtype, gray):
    tests, ref = _clips(4, H0, W0, 3, dtype, gray)
    m = fv.fvvdp(display_name="standard_4k")
    jod, Q = _loop(m, tests, ref)
    q, st = m.predict_tests(tests, ref, frames_per_second=FPS)
    _same(q, st, jod, Q)


def test_a_display_whose_clamps_can_bind():
    tests, ref = _clips(4, H0, W0, 2, "float32")
    m = fv.fvvdp(display_name="standard_hdr_pq")
    jod, Q = _loop(m, tests, ref)
    q, st = m.predict_tests(tests, ref, frames_per_second=FPS)
    _same(q, st, jod, Q)


@pytest.mark.parametrize("padding", ["replicate", "circular", "pingpong"])
def test_temporal_padding(padding):
    _, tests, ref, _, _ = _base_case()
    m = fv.fvvdp(display_name="standard_4k", temp_padding=padding)
    jod, Q = _loop(m, tests[:2], ref)
    q, st = m.predict_tests(tests[:2], ref, frames_per_second=FPS)
    _same(q, st, jod, Q)


def test_sixteen_taps():
    tests, ref = _clips(6, H0, W0, 3)
    m = fv.fvvdp(display_name="standard_4k")
    jod, Q = _loop(m, tests, ref, fps=60)
    assert 9 <= m.filter_len <= 16                                     # the 16-slot ring of the temporal kernels
    q, st = m.predict_tests(tests, ref, frames_per_second=60)
    _same(q, st, jod, Q)


def test_dim_order_and_host_arrays():
    _, tests, ref, jod, Q = _base_case()
    m = fv.fvvdp(display_name="standard_4k")
    tt = [t[0].permute(1, 2, 3, 0).cpu().numpy() for t in tests[:3]]             # FHWC on the host
    q, st = m.predict_tests(tuple(tt), ref[0].permute(1, 2, 3, 0).cpu().numpy(), dim_order="FHWC", frames_per_second=FPS)
    _same(q, st, jod[:3], Q[:3])


def test_a_row_does_not_depend_on_the_other_tests():
    m, tests, ref, jod, Q = _base_case()
    order = [2, 0, 3, 1]
    q, st = m.predict_tests([tests[k] for k in order], ref, frames_per_second=FPS)
    _same(q, st, jod[order], Q[order])
    q, st = m.predict_tests([tests[5], tests[6], tests[2], tests[7]], ref, frames_per_second=FPS)          # the others replaced
    assert torch.equal(q[2], jod[2]) and np.array_equal(st["Q_per_ch"][2], Q[2])


def test_a_test_identical_to_the_reference():
    m, tests, ref, jod, Q = _base_case()
    assert torch.equal(tests[3], ref)
    for group in ([tests[3]], [tests[0], tests[3]], [tests[0], tests[1], tests[3]]):      # beside the reference, and in another quad
        q, st = m.predict_tests(group, ref, frames_per_second=FPS)
        assert torch.equal(q[-1], jod[3]) and np.array_equal(st["Q_per_ch"][-1], Q[3])


def _call_stats(m):
    out = (ctypes.c_int64 * 3)()
    nat.check(nat.lib().fvvdp_ctx_call_stats(m._ctx.handle, out))
    return [int(v) for v in out]


def test_second_call_neither_allocates_nor_synchronises_in_the_library(monkeypatch):
    _, tests, ref, jod, Q = _base_case()
    m = fv.fvvdp(display_name="standard_4k", batch_frames=3)
    m.predict_tests(tests[:5], ref, frames_per_second=FPS)             # warm-up: the context
    s0 = _call_stats(m)
    syncs = []
    real = torch.cuda.Stream.synchronize
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (syncs.append(1), real(self))[1])
    q, st = m.predict_tests(tests[:5], ref, frames_per_second=FPS)
    assert _call_stats(m) == s0                                        # syncs, allocations, frees inside the library: none added
    assert len(syncs) == 1                                             # the one result copy
    assert tuple(q.shape) == (5,)


def test_out_of_range_warning_once(caplog):
    tests, ref = _clips(4, H0, W0, 3, "float32")
    tests = [t.clone() for t in tests]
    tests[1][0, 1, 2, 7, 9] = 1.5
    m = fv.fvvdp(display_name="standard_4k")
    with caplog.at_level(logging.WARNING):
        m.predict_tests(tests, ref, frames_per_second=FPS)
    assert sum("outside the valid range" in rec.getMessage() for rec in caplog.records) == 1
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        m.predict_tests([tests[0], tests[2]], ref, frames_per_second=FPS)
    assert not any("outside the valid range" in rec.getMessage() for rec in caplog.records)


def test_argument_checks_that_need_a_context():
    lib, dev = nat.lib(), torch.device("cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    W, H, n, T = 121, 68, 3, 3
    m = fv.fvvdp(display_name="standard_4k")
    n_bands, rho = m._band_count(W, H)
    nbytes = ctypes.c_size_t()
    nat.check(lib.fvvdp_tests_workspace(W, H, n_bands, T, n, ctypes.byref(nbytes)))
    work = torch.zeros(nbytes.value // 4 + 64, device=dev)
    Q = torch.zeros((T, n_bands, 2, n), device=dev)
    qp, wp = ctypes.c_void_p(Q.data_ptr()), ctypes.c_void_p(work.data_ptr())

    def call(ctx, n_=n, T_=T, q=qp, w=wp, wb=nbytes.value, col0=0):
        return lib.fvvdp_bands_forward_tests(ctx.handle, n_, T_, q, n, col0, w, wb, stream), lib.fvvdp_last_error().decode()

    ctx = m._context(W, H, n_bands, 4, 2 * n, rho)                     # 2 quads of 3 frames: T <= 3
    assert call(ctx)[0] == 0
    for kw, word in ((dict(T_=0), "n_tests"), (dict(n_=0), "n must"), (dict(T_=4), "frame slots"), (dict(q=None), "null"),
                     (dict(w=None), "null"), (dict(w=ctypes.c_void_p(work.data_ptr() + 64)), "aligned"),
                     (dict(wb=nbytes.value - 4), "too small"), (dict(col0=1), "columns")):
        rc, msg = call(ctx, **kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    still = m._context(W, H, n_bands, 2, 2 * n, rho)                   # replaces the video context
    rc, msg = call(still)
    assert rc == -1 and "still-image" in msg
    fov = fv.fvvdp(display_name="standard_4k", foveated=True)
    rc, msg = call(fov._context(W, H, n_bands, 4, 2 * n, rho))
    assert rc == -1 and "foveated" in msg
    torch.cuda.synchronize()
