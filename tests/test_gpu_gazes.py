"""fvvdp.predict_gazes on the GPU.  The yardstick is the existing path, never the new one:

    ref_loop[g] = predict(test, ref, fixation_point=fp[g])

(itself pinned to the reference by g4_foveated_135x240, tests/test_gpu_parity.py), and the contract is bit identity: every
comparison below is torch.equal / np.array_equal."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fovvideovdp_amd as fv
from fovvideovdp_amd import _native as nat
from fovvideovdp_amd.synth import synth_gaze, synth_video_pair

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NG = nat.GAZE_GROUP_MAX
COUNTS = (1, NG - 1, NG, NG + 1, 2 * NG + 1)
N = 5
FPS = 30

# standard_hmd: a 110 degree field of view, every band's slice of the CSF table spans 8-9 rho intervals and does not fit the LDS --
# those bands take the single-gaze kernel once per gaze (only the temporal channels are shared), as predict() does per call.
# (H, W) of the clips.  68x121 and 135x240 are odd sizes (both reduce parities; 135x240 has two strips at level 0: wc = 120 > 62).
# 5x9 is the smallest size whose level 0 is walked in two chunks: chunking() never picks a chunk of fewer than 2 coarse rows and,
# while one round of resident waves covers the launch, takes exactly 2 -- so level 0 has ceil(hc / 2) chunks and hc = 3, i.e.
# H = 5, is the first height with two (a frame needs min(H, W) >= 4 for one band-pass level).
SIZES = {"gray68x121": (68, 121), "rgb135x240": (135, 240), "gray5x9": (5, 9)}


def _clip(name):
    H, W = SIZES[name]
    t, r = synth_video_pair(N, H, W, pair=7)
    if name.startswith("gray"):           # float32 gray in [0, 1]
        t = (t.to(torch.float32).mean(dim=1, keepdim=True) / 255).contiguous()
        r = (r.to(torch.float32).mean(dim=1, keepdim=True) / 255).contiguous()
    return t.cuda(), r.cuda()


def _gazes(H, W, kind):
    """2 NG + 1 gazes: the frame corners, 500 pixels outside the frame on either side (the eccentricity clamp), the centre, then
    seeded points.  fixed: [G, 2]; moving: [G, N, 2], gaze g drifting from point g to point g + 5."""
    rng = np.random.RandomState(11)
    pts = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W + 499, H + 499), (-500, -500), (W // 2, H // 2)]
    while len(pts) < 2 * NG + 1:
        pts.append((float(rng.uniform(0, W - 1)), float(rng.uniform(0, H - 1))))
    fixed = np.asarray(pts, np.float32)
    if kind == "fixed":
        return fixed
    w = np.linspace(0.0, 1.0, N, dtype=np.float32)[None, :, None]
    return np.ascontiguousarray(fixed[:, None, :] * (1 - w) + np.roll(fixed, -5, axis=0)[:, None, :] * w)


_cache = {}


def _case(clip, display, kind):
    """(metric, test, ref, gazes, the loop of predict calls: JOD [G] and Q_per_ch [G, bands, 2, N]) -- made once, never changed."""
    key = (clip, display, kind)
    if key not in _cache:
        t, r = _clip(clip)
        H, W = SIZES[clip]
        fp = _gazes(H, W, kind)
        m = fv.fvvdp(display_name=display, foveated=True)
        jod, Q = [], []
        for g in range(len(fp)):
            q, st = m.predict(t, r, frames_per_second=FPS, fixation_point=fp[g])
            jod.append(q.clone())
            Q.append(st["Q_per_ch"].copy())
        _cache[key] = (m, t, r, fp, torch.stack(jod), np.stack(Q))
    return _cache[key]


def _same(q, st, jod, Q):
    assert q.dtype is torch.float32 and q.is_cuda and tuple(q.shape) == (len(jod),)
    assert st["Q_per_ch"].shape == Q.shape and st["Q_per_ch"].dtype == np.float32
    assert np.array_equal(st["Q_per_ch"], Q)
    assert torch.equal(q, jod)


@pytest.mark.parametrize("kind", ["fixed", "moving"])
@pytest.mark.parametrize("clip,display", [("gray68x121", "standard_4k"), ("rgb135x240", "standard_4k"), ("gray5x9", "standard_4k"),
                                          ("gray68x121", "standard_hdr_pq"), ("rgb135x240", "standard_hmd")])
def test_bit_identical_to_the_loop_of_predict_calls(clip, display, kind):
    m, t, r, fp, jod, Q = _case(clip, display, kind)
    assert len(set(float(v) for v in jod)) >= 2                     # the gazes do matter
    for G in COUNTS:
        q, st = m.predict_gazes(t, r, fp[:G], frames_per_second=FPS)
        _same(q, st, jod[:G], Q[:G])
        assert st["N_frames"] == N and st["width"] == SIZES[clip][1] and st["height"] == SIZES[clip][0]
        assert st["frames_per_second"] == FPS and len(st["rho_band"]) == Q.shape[1] + 1


@pytest.mark.parametrize("cap", [1, 2, 4])
def test_the_group_size_does_not_matter(cap, monkeypatch):
    """FVVDP_GAZE_GROUP (read when a context is created) caps the gazes per launch: smaller groups, more launches over the same
    levels of which only the first stores the next level -- same bits."""
    _, t, r, fp, jod, Q = _case("rgb135x240", "standard_4k", "moving")
    monkeypatch.setenv("FVVDP_GAZE_GROUP", str(cap))
    m = fv.fvvdp(display_name="standard_4k", foveated=True)
    q, st = m.predict_gazes(t, r, fp[:NG + 1], frames_per_second=FPS)
    _same(q, st, jod[:NG + 1], Q[:NG + 1])


def test_golden_gaze_among_others():
    """g4_foveated_135x240 (the reference's own run): its moving gaze as one of three, within the tolerances
    tests/test_gpu_parity.py::test_foveated_pq_golden uses for this golden."""
    z = np.load(os.path.join(GOLDEN, "g4_foveated_135x240.npz"))
    n, H, W = 6, 135, 240
    test, ref = synth_video_pair(n, H, W)
    gaze = synth_gaze(n, H, W).numpy()
    fp = np.stack([np.tile(np.float32([[3, 130]]), (n, 1)), gaze, gaze[::-1]])
    m = fv.fvvdp(display_name="standard_hdr_pq", foveated=True)
    q, st = m.predict_gazes(test, ref, fp, frames_per_second=30)
    assert abs(float(q[1]) - float(z["jod"])) < 1e-4
    qq, gq = st["Q_per_ch"][1].astype(np.float64), z["Q_per_ch"].astype(np.float64)
    assert np.all(np.abs(qq - gq) <= 3e-3 * np.abs(gq) + 1e-6 * np.max(gq))
    q1, st1 = m.predict(test, ref, frames_per_second=30, fixation_point=gaze)
    assert torch.equal(q[1], q1) and np.array_equal(st["Q_per_ch"][1], st1["Q_per_ch"])
    assert float(q[0]) != float(q[1]) != float(q[2])


def test_gazes_are_independent():
    m, t, r, fp, jod, Q = _case("rgb135x240", "standard_4k", "fixed")
    G = NG + 3
    perm = np.random.RandomState(5).permutation(G)
    q, st = m.predict_gazes(t, r, fp[:G][perm], frames_per_second=FPS)
    _same(q, st, jod[:G][torch.as_tensor(perm, device=jod.device)], Q[:G][perm])
    twice = np.stack([fp[3], fp[8], fp[3], fp[3]])
    q, st = m.predict_gazes(t, r, twice, frames_per_second=FPS)
    assert torch.equal(q[0], q[2]) and torch.equal(q[0], q[3]) and np.array_equal(st["Q_per_ch"][0], st["Q_per_ch"][2])
    _same(q, st, jod[[3, 8, 3, 3]], Q[[3, 8, 3, 3]])
    # a torch tensor of gazes is taken as well
    q, st = m.predict_gazes(t, r, torch.from_numpy(fp[:2]), frames_per_second=FPS)
    _same(q, st, jod[:2], Q[:2])


def test_batches_shorter_than_the_clip():
    _, t, r, fp, jod, Q = _case("rgb135x240", "standard_4k", "moving")
    m = fv.fvvdp(display_name="standard_4k", foveated=True, batch_frames=2)
    G = NG + 1
    q, st = m.predict_gazes(t, r, fp[:G], frames_per_second=FPS)
    _same(q, st, jod[:G], Q[:G])                       # the single-batch result ...
    q1, st1 = m.predict(t, r, frames_per_second=FPS, fixation_point=fp[2])
    assert torch.equal(q[2], q1) and np.array_equal(st["Q_per_ch"][2], st1["Q_per_ch"])     # ... and predict in the same batches


@pytest.mark.parametrize("C", [1, 3])
def test_single_frame(C):
    H, W = 68, 121
    t, r = synth_video_pair(1, H, W, C=C, pair=3)
    t, r = t.cuda(), r.cuda()
    fp = _gazes(H, W, "fixed")[:NG + 1]
    m = fv.fvvdp(display_name="standard_4k", foveated=True)
    q, st = m.predict_gazes(t, r, fp)
    assert st["Q_per_ch"].shape[0] == NG + 1 and st["Q_per_ch"].shape[2:] == (2, 1) and st["N_frames"] == 1
    for g in range(NG + 1):
        q1, st1 = m.predict(t, r, fixation_point=fp[g])
        assert torch.equal(q[g], q1) and np.array_equal(st["Q_per_ch"][g], st1["Q_per_ch"])


def test_uint16_source():
    H, W = SIZES["gray68x121"]
    t, r = synth_video_pair(N, H, W, C=1, pair=2)
    t16, r16 = (t.numpy().astype(np.uint16) * 257), (r.numpy().astype(np.uint16) * 257)
    fp = _gazes(H, W, "fixed")[:3]
    m = fv.fvvdp(display_name="standard_4k", foveated=True)
    q, st = m.predict_gazes(t16, r16, fp, frames_per_second=FPS)
    for g in range(3):
        q1, st1 = m.predict(t16, r16, frames_per_second=FPS, fixation_point=fp[g])
        assert torch.equal(q[g], q1) and np.array_equal(st["Q_per_ch"][g], st1["Q_per_ch"])


def test_identical_pair_and_determinism():
    m, t, r, fp, jod, Q = _case("rgb135x240", "standard_4k", "moving")
    q, st = m.predict_gazes(r, r, fp, frames_per_second=FPS)
    assert torch.all(q == 10.0) and np.all(st["Q_per_ch"] == 0)
    a = m.predict_gazes(t, r, fp, frames_per_second=FPS)
    b = m.predict_gazes(t, r, fp, frames_per_second=FPS)
    assert torch.equal(a[0], b[0]) and np.array_equal(a[1]["Q_per_ch"], b[1]["Q_per_ch"])
    _same(a[0], a[1], jod, Q)


def test_no_residue():
    m, t, r, fp, jod, Q = _case("gray68x121", "standard_hdr_pq", "moving")
    a = fp[4]
    before = m.predict(t, r, frames_per_second=FPS, fixation_point=a)
    q, st = m.predict_gazes(t, r, fp[:NG + 1], frames_per_second=FPS)
    plain = fv.fvvdp(display_name="standard_hdr_pq")                    # not foveated, same frame size, between the calls
    p0 = plain.predict(t, r, frames_per_second=FPS)
    after = m.predict(t, r, frames_per_second=FPS, fixation_point=a)
    assert torch.equal(before[0], after[0]) and np.array_equal(before[1]["Q_per_ch"], after[1]["Q_per_ch"])
    assert torch.equal(before[0], jod[4])
    q2, st2 = m.predict_gazes(t, r, fp[:NG + 1], frames_per_second=FPS)
    p1 = plain.predict(t, r, frames_per_second=FPS)
    assert torch.equal(q, q2) and np.array_equal(st["Q_per_ch"], st2["Q_per_ch"])
    assert torch.equal(p0[0], p1[0]) and np.array_equal(p0[1]["Q_per_ch"], p1[1]["Q_per_ch"])


def _call_stats(m):
    out = (ctypes.c_int64 * 3)()
    nat.check(nat.lib().fvvdp_ctx_call_stats(m._ctx.handle, out))
    return [int(v) for v in out]


def test_second_call_neither_allocates_nor_synchronises_in_the_library(monkeypatch):
    _, t, r, fp, jod, Q = _case("rgb135x240", "standard_4k", "moving")
    m = fv.fvvdp(display_name="standard_4k", foveated=True)
    m.predict_gazes(t, r, fp, frames_per_second=FPS)                   # warm-up: context, foveated tables
    s0 = _call_stats(m)
    syncs = []
    real = torch.cuda.Stream.synchronize
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (syncs.append(1), real(self))[1])
    q, st = m.predict_gazes(t, r, fp, frames_per_second=FPS)
    assert _call_stats(m) == s0                                        # syncs, allocations, frees inside the library: none added
    assert len(syncs) == 1                                             # the one result copy
    _same(q, st, jod, Q)


def test_argument_checks_that_need_a_context():
    H, W = SIZES["gray68x121"]
    lib = nat.lib()
    dev = torch.device("cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    G = 3
    gaze = torch.zeros((G, N, 2), device=dev)
    nbytes = ctypes.c_size_t()

    def call(m, foveated_ctx, work_off=0, work_bytes=None, stride=2 * N, n=N):
        n_bands, rho = m._band_count(W, H)
        ctx = m._context(W, H, n_bands, 4, N, rho)
        nat.check(lib.fvvdp_gaze_workspace(W, H, n_bands, G, N, ctypes.byref(nbytes)))
        work = torch.empty(nbytes.value // 4 + 64, dtype=torch.float32, device=dev)
        Q = torch.zeros((G, n_bands, 2, N), device=dev)
        g = m._geom_struct()
        rc = lib.fvvdp_bands_forward_gazes(ctx.handle, n, G, ctypes.c_void_p(gaze.data_ptr()), stride, ctypes.c_void_p(Q.data_ptr()),
                                           N, 0, ctypes.byref(g), ctypes.c_void_p(work.data_ptr() + work_off),
                                           nbytes.value if work_bytes is None else work_bytes, stream)
        return rc, lib.fvvdp_last_error(), ctx

    m0 = fv.fvvdp(display_name="standard_4k", foveated=True)
    nb0, rho0 = m0._band_count(W, H)
    c0 = m0._context(W, H, nb0, 4, N, rho0)
    g0 = m0._geom_struct()
    nat.check(lib.fvvdp_gaze_workspace(W, H, nb0, G, N, ctypes.byref(nbytes)))
    w0 = torch.empty(nbytes.value // 4, dtype=torch.float32, device=dev)
    Q0 = torch.zeros((G, nb0, 2, N), device=dev)
    good = [c0.handle, N, G, ctypes.c_void_p(gaze.data_ptr()), 2 * N, ctypes.c_void_p(Q0.data_ptr()), N, 0, ctypes.byref(g0),
            ctypes.c_void_p(w0.data_ptr()), nbytes.value, stream]
    for k in (3, 5, 8, 9):                                   # gazes, Q, geometry, workspace: null
        args = list(good)
        args[k] = None
        assert lib.fvvdp_bands_forward_gazes(*args) == -1 and b"null" in lib.fvvdp_last_error()
    for bad_G in (0, -3):
        args = list(good)
        args[2] = bad_G
        assert lib.fvvdp_bands_forward_gazes(*args) == -1 and b"n_gazes" in lib.fvvdp_last_error()
    pp = nat.PoolParams(1, 0.67, 1, 0.25, -0.016, 0.6)
    jod0 = torch.zeros(G, device=dev)
    assert lib.fvvdp_bands_forward_gazes_pool(*good[:11], None, ctypes.c_void_p(jod0.data_ptr()), stream) == -1
    assert b"null" in lib.fvvdp_last_error()
    assert lib.fvvdp_bands_forward_gazes_pool(*good[:11], ctypes.byref(pp), None, stream) == -1 and b"null" in lib.fvvdp_last_error()
    bad = nat.PoolParams(1, 0.67, 0, 0.25, -0.016, 0.6)
    assert lib.fvvdp_bands_forward_gazes_pool(*good[:11], ctypes.byref(bad), ctypes.c_void_p(jod0.data_ptr()), stream) == -1
    assert b"exponents" in lib.fvvdp_last_error()
    plain = fv.fvvdp(display_name="standard_4k")
    rc, msg, _ = call(plain, False)
    assert rc == -1 and b"not foveated" in msg
    m = fv.fvvdp(display_name="standard_4k", foveated=True)
    rc, msg, _ = call(m, True, work_off=4)
    assert rc == -1 and b"aligned" in msg
    rc, msg, _ = call(m, True, work_bytes=nbytes.value - 4)
    assert rc == -1 and b"too small" in msg
    rc, msg, _ = call(m, True, stride=2 * N - 1)
    assert rc == -1 and b"gaze_stride" in msg
    rc, msg, _ = call(m, True, n=N + 1)
    assert rc == -1 and b"max_frames" in msg
    rc, msg, ctx = call(m, True, n=0)
    assert rc == -1
    keep = []
    for b, (w_b, h_b) in enumerate(m._level_sizes(W, H, ctx.key[2])[:ctx.key[2]]):       # map mode needs the maps of every band
        maps = [torch.ones((h_b, w_b), device=dev) for _ in range(3)]
        keep.append(maps)
        nat.check(lib.fvvdp_ctx_set_view_maps(ctx.handle, b, *[ctypes.c_void_p(x.data_ptr()) for x in maps], 1.0, 1.5))
    rc, msg, _ = call(m, True)
    assert rc == -1 and b"view maps" in msg
    torch.cuda.synchronize()
    m._drop_context()
