"""GPU: the two-levels-per-pass pyramid kernel (band2_kernel) checked one pixel at a time, at the production sizes and plans.

Pooled Q alone cannot say which pixel is wrong: a wrong tap in one strip-seam column of a 4K frame touches ~2000 of 8.3 M
pixels and disappears in the L_p pooling.  Two kinds of check here:

a. The Gaussian level that band2 writes (level C = level b+2, the input of the next pass) against a float64 reduce of the
   exported level 0 (oracle `gausspyr_reduce(..., dtype=np.float64)`), every pixel, at full size, through the low-level
   pipeline and through a 128-slot `predict_images` context; bit-identical whatever the launch shape (waves per workgroup,
   tickets, chunk heights).
b. Impulse probes: a test image equal to the reference except at one pixel (or one 2x2 block).  Every band's D is exactly 0
   outside the probe's footprint, so Q of each band pools the footprint only and an error there moves Q by O(1).  Probes sit
   at the corners, the edges, every strip seam of both passes (108 level-0 columns per strip of pass 0+1, 432 of pass 2+3),
   and around every chunk seam, read from the launched plan (FVVDP_DEBUG_VARIANT).

The launched plan comes from the FVVDP_DEBUG_VARIANT line of every band2 launch (fvvdp_hip.hip, bands_forward_core)."""
import re

import numpy as np
import pytest
import torch

from oracle import fvvdp_oracle as orc

pytestmark = pytest.mark.gpu

F64 = np.float64
PLAN_RE = re.compile(r"levels (\d+)\+(\d+): band2_kernel<(\d), (true|false)>.*?(\d+) waves per workgroup, n_strips (\d+), kr (\d+), "
                     r"kr2 (\d+), n_big (\d+), n_chunks (\d+), tickets (on|off)")
KNOBS = ("FVVDP_BAND_FUSE", "FVVDP_BAND2_KR", "FVVDP_BAND2_KR2", "FVVDP_BAND2_WPB", "FVVDP_BAND2_TICKET", "FVVDP_BAND_INRANGE")


def _env(monkeypatch, **kw):
    """Launch knobs (read when a native context is created): everything not named goes back to the library's default."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv("FVVDP_" + k, str(v))
    monkeypatch.setenv("FVVDP_DEBUG_VARIANT", "1")


def _plans(err):
    """band2 launches in a captured stderr: [{b, P, inrange, wpb, n_strips, kr, kr2, n_big, n_chunks, tickets}]."""
    out = []
    for m in PLAN_RE.finditer(err):
        g = m.groups()
        out.append(dict(b=int(g[0]), P=int(g[2]), inrange=g[3] == "true", wpb=int(g[4]), n_strips=int(g[5]), kr=int(g[6]),
                        kr2=int(g[7]), n_big=int(g[8]), n_chunks=int(g[9]), tickets=g[10] == "on"))
    return out


def _reduce64(x, times):
    """float64 Gaussian reduce (the reference's gausspyr_reduce, row-parity quirk included), `times` times; x [P,H,W]."""
    y = np.asarray(x, F64)
    for _ in range(times):
        y = orc.gausspyr_reduce(y, F64)
    return y


def _level_err(gpu, ref64):
    """Worst per-pixel relative error of one exported level (all planes are positive luminances here)."""
    assert gpu.shape == ref64.shape, (gpu.shape, ref64.shape)
    return float(np.max(np.abs(gpu.astype(F64) - ref64) / np.abs(ref64)))


# measured on MI355X: worst per-pixel error of level C (band2 output) against the float64 reduce of level 0 is 3.0e-7
# relative at 1080p / 1440p / 4K and 3.1e-7 for level 4 of 8K (fp32 rounding of positive-weight 5-tap sums)
LEVEL_TOL = 9e-7


def _planar(n, P, H, W, seed):
    """Random positive planar luminance [n,P,H,W]: every pixel independent, so any wrong tap is visible at its pixel."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return 0.6 + 199.4 * torch.rand((n, P, H, W), generator=g, device="cuda", dtype=torch.float32)


def _pipeline_levels(monkeypatch, capfd, W, H, P, n, R, levels, **knobs):
    """Level 0 = R through the low-level pipeline, one bands_forward without maps; returns ({level: [n,P,h,w] numpy}, plans)."""
    import fovvideovdp_amd as fv
    from lowlevel import Pipeline
    _env(monkeypatch, **knobs)
    m = fv.fvvdp(display_name="standard_4k")
    capfd.readouterr()
    pipe = Pipeline(m, W, H, P, n)
    try:
        pipe.load_planar(R)
        pipe.bands_forward(n)
        out = {lv: pipe.export_level(lv, n).cpu().numpy() for lv in levels}
        torch.cuda.synchronize()
    finally:
        pipe.close()
    return out, _plans(capfd.readouterr().err)


# (W, H): the benchmark sizes, the 4-wave threshold (2560 columns) and odd / ragged neighbours of each
FULL_SIZES = [(3840, 2160), (1920, 1080), (2560, 1440), (3838, 2161), (1921, 1081), (2561, 1441)]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("W,H", FULL_SIZES)
@pytest.mark.parametrize("P", [2, 4])
def test_level_c_per_pixel_full_size(monkeypatch, capfd, W, H, P):
    n = 1
    R = _planar(n, P, H, W, seed=W + 7 * H + P)
    four_k = W >= 3800
    levels = (0, 2, 4) if four_k else (0, 2)
    got, plans = _pipeline_levels(monkeypatch, capfd, W, H, P, n, R, levels)
    assert [p["b"] for p in plans] == ([0, 2] if four_k else [0]), plans       # band2 wrote every level checked below
    L0 = got[0][0]
    assert np.array_equal(L0, R[0].cpu().numpy())
    c64 = _reduce64(L0, 2)
    e2 = _level_err(got[2][0], c64)
    msg = "level 2 %.3g" % e2
    if four_k:
        e4 = _level_err(got[4][0], _reduce64(c64, 2))
        msg += ", level 4 %.3g" % e4
        assert e4 <= LEVEL_TOL, msg
    print("\n%dx%d P=%d: %s, plans %s" % (W, H, P, msg, plans))
    assert e2 <= LEVEL_TOL, msg


@pytest.mark.timeout(900)
def test_level_c_per_pixel_8k(monkeypatch, capfd):
    W, H, P = 7680, 4320, 2
    R = _planar(1, P, H, W, seed=8)
    got, plans = _pipeline_levels(monkeypatch, capfd, W, H, P, 1, R, (0, 2, 4))
    assert [p["b"] for p in plans][:2] == [0, 2], plans
    c64 = _reduce64(got[0][0], 2)
    e2, e4 = _level_err(got[2][0], c64), _level_err(got[4][0], _reduce64(c64, 2))
    print("\n8K: level 2 %.3g, level 4 %.3g" % (e2, e4))
    assert e2 <= LEVEL_TOL and e4 <= LEVEL_TOL, (e2, e4)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("W,H,P", [(3840, 2160, 4), (1920, 1080, 4), (2560, 1440, 2), (3838, 2161, 2)])
def test_level_c_independent_of_launch_shape(monkeypatch, capfd, W, H, P):
    """Waves per workgroup, tickets and chunk heights decide who computes which pixel, not how: level C (and level 4 at 4K)
    bit-identical to the default launch.  Level C written by the one-level kernel (FVVDP_BAND_FUSE=0: level 1 stored, then
    reduced) is bit-identical as well -- both kernels evaluate the same two fp32 5-tap passes in the same order."""
    n = 2
    R = _planar(n, P, H, W, seed=3 * W + H)
    levels = (2, 4) if W >= 3800 else (2,)
    base, plans = _pipeline_levels(monkeypatch, capfd, W, H, P, n, R, levels)
    assert plans
    variants = [dict(BAND2_WPB=1), dict(BAND2_WPB=2), dict(BAND2_WPB=4), dict(BAND2_TICKET=0), dict(BAND2_TICKET=1),
                dict(BAND2_KR=1), dict(BAND2_KR=3), dict(BAND2_KR=7, BAND2_KR2=2), dict(BAND2_KR=20, BAND2_KR2=3),
                dict(BAND2_KR2=0)]
    for v in variants:
        got, pl = _pipeline_levels(monkeypatch, capfd, W, H, P, n, R, levels, **v)
        assert pl, v
        for lv in levels:
            assert np.array_equal(got[lv], base[lv]), (W, H, P, v, lv, pl)
    one, pl = _pipeline_levels(monkeypatch, capfd, W, H, P, n, R, levels, BAND_FUSE=0)
    assert not pl
    for lv in levels:
        d = np.max(np.abs(one[lv].astype(F64) - base[lv]) / np.abs(base[lv].astype(F64)))
        print("\n%dx%d P=%d level %d: one-level vs band2 max rel %.3g" % (W, H, P, lv, d))
        assert np.array_equal(one[lv], base[lv]), (W, H, P, lv, d)


# small sizes forced onto band2 (test_gpu_fused.IMG_SIZES): strip seams, chunk seams and every row / column parity
SMALL_SIZES = [(16, 16), (17, 19), (20, 24), (33, 107), (34, 108), (35, 109), (36, 110), (37, 215), (38, 216), (39, 217),
               (40, 218), (41, 219), (63, 64), (64, 65), (65, 66), (66, 67), (130, 323), (131, 324), (97, 433), (255, 256)]


@pytest.mark.parametrize("H,W", SMALL_SIZES)
def test_level_c_per_pixel_forced_small(monkeypatch, capfd, H, W):
    n, P = 3, 4
    R = _planar(n, P, H, W, seed=H * 1000 + W)
    want = _reduce64(R[0].cpu().numpy(), 2)
    worst = 0.0
    for kr, kr2 in ((None, None), (1, None), (2, None), (3, None), (5, None), (5, 2), (3, 1)):
        knobs = dict(BAND_FUSE=1)
        if kr is not None:
            knobs["BAND2_KR"] = kr
        if kr2 is not None:
            knobs["BAND2_KR2"] = kr2
        got, plans = _pipeline_levels(monkeypatch, capfd, W, H, P, n, R, (2,), **knobs)
        assert plans and plans[0]["b"] == 0, (H, W, kr)
        if kr2 is not None and plans[0]["n_chunks"] >= 2 and kr2 < plans[0]["kr"]:
            assert plans[0]["kr2"] == kr2, plans
        for f in range(n):
            ref64 = want if f == 0 else _reduce64(R[f].cpu().numpy(), 2)
            e = _level_err(got[2][f], ref64)
            worst = max(worst, e)
            assert e <= LEVEL_TOL, (H, W, kr, kr2, f, e, np.unravel_index(np.argmax(np.abs(got[2][f] - ref64)), ref64.shape))
    print("\n%dx%d: worst %.3g" % (H, W, worst))


def _images(n, H, W, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (n, H, W)).astype(np.uint8), rng.randint(0, 256, (n, H, W)).astype(np.uint8)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("W,H", [(3840, 2160), (1921, 1081), (2560, 1440)])
def test_level_c_per_pixel_image_batch_context(monkeypatch, capfd, W, H):
    """The batched still-image path plans its chunks for 128 slots: level C of its context against the float64 reduce."""
    import ctypes
    import fovvideovdp_amd as fv
    from fovvideovdp_amd import _native as nat
    _env(monkeypatch)
    B = 2
    tb, rb = _images(B, H, W, seed=W + H)
    m = fv.fvvdp(display_name="standard_4k")
    capfd.readouterr()
    m.predict_images(tb, rb, dim_order="BHW")
    plans = _plans(capfd.readouterr().err)
    assert plans and plans[0]["b"] == 0
    ctx = m._ctx
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    for lv in (0, 2, 4) if W >= 3800 else (0, 2):
        w, h = ctypes.c_int(), ctypes.c_int()
        nat.check(nat.lib().fvvdp_ctx_level_size(ctx.handle, lv, ctypes.byref(w), ctypes.byref(h)))
        o = torch.empty((B, 2, h.value, w.value), dtype=torch.float32, device="cuda")
        nat.check(nat.lib().fvvdp_export_level(ctx.handle, lv, B, ctypes.c_void_p(o.data_ptr()), stream))
        out[lv] = o.cpu().numpy()
    worst = 0.0
    for k in range(B):
        c64 = _reduce64(out[0][k], 2)
        worst = max(worst, _level_err(out[2][k], c64))
        if 4 in out:
            worst = max(worst, _level_err(out[4][k], _reduce64(c64, 2)))
    print("\n%dx%d batch: worst %.3g, plans %s" % (W, H, worst, plans))
    assert worst <= LEVEL_TOL, worst


# ------------------------------------------------------------------------------------------------------------------------------
# b. impulse probes
# ------------------------------------------------------------------------------------------------------------------------------
def _structured(H, W, seed):
    """Reference content: smooth gradients, a grating and mild noise (uint8), away from the code-value ends."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    v = 90 + 50 * (xx / W) + 30 * (yy / H) + 25 * np.sin(xx / 9.0) * np.cos(yy / 13.0) + rng.randint(-8, 9, (H, W))
    return np.clip(v, 0, 255).astype(np.uint8)


def _clip_rows(rows, H):
    return sorted(set(int(r) for r in rows if 0 <= r < H))


def _probe_positions(H, W, plan01, plan23=None):
    """(y, x, size) probes in level-0 pixels: corners, edge midpoints, last row / column, strip seams of pass 0+1 (and 2+3),
    rows around every chunk seam of the launched plan (tall chunks, short bottom chunks, the last chunk)."""
    P = set()
    for (y, x) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1),
                   (H - 1, W // 3), (H // 3, W - 1), (H - 2, W - 2), (1, 1)):
        P.add((y, x, 1))
    P.add((H - 2, W - 2, 2))
    P.add((0, 0, 2))
    mid = H // 2 + 3
    for s in range(1, plan01["n_strips"] + 1):
        for d in range(-14, 15):
            x = 108 * s + d
            if 0 <= x < W:
                P.add((mid, x, 1))
    if plan23 is not None:
        for s in range(1, plan23["n_strips"] + 1):
            for d in range(-14, 15):
                x = 4 * (108 * s + d)
                if 0 <= x < W:
                    P.add((mid + 1, x, 1))
    kr, kr2, nb, nc = plan01["kr"], plan01["kr2"], plan01["n_big"], plan01["n_chunks"]
    seams = [kr * k for k in range(1, nb + 1)] + [nb * kr + kr2 * j for j in range(1, nc - nb)]
    cx = W // 2 + 1
    for ka in seams:
        for d in (-9, -6, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 8):
            P.add((4 * ka + d, cx, 1))
    for y in _clip_rows(range(H - 9, H), H):
        P.add((y, cx + 5, 1))
    return sorted((y, x, s) for (y, x, s) in P if 0 <= y < H and 0 <= x < W)


def _probe_stack(ref_dev, probes):
    """[n,H,W] uint8 test images on the device: the reference with one pixel / 2x2 block moved by 80 code values."""
    t = ref_dev.unsqueeze(0).repeat(len(probes), 1, 1)
    for k, (y, x, s) in enumerate(probes):
        blk = t[k, y:y + s, x:x + s]
        t[k, y:y + s, x:x + s] = torch.where(blk < 128, blk + 80, blk - 80)
    return t


def _batched_q(monkeypatch, capfd, disp, ref_dev, probes, **knobs):
    """Q_per_ch [n_probes, bands, 2] through predict_images, up to 128 probes per call; also the band2 plans seen."""
    import fovvideovdp_amd as fv
    _env(monkeypatch, **knobs)
    m = fv.fvvdp(display_name=disp)
    out, plans = [], []
    for i in range(0, len(probes), 128):
        chunk = probes[i:i + 128]
        t = _probe_stack(ref_dev, chunk)
        r = ref_dev.unsqueeze(0).expand(len(chunk), -1, -1).contiguous()
        capfd.readouterr()
        _, st = m.predict_images(t, r, dim_order="BHW")
        plans += _plans(capfd.readouterr().err)
        out.append(np.asarray(st["Q_per_ch"])[:, :, :, 0].astype(F64))
    return np.concatenate(out, 0), plans


def _rel(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):          # (Q = 0 entries of the video check are masked there)
        return np.abs(a - b) / np.abs(b)


# measured on MI355X (see the prints): band2 vs the one-level kernel on one probe, worst 3.0e-7 (2561x1441, band 1) -- both pool
# the same per-pixel terms, in a different order of the per-wave partial sums
ONE_LEVEL_TOL = 9e-7


def _oracle_q(disp, ref, probe):
    y, x, s = probe
    t = ref.copy()
    blk = t[y:y + s, x:x + s].astype(np.int32)
    t[y:y + s, x:x + s] = np.where(blk < 128, blk + 80, blk - 80).astype(np.uint8)
    _, st = orc.Oracle(disp, dtype=F64).predict(t, ref, dim_order="HW")
    return st["Q_per_ch"][:, :, 0]


def _oracle_tol(nb):
    """Per-band bound on |Q_gpu - Q_oracle64| / Q_oracle64 for one probe, 3x the worst measured on MI355X over every probe test
    here.  A coarse band sees the impulse diluted by 4x per level: its contrast difference is a difference of nearly equal fp32
    numbers and carries their rounding (the one-level kernel computes the bands below the last band2 pass, and agrees with
    band2 to 3e-7 where they overlap).  The bands band2 computes (0-1, and 2-3 at 4K) are the tight ones."""
    measured = np.array([9.7e-6,      # band 0: HDR probes (1.8e-6 .. 2.9e-6 on SDR)
                         1.05e-5,     # band 1: HDR probes (5.6e-6 on SDR)
                         1.4e-4,      # band 2: 1080p corner probe
                         9.8e-4,      # band 3: 4K
                         3.1e-3,      # band 4: 4K
                         1.31e-2,     # band 5: 4K
                         1.28e-1])    # band 6: 4K, 30 level pixels
    return 3.0 * measured[:nb]


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("W,H,disp,n_oracle", [(1920, 1080, "standard_fhd", 24), (3840, 2160, "standard_4k", 16),
                                              (1921, 1081, "standard_fhd", 12), (2561, 1441, "standard_4k", 8)])
def test_impulse_probes_batched(monkeypatch, capfd, W, H, disp, n_oracle):
    ref = _structured(H, W, seed=W)
    ref_dev = torch.from_numpy(ref).cuda()
    _, plans = _batched_q(monkeypatch, capfd, disp, ref_dev, [(0, 0, 1)])
    p01 = [p for p in plans if p["b"] == 0][0]
    p23 = [p for p in plans if p["b"] == 2]
    assert p01["inrange"], plans                         # uint8 on an SDR display: the clamp-free variant
    probes = _probe_positions(H, W, p01, p23[0] if p23 else None)
    q2, _ = _batched_q(monkeypatch, capfd, disp, ref_dev, probes)
    q1, pl1 = _batched_q(monkeypatch, capfd, disp, ref_dev, probes, BAND_FUSE=0)
    assert not pl1
    assert np.all(q1[:, :, 0] > 0)
    e1 = _rel(q2[:, :, 0], q1[:, :, 0])
    k = int(np.argmax(e1.max(axis=1)))
    print("\n%dx%d: %d probes, band2 vs one-level max rel %.3g (probe %s), per band %s" % (
        W, H, len(probes), e1.max(), probes[k], np.array2string(e1.max(axis=0), precision=2)))
    assert e1.max() <= ONE_LEVEL_TOL, (probes[k], e1[k])
    # the float64 oracle on a fixed sample: corners and edges first, then evenly over the rest
    sample = list(range(min(6, len(probes)))) + list(np.linspace(6, len(probes) - 1, max(0, n_oracle - 6)).astype(int))
    errs = np.stack([_rel(q2[i, :, 0], _oracle_q(disp, ref, probes[i])[:, 0]) for i in sorted(set(sample))])
    print("%dx%d: band2 vs float64 oracle, worst per band %s" % (W, H, np.array2string(errs.max(axis=0), precision=2)))
    tol = _oracle_tol(q2.shape[1])
    assert np.all(errs <= tol), (errs.max(axis=0), tol)


@pytest.mark.timeout(900)
def test_impulse_probes_single_predict(monkeypatch, capfd):
    """predict() plans for n = 1: other chunk seams than the 128-slot batch plan.  A subset of the probes, one call each."""
    import fovvideovdp_amd as fv
    W, H, disp = 1920, 1080, "standard_fhd"
    ref = _structured(H, W, seed=5)
    _env(monkeypatch)
    capfd.readouterr()
    fv.fvvdp(display_name=disp).predict(ref, ref, dim_order="HW")
    p01 = [p for p in _plans(capfd.readouterr().err) if p["b"] == 0][0]
    probes = _probe_positions(H, W, p01)
    probes = [p for p in probes if p[1] % 108 in (0, 1, 94, 95, 96, 107) or p[1] in (0, W - 1) or p[0] % (4 * p01["kr"]) in (0, 1, 4 * p01["kr"] - 1)]
    probes = probes[:40]
    qs = {}
    for fuse in (None, 0):
        _env(monkeypatch, **({} if fuse is None else dict(BAND_FUSE=0)))
        m = fv.fvvdp(display_name=disp)
        res = []
        for (y, x, s) in probes:
            t = ref.copy()
            blk = t[y:y + s, x:x + s].astype(np.int32)
            t[y:y + s, x:x + s] = np.where(blk < 128, blk + 80, blk - 80).astype(np.uint8)
            _, st = m.predict(t, ref, dim_order="HW")
            res.append(st["Q_per_ch"][:, 0, 0].astype(F64))
        qs[fuse] = np.stack(res)
    e = _rel(qs[None], qs[0])
    print("\nsingle predict: %d probes, band2 vs one-level max rel %.3g" % (len(probes), e.max()))
    assert e.max() <= ONE_LEVEL_TOL, probes[int(np.argmax(e.max(axis=1)))]
    errs = np.stack([_rel(qs[None][i], _oracle_q(disp, ref, probes[i])[:, 0]) for i in range(0, len(probes), 5)])
    print("single predict: vs float64 oracle, worst per band %s" % np.array2string(errs.max(axis=0), precision=2))
    assert np.all(errs <= _oracle_tol(errs.shape[1])), errs.max(axis=0)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("W,H,disp,N,oracle", [(1920, 1080, "standard_fhd", 6, True), (3840, 2160, "standard_4k", 4, False)])
def test_impulse_probe_video(monkeypatch, capfd, W, H, disp, N, oracle):
    """A short clip (P = 4, the benchmark's path) with the impulse in one frame, at a strip seam and near the bottom."""
    import fovvideovdp_amd as fv
    ref = np.stack([_structured(H, W, seed=f) for f in range(N)])
    test = ref.copy()
    y, x = H - 3, 108 * 3 + 1
    test[N // 2, y, x] = int(ref[N // 2, y, x]) + (80 if ref[N // 2, y, x] < 128 else -80)
    test[N // 2, 4 * 5 - 1, 108 * 2 - 13] = 255
    out = {}
    for fuse in (None, 0):
        _env(monkeypatch, **({} if fuse is None else dict(BAND_FUSE=0)))
        capfd.readouterr()
        _, st = fv.fvvdp(display_name=disp).predict(test, ref, dim_order="FHW", frames_per_second=30)
        plans = _plans(capfd.readouterr().err)
        assert (fuse is None) == bool(plans) and all(p["P"] == 4 for p in plans)
        out[fuse] = st["Q_per_ch"].astype(F64)
    e = _rel(out[None], out[0])[out[0] > 0]
    print("\nvideo %dx%d: band2 vs one-level max rel %.3g" % (W, H, e.max()))
    assert e.max() <= ONE_LEVEL_TOL
    if oracle:
        _, ost = orc.Oracle(disp, dtype=F64).predict(test, ref, dim_order="FHW", frames_per_second=30)
        qo = ost["Q_per_ch"]
        tol = _oracle_tol(qo.shape[0])[:, None, None]
        eo = _rel(out[None], qo)
        print("video %dx%d: vs float64 oracle per band %s" % (W, H, np.array2string(np.nanmax(eo, axis=(1, 2)), precision=2)))
        mask = qo > 1e-6 * qo.max()
        assert np.all((eo <= tol) | ~mask), np.nanmax(eo, axis=(1, 2))


@pytest.mark.timeout(900)
def test_impulse_probes_hdr_clamps_bind(monkeypatch, capfd):
    """standard_hdr_pq with float input runs band2_kernel<2, false>: bright impulses on a black area make both clamps bind
    (L_bkg >= 0.1, contrast <= 1000).  Against the one-level kernel and the float64 oracle."""
    W, H, disp = 1920, 1080, "standard_hdr_pq"
    ref = (_structured(H, W, seed=9).astype(np.float32) / np.float32(255)) * np.float32(0.6)
    ref[:, :W // 3] = 0.0                                             # black area on the left third, seams at 108, 216, ...
    ref_dev = torch.from_numpy(ref).cuda()
    probes = [(0, 0, 1), (H // 2, 107, 1), (H // 2, 108, 1), (H // 2, 96, 1), (H - 1, 215, 2), (H // 3, 324, 1), (5, 434, 1),
              (H - 1, W - 1, 1), (H // 2, 1080, 1), (H // 2 + 1, 1190, 1)]

    def stack(ps):
        t = ref_dev.unsqueeze(0).repeat(len(ps), 1, 1)
        for k, (y, x, s) in enumerate(ps):
            t[k, y:y + s, x:x + s] = 0.9 if ref[y, x] < 0.3 else 0.05    # ~2000 cd/m^2 on black
        return t
    import fovvideovdp_amd as fv
    qs = {}
    for fuse in (None, 0):
        _env(monkeypatch, **({} if fuse is None else dict(BAND_FUSE=0)))
        capfd.readouterr()
        _, st = fv.fvvdp(display_name=disp).predict_images(stack(probes), ref_dev.unsqueeze(0).expand(len(probes), -1, -1).contiguous(),
                                                           dim_order="BHW")
        plans = _plans(capfd.readouterr().err)
        if fuse is None:
            assert plans and not plans[0]["inrange"], plans               # the variant with the clamps ran
        qs[fuse] = np.asarray(st["Q_per_ch"])[:, :, 0, 0].astype(F64)
    e = _rel(qs[None], qs[0])
    print("\nhdr: band2 vs one-level max rel %.3g" % e.max())
    assert e.max() <= ONE_LEVEL_TOL
    # the clamps bind on the probes over black: check on the oracle's own bands
    o = orc.Oracle(disp, dtype=F64)
    o.capture = {}
    t = stack(probes[1:2]).cpu().numpy()[0]
    o.predict(t, ref, dim_order="HW")
    assert np.min(o.capture["L_bkg"][0][0]) == 0.1 and np.max(o.capture["bands"][0][0]) == 1000.0
    errs = np.stack([_rel(qs[None][i], orc.Oracle(disp, dtype=F64).predict(stack([p]).cpu().numpy()[0], ref, dim_order="HW")[1]
                          ["Q_per_ch"][:, 0, 0]) for i, p in enumerate(probes)])
    print("hdr: vs float64 oracle, worst per band %s" % np.array2string(errs.max(axis=0), precision=2))
    assert np.all(errs <= _oracle_tol(errs.shape[1])), errs.max(axis=0)
