"""Batched still-image evaluation on the GPU (fvvdp.predict_images / predict_image_pairs, include/fvvdp_hip_images.h): goldens
inside a batch, batch invariance (bit-identical), agreement with single predict() calls, the oracle, mixed inputs, per-pair
range flags and the asynchrony of a batch."""
import ctypes
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")


def load(name):
    return np.load(os.path.join(G, name + ".npz"))


@pytest.fixture(scope="module")
def fv():
    import fovvideovdp_amd
    from fovvideovdp_amd import _native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _native.lib()
    return fovvideovdp_amd


def check_q(q, gq, coarse=1e-3, fine=1.5e-4):
    """The tolerance rule of the single-image tests (test_gpu_parity.check_q)."""
    q, gq = np.asarray(q, np.float64), np.asarray(gq, np.float64)
    assert q.shape == gq.shape
    assert np.all(np.abs(q - gq) <= coarse * np.abs(gq) + 1e-6 * np.max(np.abs(gq)))
    nb = min(3, q.shape[0])
    assert np.all(np.abs(q[:nb] - gq[:nb]) <= fine * np.abs(gq[:nb]) + 1e-7 * np.max(np.abs(gq)))


def gaussblur(img, sigma):
    from scipy.ndimage import gaussian_filter
    out = np.zeros_like(img)
    for cc in range(img.shape[2]):
        out[..., cc] = gaussian_filter(img[..., cc], sigma, mode="nearest", truncate=2.0)
    return out


def rand_pairs(n, H, W, C=3, dtype=np.uint8, seed=0):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        r = rs.rand(C, H, W).astype(np.float32)
        t = np.clip(r + 0.08 * rs.randn(C, H, W).astype(np.float32), 0, 1)
        if dtype == np.uint8:
            r, t = (r * 255).round().astype(np.uint8), (t * 255).round().astype(np.uint8)
        elif dtype == np.uint16:
            r, t = (r * 65535).round().astype(np.uint16), (t * 65535).round().astype(np.uint16)
        out.append((t, r))
    return out


def stack(pairs):
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def near(qa, qb, ja, jb, tol=2e-6):
    assert abs(float(ja) - float(jb)) <= tol, (float(ja), float(jb))
    qa, qb = np.asarray(qa, np.float64), np.asarray(qb, np.float64)
    assert np.all(np.abs(qa - qb) <= tol * np.abs(qb) + 1e-12), np.max(np.abs(qa - qb) / (np.abs(qb) + 1e-30))


def test_goldens_inside_a_batch(fv):
    z0, z1 = load("g0_wavy_facade_blur_4k"), load("g1_crop512_blur_fhd")
    ref0 = z0["ref_u16"]
    test0 = gaussblur(ref0, 2)
    # g0 (README known answer) among other pairs of its size, HWC uint16
    others = [(np.roll(ref0, k * 7, axis=1), ref0) for k in range(1, 4)]
    m = fv.fvvdp(display_name="standard_4k")
    q, st = m.predict_images(np.stack([others[0][0], test0] + [o[0] for o in others[1:]]),
                             np.stack([ref0] * 4), dim_order="BHWC")
    assert q.shape == (4,) and q.device.type == "cuda"
    assert abs(float(q[1]) - 8.693) < 1e-3 and abs(float(q[1]) - float(z0["jod"])) < 2e-5
    check_q(st["Q_per_ch"][1][:, 0:1], z0["Q_per_ch"][:, 0:1], coarse=7e-5, fine=7e-5)
    assert np.all(st["Q_per_ch"][:, :, 1] == 0) and st["Q_per_ch"].shape == (4, 7, 2, 1)
    assert np.allclose(st["rho_band"], z0["rho_band"], rtol=1e-12)
    # g1 (512^2 crop)
    ref1 = ref0[85:597, 256:768]
    m = fv.fvvdp(display_name="standard_fhd")
    res = m.predict_image_pairs([(ref1[::-1].copy(), ref1), (z1["test_u16"], ref1), (ref1, ref1)], dim_order="HWC")
    assert abs(float(res[1][0]) - float(z1["jod"])) < 2e-5
    check_q(res[1][1]["Q_per_ch"][:, 0:1], z1["Q_per_ch"][:, 0:1], coarse=4e-5, fine=4e-5)
    assert abs(float(res[2][0]) - 10.0) < 1e-6
    # g2 (uint16 gray, 68x121: a pixel count that takes the four-pixel loads) behind standard_phone
    from fovvideovdp_amd.synth import synth_video_pair
    z2 = load("g2_image_68x121_u16gray")
    test, ref = synth_video_pair(6, 68, 121, C=1)
    t16 = test[0, 0, 0].numpy().astype(np.uint16) * 257
    r16 = ref[0, 0, 0].numpy().astype(np.uint16) * 257
    m = fv.fvvdp(display_name="standard_phone")
    tb = np.stack([r16, t16, t16[::-1].copy()])
    rb = np.stack([r16, r16, r16])
    q, st = m.predict_images(tb, rb, dim_order="BHW")
    assert abs(float(q[1]) - float(z2["jod"])) < 1e-4
    check_q(st["Q_per_ch"][1][:, 0:1], z2["Q_per_ch"][:, 0:1])


def test_heatmaps_in_a_batch(fv):
    from fovvideovdp_amd.synth import synth_video_pair
    z = load("g6_heatmaps")
    t2, r2 = synth_video_pair(1, 135, 240)
    t2, r2 = t2[0, :, 0], r2[0, :, 0]
    for mode, tag in (("raw", "raw"), ("threshold", "thr")):
        m = fv.fvvdp(display_name="standard_4k", heatmap=mode)
        q, st = m.predict_images(torch.stack([r2, t2, t2.flip(2)]), torch.stack([r2, r2, r2]), dim_order="BCHW")
        hm, g = st["heatmap"], z[f"image_{tag}"]
        assert hm.dtype == torch.float16 and tuple(hm.shape) == (3,) + g.shape[1:]
        assert abs(float(q[1]) - float(z[f"image_{tag}_jod"])) < 1e-4
        d = np.abs(hm[1:2].float().numpy() - g.astype(np.float32))
        assert np.max(d / (np.abs(g.astype(np.float32)) + 2e-3)) < 2e-2, tag
        # the single call on the same pair
        q1, st1 = m.predict(t2.flip(2), r2, dim_order="CHW")
        near(st["Q_per_ch"][2], st1["Q_per_ch"], q[2], q1)
        d1 = np.abs(hm[2:3].float().numpy() - st1["heatmap"].float().numpy())
        assert np.max(d1 / (np.abs(st1["heatmap"].float().numpy()) + 2e-3)) < 2e-2, tag


def test_batch_invariance_is_bit_exact(fv):
    pairs = rand_pairs(50, 96, 136, seed=3)
    t, r = stack(pairs)
    k = 37
    m = fv.fvvdp(display_name="standard_fhd")
    qa, sa = m.predict_images(t[k:k + 1], r[k:k + 1])
    qb, sb = m.predict_images(t, r)
    assert np.array_equal(sa["Q_per_ch"][0], sb["Q_per_ch"][k]) and float(qa[0]) == float(qb[k])
    ms = fv.fvvdp(display_name="standard_fhd", batch_frames=7)          # forced split into batches of 7
    qc, sc = ms.predict_images(t, r)
    assert np.array_equal(sc["Q_per_ch"], sb["Q_per_ch"]) and torch.equal(qc, qb)
    res = m.predict_image_pairs([(pairs[k][0], pairs[k][1]), (pairs[0][0], pairs[0][1])], dim_order="CHW")
    assert np.array_equal(res[0][1]["Q_per_ch"], sb["Q_per_ch"][k]) and float(res[0][0]) == float(qb[k])
    assert res[0][1]["Q_per_ch"].shape == (sb["Q_per_ch"].shape[1], 2, 1)


def _single_vs_batch(m, tb, rb, dim_order="BCHW", fix=None):
    q, st = m.predict_images(tb, rb, dim_order=dim_order, fixation_point=fix)
    for k in range(tb.shape[0]):
        q1, st1 = m.predict(tb[k], rb[k], dim_order=dim_order[1:], fixation_point=None if fix is None else fix[k])
        near(st["Q_per_ch"][k], st1["Q_per_ch"], q[k], q1)
    return q, st


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("C", [3, 1])
def test_against_single_calls(fv, dtype, C):
    pairs = rand_pairs(4, 97, 131, C=C, dtype=dtype, seed=C)          # 97 x 131: odd pixel count, one-pixel loads
    tb, rb = stack(pairs)
    for disp in ("standard_4k", "standard_hdr_pq"):
        _single_vs_batch(fv.fvvdp(display_name=disp), tb, rb)
    pairs = rand_pairs(3, 64, 120, C=C, dtype=dtype, seed=5)          # four-pixel loads
    _single_vs_batch(fv.fvvdp(display_name="standard_fhd"), *stack(pairs))


def test_level0_bit_equal_to_single_path(fv):
    from fovvideovdp_amd import _native as nat
    for dtype, disp in ((np.uint8, "standard_fhd"), (np.uint16, "standard_hdr_pq"), (np.float32, "standard_4k")):
        for (H, W) in ((64, 120), (67, 121)):
            pairs = rand_pairs(3, H, W, dtype=dtype, seed=11)
            tb, rb = stack(pairs)
            m = fv.fvvdp(display_name=disp)
            m.predict_images(tb, rb)
            ctx = m._ctx
            out = torch.empty((3, 2, H, W), dtype=torch.float32, device="cuda")
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            nat.check(nat.lib().fvvdp_export_level(ctx.handle, 0, 3, ctypes.c_void_p(out.data_ptr()), stream))
            batched = out.cpu()
            for k in range(3):
                m1 = fv.fvvdp(display_name=disp)
                m1.predict(tb[k], rb[k], dim_order="CHW")
                o1 = torch.empty((1, 2, H, W), dtype=torch.float32, device="cuda")
                nat.check(nat.lib().fvvdp_export_level(m1._ctx.handle, 0, 1, ctypes.c_void_p(o1.data_ptr()), stream))
                assert torch.equal(o1.cpu()[0], batched[k]), (dtype, H, W, k)


def test_foveated_per_pair_fixation(fv):
    pairs = rand_pairs(3, 120, 160, seed=7)
    tb, rb = stack(pairs)
    fix = np.array([[20, 30], [80, 60], [150, 100]], dtype=np.float32)
    q, st = _single_vs_batch(fv.fvvdp(display_name="standard_fhd", foveated=True), tb, rb, fix=fix)
    q2, _ = fv.fvvdp(display_name="standard_fhd", foveated=True).predict_images(tb, rb, fixation_point=fix[::-1].copy())
    assert float(q2[0]) != float(q[0])          # the fixation reaches its own pair


def test_against_oracle_random_sizes(fv):
    from oracle import fvvdp_oracle as orc
    for (H, W, disp) in ((97, 263, "standard_4k"), (130, 129, "standard_fhd"), (271, 481, "standard_4k"), (64, 96, "standard_fhd")):
        pairs = rand_pairs(3, H, W, seed=H)
        tb, rb = stack(pairs)
        q, st = fv.fvvdp(display_name=disp).predict_images(tb, rb)
        for k in range(3):
            oq, ostats = orc.Oracle(disp).predict(tb[k][None, :, None], rb[k][None, :, None], frames_per_second=0)
            assert abs(float(q[k]) - float(oq)) < 1e-4, (H, W, k)
            check_q(st["Q_per_ch"][k], ostats["Q_per_ch"])


def test_mixed_inputs_keep_order_and_bits(fv):
    m = fv.fvvdp(display_name="standard_fhd")
    a8 = rand_pairs(3, 72, 100, seed=1)
    a16 = rand_pairs(2, 80, 90, C=1, dtype=np.uint16, seed=2)
    af = rand_pairs(2, 72, 100, dtype=np.float32, seed=4)
    dev = torch.device("cuda")
    big = torch.from_numpy(np.stack([a8[2][0], a8[2][0]], axis=-1)).to(dev)        # a non-contiguous device view
    view_t = big[..., 0]
    pairs = [a8[0], (torch.from_numpy(a16[0][0].view(np.int16)).to(dev), a16[0][1]), af[0], (view_t, torch.from_numpy(a8[2][1]).to(dev)),
             a8[1], af[1], a16[1], (af[0][0], a8[0][1])]                            # the last: float test, uint8 reference
    res = m.predict_image_pairs(pairs, dim_order="CHW")
    assert len(res) == len(pairs)
    g8 = m.predict_images(*stack([a8[0], a8[2], a8[1]]))
    g16 = m.predict_images(*stack(a16))
    gf = m.predict_images(*stack(af))
    for i, (grp, j) in enumerate([(g8, 0), (g16, 0), (gf, 0), (g8, 1), (g8, 2), (gf, 1), (g16, 1)]):
        assert np.array_equal(res[i][1]["Q_per_ch"], grp[1]["Q_per_ch"][j]), i
        assert float(res[i][0]) == float(grp[0][j]), i
        assert res[i][1]["width"] == pairs[i][0].shape[-1] and res[i][1]["N_frames"] == 1
    q1, st1 = m.predict(af[0][0], a8[0][1], dim_order="CHW")
    near(res[7][1]["Q_per_ch"], st1["Q_per_ch"], res[7][0], q1)


def test_per_pair_range_flags(fv, caplog):
    pairs = rand_pairs(5, 64, 64, dtype=np.float32, seed=9)
    tb, rb = stack(pairs)
    tb[3, 0, 5, 5] = 1.5
    m = fv.fvvdp(display_name="standard_fhd")
    with caplog.at_level(logging.WARNING):
        _, st = m.predict_images(tb, rb)
    assert list(st["range_flags"]) == [False, False, False, True, False]
    msgs = [r.message for r in caplog.records if "Pixel outside the valid range 0-1" in r.message]
    assert len(msgs) == 1 and "pair 3" in msgs[0]
    _, st = m.predict_images(torch.from_numpy(tb).cuda(), torch.from_numpy(rb).cuda(), sync=False)
    m.finish(st)
    assert list(st["range_flags"]) == [False, False, False, True, False]


def test_async_batch_makes_no_sync_or_allocation(fv):
    from fovvideovdp_amd import _native as nat
    pairs = rand_pairs(20, 128, 128, seed=12)
    tb, rb = (torch.from_numpy(a).cuda() for a in stack(pairs))
    m = fv.fvvdp(display_name="standard_fhd")
    q0, st0 = m.predict_images(tb, rb)                                    # warm-up: context, tables
    stats = (ctypes.c_int64 * 3)()
    nat.check(nat.lib().fvvdp_ctx_call_stats(m._ctx.handle, stats))
    before = list(stats)
    q, st = m.predict_images(tb, rb, sync=False)
    assert isinstance(st["Q_per_ch"], torch.Tensor) and st["Q_per_ch"].shape == (20, st0["Q_per_ch"].shape[1], 2, 1)
    nat.check(nat.lib().fvvdp_ctx_call_stats(m._ctx.handle, stats))
    assert list(stats) == before
    m.finish(st)
    assert np.array_equal(st["Q_per_ch"], st0["Q_per_ch"]) and torch.equal(q, q0)
    # errors leave the metric usable
    with pytest.raises(RuntimeError, match="same shape"):
        m.predict_images(tb, rb[:, :, :64])
    with pytest.raises(RuntimeError):
        m.predict_images(tb[:, :2], rb[:, :2])                             # two colour channels
    q2, st2 = m.predict_images(tb, rb)
    assert np.array_equal(st2["Q_per_ch"], st0["Q_per_ch"])


def test_pairs_on_a_foveated_metric(fv):
    """predict_image_pairs on a foveated metric: the gaze defaults to each pair's image centre, as in predict()."""
    a = rand_pairs(2, 120, 160, seed=21)
    b = rand_pairs(1, 90, 130, C=1, dtype=np.float32, seed=22)
    pairs = [a[0], b[0], a[1]]
    m = fv.fvvdp(display_name="standard_fhd", foveated=True)
    res = m.predict_image_pairs(pairs, dim_order="CHW")
    for (t, r), (q, st) in zip(pairs, res):
        q1, st1 = m.predict(t, r, dim_order="CHW")
        near(st["Q_per_ch"], st1["Q_per_ch"], q, q1)
    fixes = [[10, 20], None, [150, 100]]
    res = m.predict_image_pairs(pairs, dim_order="CHW", fixation_points=fixes)
    for (t, r), f, (q, st) in zip(pairs, fixes, res):
        q1, st1 = m.predict(t, r, dim_order="CHW", fixation_point=f)
        near(st["Q_per_ch"], st1["Q_per_ch"], q, q1)


def test_pairs_range_warning_names_the_input_pair(fv, caplog):
    a = rand_pairs(2, 64, 64, dtype=np.float32, seed=31)
    b = rand_pairs(2, 48, 80, dtype=np.float32, seed=32)
    bad = b[1][0].copy()
    bad[1, 3, 3] = -0.2
    pairs = [a[0], b[0], a[1], (bad, b[1][1])]            # the offending pair is input 3, index 1 of its size group
    m = fv.fvvdp(display_name="standard_fhd")
    with caplog.at_level(logging.WARNING):
        res = m.predict_image_pairs(pairs, dim_order="CHW")
    msgs = [r.message for r in caplog.records if "Pixel outside the valid range 0-1" in r.message]
    assert msgs == ["Pixel outside the valid range 0-1 (image pair 3)"], msgs
    assert [st["out_of_range"] for _, st in res] == [False, False, False, True]
