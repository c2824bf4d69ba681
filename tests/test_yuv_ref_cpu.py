"""The yardstick of tests/test_gpu_yuv_pixels.py without a GPU (tests/yuv_channels_ref.py): its unpack equals the oracle's restatement
of the reference's, its float32 chain reproduces the oracle's temporal channels bit for bit, the product's own torch unpack agrees
with it, and the comparison the GPU tests apply -- on the clips they use -- rejects six deliberately wrong pipelines by at least
ten times its bound.  The GPU tests hold the kernels against this reference, so it is pinned here on code that shares nothing with
the kernels."""
import numpy as np
import pytest

from oracle import fvvdp_oracle as orc

import yuv_channels_ref as yref

F32, F64 = np.float32, np.float64


@pytest.mark.parametrize("color_space", ["bt709", "bt2020nc"])
@pytest.mark.parametrize("chroma_ss", ["420", "444"])
@pytest.mark.parametrize("bit_depth", [8, 10, 12, 16])
def test_reference_equals_the_oracle(color_space, chroma_ss, bit_depth):
    H, W, N, fps = 12, 16, 4, 30
    test, ref = yref.yuv_clip(N, H, W, bit_depth, chroma_ss, seed=[bit_depth, int(chroma_ss), len(color_space)])
    for f in range(N):
        mine = yref.yuv_rgb(test[f], W, H, bit_depth, chroma_ss, yref.MATRICES[color_space], F64)
        theirs = orc.yuv_unpack(test[f], W, H, bit_depth, chroma_ss, color_space, dtype=F64)
        assert mine.dtype == F64 and mine.shape == (H, W, 3)
        assert np.max(np.abs(mine - theirs)) <= 1e-12
    o = orc.Oracle("standard_fhd")
    o.capture = {}
    o.predict_yuv(test, ref, fps, W, H, bit_depth=bit_depth, chroma_ss=chroma_ss, color_space=color_space)
    fl = orc.filter_len(fps)
    R, S = yref.yuv_temporal_channels(test, ref, W, H, bit_depth, chroma_ss, yref.MATRICES[color_space], o.photometry, o.rgb2y,
                                      orc.temporal_filters(fps), orc.window_frame_indices(N, fl, "replicate"), dtype=F32)
    assert R.dtype == F32 and R.shape == (N, 4, H, W) and S.shape == R.shape
    assert len(o.capture["R"]) == N
    for f in range(N):
        assert np.array_equal(R[f], o.capture["R"][f]), f
    assert np.all(S[:, :2] >= np.abs(R[:, :2])) and np.all(S[:, 2:] * (1 + 1e-5) >= np.abs(R[:, 2:]))


def test_error_scale_is_the_absolute_tap_sum():
    """S on constant luminance L is L * sum |taps|; the transient channel itself is under 1 % of it there, which is why |R| is no scale."""
    H, W, N, fps = 4, 4, 3, 30
    frame = np.concatenate([np.full(H * W, 180), np.full(2 * H * W, 128)]).astype(np.uint8)
    clip = np.stack([frame] * N)
    taps = orc.temporal_filters(fps)
    ph = yref.photometry_for("standard_fhd")
    R, S = yref.yuv_temporal_channels(clip, clip, W, H, 8, "444", yref.MATRICES["bt709"], ph, [0.2126, 0.7152, 0.0722], taps,
                                      orc.window_frame_indices(N, orc.filter_len(fps), "replicate"))
    L = R[0, 0, 0, 0] / np.sum(taps[0].astype(F64))
    assert np.allclose(S[:, 0], L * np.sum(np.abs(taps[0].astype(F64))), rtol=1e-12)
    assert np.allclose(S[:, 2], L * np.sum(np.abs(taps[1].astype(F64))), rtol=1e-12)
    assert np.max(np.abs(R[:, 2])) < 0.01 * np.min(S[:, 2])            # sum taps / sum |taps| of the transient filter: 0.0066


@pytest.mark.parametrize("H,W,chroma_ss", [(8, 12, "444"), (5, 12, "444"), (2, 4, "420")])
@pytest.mark.parametrize("matrix", ["bt709", "dense"])
def test_product_torch_unpack_agrees(H, W, chroma_ss, matrix):
    """The product's torch restatement of the unpack (the path of callers that ask for single frames), 16-bit codes up to 65535:
    within 5e-7 absolute of the float64 reference (float32 arithmetic on values of order 1; measured 0.75-1.5e-7)."""
    import torch
    from fovvideovdp_amd import fvvdp_video_source_yuv_frames
    rng = np.random.default_rng([H, W, len(matrix)])
    elems = H * W + 2 * (H * W // 4 if chroma_ss == "420" else H * W)
    clip = rng.integers(0, 65536, (3, elems)).astype(np.uint16)
    clip[0, :3] = (32768, 65535, 40000)
    assert (clip >= 32768).any()
    vs = fvvdp_video_source_yuv_frames(clip, clip, 30, W, H, bit_depth=16, chroma_ss=chroma_ss, color_space="bt709",
                                       display_photometry="standard_fhd")
    M = np.asarray(yref.MATRICES[matrix], dtype=F32)
    vs.ycbcr2rgb = M.tolist()
    for f in range(clip.shape[0]):
        got = vs.unpack(vs.test_yuv[f], torch.device("cpu")).numpy()
        want = yref.yuv_rgb(clip[f], W, H, 16, chroma_ss, M, F64)
        assert got.shape == want.shape
        assert np.max(np.abs(got.astype(F64) - want)) <= 5e-7


# ---- power of the comparison: six wrong pipelines, on the GPU tests' own clips ---------------------------------------------------
def _wrong_upsample(what):
    def up(uv, H, W, F):
        uvh, uvw = uv.shape[1:]

        def axis(n_out, n_in, unclamped):
            src = np.maximum((np.arange(n_out, dtype=F) + F(0.5)) * F(0.5) - F(0.5), F(0))
            i0 = src.astype(np.int64)
            i1 = np.where(i0 + 1 > n_in - 1, n_in - 2, i0 + 1) if unclamped else np.minimum(i0 + 1, n_in - 1)
            return i0, i1, (src - i0.astype(F)).astype(F)
        y0, y1, fy = axis(H, uvh, what == "last_row_unclamped")
        x0, x1, fx = axis(W, uvw, what == "right_edge_unclamped")
        if what == "weights_swapped":
            fx = np.where(fx > 0, F(1) - fx, fx).astype(F)
        fy, fx = fy[None, :, None], fx[None, None, :]
        top = (F(1) - fx) * uv[:, y0][:, :, x0] + fx * uv[:, y0][:, :, x1]
        bot = (F(1) - fx) * uv[:, y1][:, :, x0] + fx * uv[:, y1][:, :, x1]
        return ((F(1) - fy) * top + fy * bot).astype(F)
    return up


def _mutant(c, what):
    """The float32 chain of case `c` with one defect."""
    test, ref, W, H, bd, css, M, ph, rgb2y, taps, idx = c["args"]
    kw = {}
    if what in ("weights_swapped", "right_edge_unclamped", "last_row_unclamped"):
        assert css == "420"
        kw["upsample"] = _wrong_upsample(what)
    elif what == "m1_m2_exchanged":
        M = M.copy()
        M[0, 1], M[0, 2] = M[0, 2], M[0, 1]
    elif what == "sign_extended":
        test, ref = test.view(np.int16), ref.view(np.int16)
    elif what == "window_rotated":
        idx = np.roll(idx, 1, axis=1)
    else:
        raise ValueError(what)
    return yref.yuv_temporal_channels(test, ref, W, H, bd, css, M, ph, rgb2y, taps, idx, dtype=F32, **kw)[0]


POWER = [("weights_swapped", (8, 8, 8, "420", "standard_fhd", 30, "bt709")),
         ("weights_swapped", (8, 252, 10, "420", "standard_hdr_pq", 30, "bt2020nc")),
         ("right_edge_unclamped", (8, 8, 8, "420", "standard_fhd", 30, "bt709")),
         ("right_edge_unclamped", (8, 500, 8, "420", "standard_hdr_pq", 60, "bt709")),
         ("last_row_unclamped", (8, 8, 8, "420", "standard_fhd", 30, "bt709")),
         ("last_row_unclamped", (6, 36, 12, "420", "standard_hdr_pq", 30, "bt709")),
         ("m1_m2_exchanged", (8, 252, 8, "420", "standard_fhd", 30, "dense")),
         ("m1_m2_exchanged", (8, 250, 16, "444", "standard_hdr_pq", 30, "dense")),
         ("sign_extended", (8, 248, 16, "420", "standard_fhd", 30, "bt709")),
         ("sign_extended", (5, 36, 16, "444", "standard_hdr_pq", 30, "bt2020nc")),
         ("window_rotated", (8, 8, 8, "420", "standard_fhd", 30, "bt709")),
         ("window_rotated", (8, 248, 12, "444", "standard_hdr_pq", 60, "bt709"))]


@pytest.mark.parametrize("what,case", POWER)
def test_comparison_rejects_a_wrong_pipeline(what, case):
    c = yref.case_reference(*case)
    err, e_ref = yref.assert_channels_close(c["R32"], c["R32"], c["R64"], c["S64"])       # the float32 chain itself passes
    bad = _mutant(c, what)
    e_bad = yref.channel_error(bad, c["R64"], c["S64"])
    assert e_bad >= 10 * yref.error_bound(e_ref), (what, e_bad, yref.error_bound(e_ref))
    with pytest.raises(AssertionError):
        yref.assert_channels_close(bad, c["R32"], c["R64"], c["S64"])


def test_clips_carry_what_the_cases_need():
    """Code extremes, both planted rows, bright frames above the sRGB toe, 16-bit codes that are negative as int16, and streams and
    frames that all differ."""
    for bd, css in ((8, "420"), (10, "444"), (16, "420")):
        c = yref.case_reference(8, 252, bd, css, "standard_fhd", 30)
        t, r, top = c["test"], c["ref"], (1 << bd) - 1
        assert t.min() == 0 and t.max() == top and r.min() == 0 and r.max() == top
        assert (t[0, 252:504] == 0).all() and (t[0, 504:756] == top).all()
        assert c["bright_rgb_min"] > 0.05
        assert len({a.tobytes() for s in (t, r) for a in s}) == 2 * c["N"]
        if bd == 16:
            assert (t >= 32768).any() and (r >= 32768).any()
    assert c["N"] == 11 and yref.case_reference(8, 8, 8, "420", "standard_fhd", 240)["N"] == 67
