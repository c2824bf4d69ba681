"""GPU: the raw-YUV ingest kernels, pixel by pixel, against a float64 restatement of the reference's unpack (tests/yuv_channels_ref.py,
pinned without a GPU by tests/test_yuv_ref_cpu.py).

Every case builds an fvvdp_video_source_yuv_frames, runs predict_video_source, reads level 0 of the context (the temporal channels
of the clip) and compares EVERY pixel of every frame and plane; no pixel is excluded.  The frames are the smallest that still hit
every seam of temporal_yuv_vec_kernel, which takes 4 pixels per lane and 62 quads per wave:
  (8,8)     two quads per row, nearly every lane clamped to the frame
  (8,248)   a row is exactly one wave's run: both halo lanes belong to other rows
  (8,252)   63 quads per row: the run ends one quad before the row end and every later row starts one lane further on
  (8,500)   runs cross row ends in the middle of a wave
  (6,36), (5,36) 4:4:4   odd (chroma) height
  (8,250), (200,6)       widths that are no multiple of 4: temporal_yuv_kernel
The clips (yuv_channels_ref.yuv_clip) cycle through random codes over the whole code range with a row of zeros and a row of the
largest code, bright-only frames (the wave-uniform branch that skips the sRGB toe) and frames bright on the left and random on the
right; N = ring length + 3 frames, so each straight-line FIR variant of the register window produces a live frame.

Tolerance (yuv_channels_ref.error_bound): max |R_gpu - R64| / S <= 4 * max(e_ref, 4 * 2^-24), where S = sum_k |tap_k| * L_k is the
per-pixel scale of the filter's terms and e_ref the same error of the reference's own float32 chain on the same clip, computed at
run time.  The FVVDP_DEBUG_VARIANT line of fvvdp_temporal_channels_yuv proves which instantiation ran.

Measured on MI355X, worst case per display model (error / S; e_ref of the float32 chain; share of the bound), the three paths within
10 % of each other: sRGB 7.2e-7 (e_ref 5.8e-7, 0.31), PQ 2.06e-5 (4.1e-5, 0.14), gamma 2.4 6.2e-7 (5.5e-7, 0.28), linear 2.5e-7
(3.4e-7, 0.21), absolute 3.6e-7 (5.6e-7, 0.23); the full table is in DESIGN.md, "YUV ingest, per pixel".
"""
import ctypes as C
import logging
import re

import numpy as np
import pytest
import torch

import yuv_channels_ref as yref

pytestmark = pytest.mark.gpu

VARIANT_RE = re.compile(r"yuv ingest: (vector|per-pixel|two-pass), FL (\d+), fl (\d+), bytes (\d), chroma_420 (\d), eotf kind (\d), "
                        r"matrix (four|nine)-term")
MODELS = ["standard_fhd", "standard_hdr_pq", "gamma2.4", "standard_hdr_linear", "absolute"]
EOTF_KIND = {"standard_fhd": 1, "gamma2.4": 2, "standard_hdr_pq": 3, "standard_hdr_linear": 4, "absolute": 5}    # FVVDP_EOTF_*
SZ = {"420": [(8, 8), (8, 248), (8, 252), (8, 500), (6, 36)], "444": [(8, 8), (8, 248), (8, 252), (8, 500), (5, 36)]}


def _case(path, H, W, bd, css, model, fps, matrix="bt709", general=False, scalar=False, padding="replicate"):
    ident = "%s-%dx%d-%dbit-%s-%s-%gfps-%s%s%s%s" % (path, H, W, bd, css, model, fps, matrix, "-general" if general else "",
                                                    "-scalar" if scalar else "", "" if padding == "replicate" else "-" + padding)
    return pytest.param(dict(path=path, H=H, W=W, bd=bd, css=css, model=model, fps=fps, matrix=matrix, general=general, scalar=scalar,
                             padding=padding), id=ident)


def _vector_cases(general):
    """Every (sample type, chroma format) pair with every display model at 30 fps (8-slot window), and with sRGB and PQ at 60 fps
    (16-slot window); sizes, bit depths and the two ITU matrices rotate through them, so that each size meets 4:2:0 and 4:4:4 and
    each of 8 / 10 / 12 / 16 bit meets both chroma formats."""
    out = []
    pairs = [(False, "420"), (False, "444"), (True, "420"), (True, "444")]
    for i, model in enumerate(MODELS):
        for j, (wide, css) in enumerate(pairs):
            H, W = SZ[css][(i + j) % 5]
            out.append(_case("vector", H, W, (10, 12, 16)[i % 3] if wide else 8, css, model, 30, ("bt709", "bt2020nc")[(i + j) % 2],
                             general=general))
    for i, model in enumerate(MODELS[:2]):
        for j, (wide, css) in enumerate(pairs):
            H, W = SZ[css][(2 + i + 2 * j) % 5]
            out.append(_case("vector", H, W, (16, 12, 10)[(i + j) % 3] if wide else 8, css, model, 60, ("bt2020nc", "bt709")[(i + j) % 2],
                             general=general))
    return out


CASES = _vector_cases(False) + _vector_cases(True) + [
    # one dense matrix (no zero, no one) through the vector and the per-pixel kernel
    _case("vector", 8, 252, 8, "420", "standard_fhd", 30, "dense"),
    _case("vector", 8, 500, 16, "444", "standard_hdr_pq", 60, "dense"),
    _case("per-pixel", 8, 250, 10, "420", "standard_fhd", 30, "dense"),
    _case("per-pixel", 200, 6, 8, "444", "gamma2.4", 30, "dense"),
    # widths that are no multiple of 4
    _case("per-pixel", 8, 250, 8, "420", "standard_fhd", 30),
    _case("per-pixel", 8, 250, 16, "444", "standard_hdr_pq", 60, "bt2020nc"),
    _case("per-pixel", 200, 6, 12, "420", "standard_hdr_linear", 30),
    _case("per-pixel", 200, 6, 8, "444", "absolute", 60),
    # FVVDP_TEMPORAL_SCALAR=1 at both window lengths
    _case("per-pixel", 8, 248, 8, "420", "standard_fhd", 30, scalar=True),
    _case("per-pixel", 8, 500, 10, "444", "standard_hdr_pq", 60, "bt2020nc", scalar=True),
    # 120 fps: 30 taps, the per-pixel kernel's 32-slot ring
    _case("per-pixel", 8, 252, 8, "420", "standard_fhd", 120),
    _case("per-pixel", 6, 36, 16, "444", "standard_hdr_pq", 120, "bt2020nc"),
    # 25 fps: 7 taps in the 8-slot window
    _case("vector", 8, 252, 10, "420", "standard_fhd", 25),
    _case("vector", 8, 8, 8, "444", "standard_hdr_pq", 25),
    # 144 / 240 fps: luminance frames first, then the 64-slot ring
    _case("two-pass", 8, 252, 8, "420", "standard_fhd", 144),
    _case("two-pass", 8, 250, 10, "444", "standard_hdr_pq", 240, "bt2020nc"),
    # the other temporal paddings
    _case("vector", 8, 500, 8, "420", "standard_fhd", 30, padding="circular"),
    _case("vector", 8, 248, 12, "444", "standard_hdr_pq", 60, padding="pingpong"),
]


def _ring(fl):
    return 8 if fl <= 8 else 16 if fl <= 16 else 32 if fl <= 32 else 64


def _expected_variant(c):
    fl = yref.orc.filter_len(c["fps"])
    four = c["path"] == "vector" and c["matrix"] != "dense" and not c["general"]
    return (c["path"], _ring(fl), fl, 1 if c["bd"] == 8 else 2, 1 if c["css"] == "420" else 0, EOTF_KIND[c["model"]],
            "four" if four else "nine")


def _product_photometry(model):
    import fovvideovdp_amd as fv
    if model == "gamma2.4":
        return fv.fvvdp_display_photo_eotf(200, contrast=1000, EOTF="gamma", gamma=2.4, E_ambient=250, k_refl=0.005)
    if model == "absolute":
        return fv.fvvdp_display_photo_absolute(10000, 0.005)
    return model


@pytest.mark.parametrize("c", CASES)
def test_yuv_ingest_per_pixel(c, monkeypatch, capfd, caplog):
    import fovvideovdp_amd as fv
    from fovvideovdp_amd import _native as nat
    H, W, bd, css, fps = c["H"], c["W"], c["bd"], c["css"], c["fps"]
    for k in ("FVVDP_YUV_GENERAL_MATRIX", "FVVDP_TEMPORAL_SCALAR"):
        monkeypatch.delenv(k, raising=False)
    if c["general"]:
        monkeypatch.setenv("FVVDP_YUV_GENERAL_MATRIX", "1")
    if c["scalar"]:
        monkeypatch.setenv("FVVDP_TEMPORAL_SCALAR", "1")
    monkeypatch.setenv("FVVDP_DEBUG_VARIANT", "1")
    m = fv.fvvdp(display_name="standard_fhd", temp_padding=c["padding"])       # (the library reads its switches when a context is created)
    fl, taps = m._temporal_taps(fps)
    r = yref.case_reference(H, W, bd, css, c["model"], fps, c["matrix"], c["padding"], taps=taps)
    N = r["N"]
    assert N == _ring(fl) + 3 and fl == r["fl"]
    if bd == 16:
        assert (r["test"] >= 32768).any() and (r["ref"] >= 32768).any()       # negative as int16: a sign extension would show
    assert r["bright_rgb_min"] > 0.05                                          # the bright frames never need the sRGB toe
    vs = fv.fvvdp_video_source_yuv_frames(r["test"].copy(), r["ref"].copy(), fps, W, H, bit_depth=bd, chroma_ss=css,
                                          color_space="bt2020nc" if c["matrix"] == "bt2020nc" else "bt709",
                                          display_photometry=_product_photometry(c["model"]))
    if c["matrix"] == "dense":
        vs.ycbcr2rgb = r["M"].tolist()
    assert np.array_equal(np.asarray(vs.ycbcr2rgb, dtype=np.float32), r["M"])
    assert np.array_equal(np.asarray(vs.color_to_luminance, dtype=np.float64), np.asarray(r["rgb2y"], dtype=np.float64))
    capfd.readouterr()
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        q, st = m.predict_video_source(vs)
    out = torch.empty((N, 4, H, W), dtype=torch.float32, device="cuda")
    nat.check(nat.lib().fvvdp_export_level(m._ctx.handle, 0, N, C.c_void_p(out.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    R = out.cpu().numpy()
    m._drop_context()
    ran = [(g[0], int(g[1]), int(g[2]), int(g[3]), int(g[4]), int(g[5]), g[6]) for g in VARIANT_RE.findall(capfd.readouterr().err)]
    assert ran == [_expected_variant(c)], (ran, _expected_variant(c))
    # YUV samples are clipped to [0,1] before the display model: the reference's out-of-range warning never fires
    assert not any("outside the valid range" in rec.message for rec in caplog.records)
    assert np.isfinite(float(q))
    e_ref = yref.channel_error(r["R32"], r["R64"], r["S64"])
    err = yref.channel_error(R, r["R64"], r["S64"])
    print("\nyuv-pixels %s %s FL %d: err %.3g e_ref %.3g bound %.3g" % (c["model"], c["path"], _ring(fl), err, e_ref, yref.error_bound(e_ref)))
    yref.assert_channels_close(R, r["R32"], r["R64"], r["S64"], label=str(c))


def test_cases_cover_every_instantiation_axis():
    """Each case asserts its own variant line, so the list itself shows what was covered: every window length, sample type, chroma
    format and display model of the vector kernel in both matrix forms, each (sample type, chroma format) pair with each display
    model, all four bit depths in both chroma formats, the per-pixel kernel at its three ring lengths, and the two-pass path."""
    v = [_expected_variant(p.values[0]) for p in CASES]
    vec = [x for x in v if x[0] == "vector"]
    for form in ("four", "nine"):
        assert {(x[1], x[3], x[4]) for x in vec if x[6] == form} == {(FL, b, c4) for FL in (8, 16) for b in (1, 2) for c4 in (0, 1)}
        assert {(x[3], x[4], x[5]) for x in vec if x[6] == form and x[1] == 8} == {(b, c4, k) for b in (1, 2) for c4 in (0, 1) for k in range(1, 6)}
        assert {(x[3], x[4], x[5]) for x in vec if x[6] == form and x[1] == 16} >= {(b, c4, k) for b in (1, 2) for c4 in (0, 1) for k in (1, 3)}
    assert {(p.values[0]["bd"], p.values[0]["css"]) for p in CASES} == {(b, s) for b in (8, 10, 12, 16) for s in ("420", "444")}
    assert {x[1] for x in v if x[0] == "per-pixel"} == {8, 16, 32}
    assert {x[3] for x in v if x[0] == "per-pixel"} == {1, 2} and {x[4] for x in v if x[0] == "per-pixel"} == {0, 1}
    assert {x[2] for x in v if x[0] == "two-pass"} == {36, 60}
    assert 7 in {x[2] for x in vec}
    sizes = {(p.values[0]["H"], p.values[0]["W"], p.values[0]["css"]) for p in CASES}
    assert sizes >= {(h, w, s) for s in SZ for (h, w) in SZ[s]} | {(8, 250, "420"), (8, 250, "444"), (200, 6, "420"), (200, 6, "444")}
