"""CPU side of the foveated one-level pixel tests (tests/test_gpu_fov_pixels.py): the helper is the yardstick the suite already
trusts, the restated plans say which loop phases each shape reaches, and the cases discriminate -- a one-row, one-column or
one-frame slip of the foveated walk moves Q of band 0 by far more than any tolerance the GPU test may use."""
import os

import numpy as np
import pytest

import fov_pixels_ref as fr
from oracle import fvvdp_oracle as orc
from fovvideovdp_amd.synth import synth_video_pair

F64 = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_helper_is_the_float64_oracle():
    """reference() on the temporal channels that predict() built returns predict()'s own Q_per_ch, and captures of the right shapes."""
    n, H, W = 4, 40, 64
    test, ref = synth_video_pair(n, H, W)
    gaze = np.float32([[10, 20], [50, 3], [63, 39], [-500, 7]])
    o = orc.Oracle("standard_4k", foveated=True, dtype=F64)
    o.capture = {}
    _, st = o.predict(test.numpy(), ref.numpy(), frames_per_second=30, fixation_point=gaze)
    R = np.stack(o.capture["R"], 0)
    assert R.shape == (n, 4, H, W) and R.dtype == F64
    got = fr.reference(orc.Oracle("standard_4k", foveated=True, dtype=F64), R, gaze)
    assert got["Q"].dtype == F64 and np.array_equal(got["Q"], st["Q_per_ch"])
    assert got["n_bands"] == st["Q_per_ch"].shape[0] and np.array_equal(got["rho_band"], st["rho_band"])
    sz = fr.level_sizes(W, H, got["n_bands"])
    for b in range(got["n_bands"]):
        w, h = sz[b]
        assert got["lbkg"][b].shape == (n, h, w) and got["contrast"][b].shape == (n, 4, h, w)
        assert got["S"][b].shape == (n, 2, h, w) and got["D"][b].shape == (n, 2, h, w)
    # the levels: the helper's reduce is the oracle's float64 reduce
    assert np.array_equal(fr.reduce64(R[0], 2), orc.gausspyr_reduce(orc.gausspyr_reduce(R[0], F64), F64))


def test_restated_plan_matches_the_host_source():
    """The constants the restatement depends on, read from the sources it restates."""
    with open(os.path.join(ROOT, "fovvideovdp_amd", "csrc", "pyramid_constants.hpp")) as f:
        assert "constexpr int STRIP_J = %d;" % fr.STRIP_J in f.read()
    with open(os.path.join(ROOT, "fovvideovdp_amd", "csrc", "pyramid_host.hpp")) as f:
        plans = f.read()
    assert "return wc <= 62 ? 1 : 1 + (wc - 62 + STRIP_J - 1) / STRIP_J;" in plans
    assert "const double cost = (double)rounds * ((double)c + 8.0) * (1.0 + 1e-4 * (double)chunks);" in plans
    with open(os.path.join(ROOT, "fovvideovdp_amd", "csrc", "fvvdp_hip.hip")) as f:
        src = f.read()
    assert "long long wave_capacity = %d;" % fr.WAVE_CAPACITY in src
    assert 'num("FVVDP_BAND_CR", 0)' in src


def test_existing_small_cases_never_leave_the_first_two_loop_phases():
    """135x240 with N = 5 ... 10 frames (and every smaller case): cr = 2 at every level -- step<0>, step<1> and the first break only."""
    ppd = orc.Oracle("standard_4k").ppd
    for n in range(1, 11):
        for (H, W) in ((135, 240), (68, 121), (120, 160), (5, 9)):
            p = fr.plan(W, H, orc.band_frequencies(W, H, ppd)[0], n)
            assert p and all(x["cr"] <= 2 for x in p), (H, W, n, p)
    assert fr.band_strips(120) == 2 and fr.band_strips(122) == 2 and fr.band_strips(123) == 3


def test_shapes_have_interior_strips_and_the_sweep_reaches_every_phase():
    assert [fr.band_strips((W + 1) // 2) for _, W in fr.SHAPES] == [3, 3, 3, 4, 5]
    ragged = 0
    for (H, W) in fr.SHAPES:
        nb = orc.band_frequencies(W, H, 75.0)[0]
        lengths = set()
        for cr in fr.CRS:
            p0 = fr.plan(W, H, nb, fr.N_FRAMES, cr)[0]
            assert p0["n_strips"] >= 3
            assert p0["cr"] == (min(cr, p0["hc"]) if cr else 2), (H, W, cr, p0)
            lengths |= set(fr.chunk_lengths(p0["hc"], p0["cr"]))
            ragged += (p0["n_strips"] * p0["n_chunks"] * fr.N_FRAMES) % 4 != 0
        assert set(x % 4 for x in lengths) == {0, 1, 2, 3} and max(lengths) >= 5, (H, W, lengths)
        lo, hi = fr.interior_columns(W)
        assert 124 == lo < hi <= W
        g = fr.gazes(fr.N_FRAMES, H, W)
        assert lo <= g[0, 0] < hi and lo <= g[3, 0] < hi                     # the gazes inside sit in interior strips
        assert tuple(g[1]) == (-0.5, -0.5) and tuple(g[4]) == (W - 0.5, H - 0.5) and g[2, 0] == W + 499
        on_centre = (g[:, 0] == np.floor(g[:, 0])) & (g[:, 1] == np.floor(g[:, 1])) & (g[:, 0] >= 0) & (g[:, 0] < W) & (g[:, 1] >= 0) & (g[:, 1] < H)
        assert not np.any(on_centre)                                         # no gaze on a pixel centre
    assert ragged >= 1                    # idle waves in the last 4-wave workgroup of some launch


def test_natural_plan_of_the_long_clip():
    """135x364 x 128 frames: tall chunks without the knob, at the capacity of an MI355X and at any smaller one."""
    nb = orc.band_frequencies(364, 135, 75.0)[0]
    p = fr.plan(364, 135, nb, 128)
    assert (p[0]["cr"], p[1]["cr"]) == (7, 3), p
    for cap in (4096, 3072, 2048, 1024, 512, 304 * 8, 64):
        q = fr.plan(364, 135, nb, 128, capacity=cap)
        assert q[0]["cr"] >= 7 and q[1]["cr"] >= 3, (cap, q)


def test_plan_line_parser():
    err = ("fvvdp: level 0: band_kernel<4, false, 1>, n 5, n_strips 4, n_chunks 6, cr 6, rw 2, lut_lds 1\n"
           "noise\nfvvdp: level 1: band_kernel<2, true, 2>, n 5, n_strips 2, n_chunks 9, cr 2, rw 9, lut_lds 0\n"
           "fvvdp: level 2: multigaze_kernel<4, 8>, n 128, n_strips 1, n_chunks 3, cr 7, rw 3, lut_lds 1, store_coarse 0\n"
           "fvvdp: levels 0+1: band2_kernel<4, true>, luminance range known [1, 2], widest plane range 3, 1 waves per workgroup, n_strips 2, "
           "kr 1, kr2 1, n_big 1, n_chunks 1, tickets off\n")
    p = fr.parse_plans(err)
    assert len(p) == 3
    assert p[0] == dict(level=0, kernel="band", P=4, dbg=False, fovm=1, n=5, n_strips=4, n_chunks=6, cr=6, rw=2, lut_lds=1)
    assert p[1]["dbg"] and p[1]["fovm"] == 2 and p[1]["rw"] == 9 and p[1]["lut_lds"] == 0
    assert p[2] == dict(level=2, kernel="multigaze", P=4, ng=8, n=128, n_strips=1, n_chunks=3, cr=7, rw=3, lut_lds=1, store_coarse=0)


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("H,W", fr.SHAPES)
@pytest.mark.parametrize("display", sorted(fr.DISPLAYS))
def test_cases_discriminate(display, H, W, P):
    """Band 0, every channel: |dQ| / Q >= 5e-3 under a gaze moved by one row, by one column, and a trace moved by one frame."""
    R, fp, ref = fr.case(display, H, W, P)
    d = fr.discrimination(display, H, W, P)
    tc = P // 2
    print("\n%s %dx%d P=%d: band 0 row %s col %s frame %s, mean |dS|/S under one row %s" %
          (display, H, W, P, d["row"][0], d["col"][0], d["frame"][0], d["S_row"][0]))
    for k in ("row", "col", "frame"):
        assert d[k].shape == (ref["n_bands"], tc)
        assert np.all(d[k][0] >= 5e-3), (k, d[k][0])
    assert np.all(ref["Q"][:, :tc] > 0) and np.all(ref["Q"][:, tc:] == 0)
    # D is neither 0 nor at its ceiling (d_max = 1e4) but for a handful of pixels
    for b in range(ref["n_bands"]):
        D = ref["D"][b]
        assert np.all(D > 0) and np.mean(D >= 0.999e4) < 1e-3, (b, float(D.min()), float(np.mean(D >= 0.999e4)))


@pytest.mark.parametrize("H,W", fr.SHAPES)
def test_pooled_mass_reaches_interior_strips_in_the_late_phases(H, W):
    """Q is a pooled value: it sees a wrong pixel only where D^beta has mass.  On standard_4k that mass sits within a few dozen pixels
    of the gaze (beyond, the sensitivity is on the floor of the CSF table).  Over the sweep of chunk heights, for each of the loop
    phases 2 and 3, some frame of band 0 has at least a fifth of its pooled mass in pixels that an interior strip computes in that
    phase."""
    R, fp, ref = fr.case("4k", H, W, 4)
    beta = orc.load_defaults()["fvvdp_parameters.json"]["beta"]
    lo, hi = fr.interior_columns(W)
    best = {2: 0.0, 3: 0.0}
    hc = (H + 1) // 2
    for cr in fr.CRS:
        ph = fr.row_phases(H, min(cr, hc) if cr else 2)
        for f in range(fr.N_FRAMES):
            for cc in range(2):
                M = ref["D"][0][f, cc] ** beta
                for k in best:
                    best[k] = max(best[k], float(M[ph == k, lo:hi].sum() / M.sum()))
    print("\n%dx%d: largest share of a frame's band-0 mass in interior strips, phase 2: %.2f, phase 3: %.2f" % (H, W, best[2], best[3]))
    assert best[2] >= 0.2 and best[3] >= 0.2, best
