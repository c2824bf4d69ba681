"""GPU: the foveated one-level pass (band_kernel<P, DBG, 1 | 2 | 3>) and multigaze_kernel<P, NG> with three and more strips and tall
chunks -- the later phases of the unrolled row ring (step<2>, step<3>, the back edge), strips that are neither first nor last, and the
frame-fastest work order with idle waves in the last workgroup.  The small foveated, gaze and user-geometry tests elsewhere all plan
cr = 2 and at most two strips (tests/test_fov_pixels_cpu.py); here FVVDP_BAND_CR sets the chunk height and every test reads the plan
that ran from the FVVDP_DEBUG_VARIANT lines.

a. the map-writing variant against the float64 oracle, per pixel: L_bkg, contrast, S, D of every band;
b. the pooling variants: Q[band, channel, frame] against the float64 oracle, the Gaussian levels per pixel against the float64
   reduce of level 0 and bit for bit across chunk heights and variants;
c. predict_gazes against the loop of predict calls, bit for bit.

Inputs, gazes, the float64 yardstick and the plan restatement: tests/fov_pixels_ref.py.  Measured figures are printed and kept as JSON files
(_record)."""
import numpy as np
import pytest
import torch

import fov_pixels_ref as fr

pytestmark = pytest.mark.gpu

F64 = np.float64
N = fr.N_FRAMES
LEVEL_TOL = 9e-7                  # float64 reduce of level 0 against an exported level (tests/test_gpu_band2_pixels.py)
Q_CAP = 1e-3                      # no Q tolerance above this, and none at band 0 above a fifth of the case's sensitivity


def _record(tag, obj):
    """measured figures next to the asserts: printed, and kept as JSON where test_gpu_fullsize_maps.py keeps its own"""
    from test_gpu_fullsize_maps import _record as keep
    keep("fov_pixels_" + tag, obj)


def _env(monkeypatch, cr):
    for k in ("FVVDP_BAND_CR", "FVVDP_GAZE_GROUP", "FVVDP_BAND_FUSE", "FVVDP_BAND_INRANGE"):
        monkeypatch.delenv(k, raising=False)
    if cr is not None:
        monkeypatch.setenv("FVVDP_BAND_CR", str(cr))
    monkeypatch.setenv("FVVDP_DEBUG_VARIANT", "1")


_metrics = {}


def _metric(display, H, W):
    """The metric of a display key of fov_pixels_ref.DISPLAYS (the knobs are read when a native context is created, not here)."""
    import fovvideovdp_amd as fv
    key = (display, H, W) if display == "custom" else display
    if key not in _metrics:
        if display == "custom":
            class MyGeom(fv.fvvdp_display_geometry):         # the twin of fov_pixels_ref.CustomGeometry
                def get_ppd(self, view_dir=None):
                    if view_dir is None:
                        return self.ppd_centre
                    view_angle = torch.sqrt(torch.sum(view_dir ** 2, dim=0, keepdim=False))
                    return self.ppd_centre / (view_angle / 20. + 1.)
            _metrics[key] = fv.fvvdp(display_name="standard_hmd", display_geometry=MyGeom((W, H), **fr.CUSTOM_GEOM), foveated=True)
        else:
            _metrics[key] = fv.fvvdp(display_name={"4k": "standard_4k", "hmd": "standard_hmd"}[display], foveated=True)
    return _metrics[key]


def _run(monkeypatch, capfd, display, H, W, P, cr, want_maps):
    """One pass of the case under FVVDP_BAND_CR = cr.  Returns (Q [bands,2,N] numpy, maps or None, {level: [N,P,h,w]}, plans)."""
    from lowlevel import Pipeline
    R, fp, ref = fr.case(display, H, W, P)
    _env(monkeypatch, cr)
    m = _metric(display, H, W)
    capfd.readouterr()
    pipe = Pipeline(m, W, H, P, N, foveated=True)
    try:
        assert pipe.n_bands == ref["n_bands"]
        if display == "custom":
            pipe.set_view_maps()
        pipe.load_planar(torch.tensor(R, device=m.device))
        out = pipe.bands_forward(N, want_maps=want_maps, fixation=fp)
        Q, maps = out if want_maps else (out, None)
        levels = {lv: pipe.export_level(lv, N).cpu().numpy() for lv in range(1, pipe.n_bands + 1)}
        Q = Q.cpu().numpy()
        if maps is not None:
            maps = [{k: v.cpu().numpy() for k, v in d.items()} for d in maps]
        torch.cuda.synchronize()
    finally:
        pipe.close()
    plans = fr.parse_plans(capfd.readouterr().err)
    return Q, maps, levels, plans


def _check_plans(plans, H, W, P, cr, n_bands, dbg, fovm, sweep):
    """Which kernel ran at every level, three or more strips at level 0, the chunk height asked for; adds to the sweep's record."""
    assert [p["level"] for p in plans] == list(range(n_bands)), plans
    want = fr.plan(W, H, n_bands, N, cr)
    for p, q in zip(plans, want):
        assert p["kernel"] == "band" and p["P"] == P and p["dbg"] == dbg and p["fovm"] == fovm and p["n"] == N, p
        assert (p["n_strips"], p["n_chunks"], p["cr"]) == (q["n_strips"], q["n_chunks"], q["cr"]), (p, q)
        assert p["lut_lds"] == int(p["rw"] <= 3) and (dbg or p["lut_lds"] == int(fovm in (1, 3))), p     # the slice fits the LDS or not
        sweep["ragged"] |= (p["n_strips"] * p["n_chunks"] * N) % 4 != 0
    assert plans[0]["n_strips"] >= 3
    if cr is not None:
        assert plans[0]["cr"] == cr, plans[0]
    sweep["lengths"] |= set(fr.chunk_lengths((H + 1) // 2, plans[0]["cr"]))


def _check_sweep(sweep):
    """Over the sweep: chunks of every length mod 4 (each exit of the unrolled loop), one that takes the back edge, idle waves."""
    assert set(x % 4 for x in sweep["lengths"]) == {0, 1, 2, 3} and max(sweep["lengths"]) >= 5, sweep
    assert sweep["ragged"], sweep


_levels_seen = {}


def _check_levels(levels, H, W, P, tag):
    """Every exported level: per pixel against the float64 reduce of level 0, and bit-identical to the first pass of this input
    (whatever the chunk height or the variant that wrote it).  Returns the worst relative error."""
    R = fr.case("4k", H, W, P)[0]                 # the planes depend on the shape alone
    key = (H, W, P)
    if key not in _levels_seen:
        want = {}
        for f in range(N):
            y = R[f]
            for lv in sorted(levels):
                y = fr.reduce64(y)
                want.setdefault(lv, []).append(y)
        _levels_seen[key] = ({lv: np.stack(v, 0) for lv, v in want.items()}, {lv: a.copy() for lv, a in levels.items()})
    want, first = _levels_seen[key]
    worst = 0.0
    for lv, a in levels.items():
        assert a.shape == want[lv].shape
        e = float(np.max(np.abs(a.astype(F64) - want[lv]) / np.abs(want[lv])))
        worst = max(worst, e)
        assert e <= LEVEL_TOL, (tag, lv, e)
        assert np.array_equal(a, first[lv]), (tag, lv)
    return worst


def _rel(h, g, floor=0.0):
    return np.abs(h.astype(F64) - g) / (np.abs(g) + floor)


CASES = [(d, H, W, P) for d in sorted(fr.DISPLAYS) for (H, W) in fr.SHAPES for P in (2, 4)]

# ------------------------------------------------------------------------------------------------------------------------------
# a. band_kernel<P, true, 2>: the maps per pixel
# ------------------------------------------------------------------------------------------------------------------------------
# Tolerances per band (finest first): 3x the worst value measured on MI355X over all shapes and both P, the measured values in
# the comments.  lbkg, contrast, D: largest per-pixel error; S: largest and mean per-pixel error.  contrast is relative to |c| + the
# band's mean |c| (it crosses zero), D to D + 1e-6 of the map's largest value.  The errors of contrast and D grow with the level: the
# planes are independent noise, whose Laplacian shrinks level by level while the fp32 rounding of g - expand(G) stays where it was,
# and D ~ |T - R|^2.4 carries the cancellation of two such contrasts.
_LBKG = [1.0e-6] * 5                                                          # measured 3.0e-7 3.3e-7 3.2e-7 3.6e-7 3.1e-7 (any display)
_CONTRAST = [2.4e-6, 8.4e-6, 1.9e-5, 3.0e-5, 3.8e-5]                          # measured 8.1e-7 2.8e-6 6.4e-6 1.0e-5 1.3e-5 (any display)
MAP_TOL = {
    "4k": dict(lbkg=_LBKG, contrast=_CONTRAST,
               S_max=[4.3e-5, 3.0e-5, 2.2e-5, 2.7e-6, 2.6e-6],                # measured 1.44e-5 1.0e-5 7.6e-6 9.1e-7 8.9e-7
               S_mean=[5.4e-7, 2.0e-6, 1.3e-6, 6.0e-7, 6.3e-7],               # measured 1.8e-7 7.0e-7 4.5e-7 2.0e-7 2.1e-7
               D=[1.5e-3, 6.6e-3, 1.5e-2, 3.6e-2, 6.1e-2]),                   # measured 5.1e-4 2.2e-3 5.3e-3 1.2e-2 2.06e-2
    "hmd": dict(lbkg=_LBKG, contrast=_CONTRAST,
                S_max=[6.8e-5, 4.8e-5, 6.3e-6, 4.2e-6, 3.3e-6],               # measured 2.27e-5 1.6e-5 2.1e-6 1.4e-6 1.1e-6
                S_mean=[3.0e-6, 1.3e-6, 9.3e-7, 8.1e-7, 7.5e-7],              # measured 1.0e-6 4.4e-7 3.1e-7 2.7e-7 2.5e-7
                D=[1.5e-3, 6.0e-3, 1.2e-2, 2.4e-2, 4.1e-2]),                  # measured 5.1e-4 2.0e-3 4.2e-3 8.1e-3 1.38e-2
    "custom": dict(lbkg=_LBKG, contrast=_CONTRAST,
                   S_max=[2.7e-5, 3.3e-6, 3.9e-6, 3.9e-6, 4.2e-6],            # measured 9.14e-6 1.1e-6 1.3e-6 1.3e-6 1.4e-6
                   S_mean=[1.1e-6, 7.8e-7, 7.2e-7, 9.0e-7, 9.0e-7],           # measured 3.97e-7 2.6e-7 2.4e-7 3.0e-7 3.0e-7
                   D=[1.4e-3, 5.7e-3, 1.3e-2, 2.1e-2, 6.0e-2]),               # measured 4.9e-4 1.9e-3 4.4e-3 7.1e-3 2.05e-2
}


@pytest.mark.parametrize("display,H,W,P", CASES)
def test_maps_per_pixel(monkeypatch, capfd, display, H, W, P):
    R, fp, ref = fr.case(display, H, W, P)
    nb, tc = ref["n_bands"], P // 2
    sens = fr.discrimination(display, H, W, P)
    sweep = dict(lengths=set(), ragged=False)
    first, got = None, {}
    for cr in fr.CRS:
        Q, maps, levels, plans = _run(monkeypatch, capfd, display, H, W, P, cr, True)
        _check_plans(plans, H, W, P, cr, nb, True, 2, sweep)
        _check_levels(levels, H, W, P, (display, cr))
        if first is None:
            first = maps
            for b in range(nb):
                lb, cn = ref["lbkg"][b], ref["contrast"][b]
                S, D = ref["S"][b], ref["D"][b]
                rs = _rel(maps[b]["S"][:, :tc], S)
                got[b] = dict(lbkg=float(_rel(maps[b]["lbkg"], lb).max()),
                              contrast=float(_rel(maps[b]["contrast"], cn, np.mean(np.abs(cn))).max()),
                              S_max=float(rs.max()), S_mean=float(rs.mean(axis=(0, 2, 3)).max()),
                              D=float(_rel(maps[b]["D"][:, :tc], D, 1e-6 * D.max(axis=(2, 3), keepdims=True)).max()))
                if tc == 1:                       # images: the second channel's maps are not written
                    assert not maps[b]["S"][:, 1].any() and not maps[b]["D"][:, 1].any()
        else:
            for b in range(nb):                   # cr decides who computes a pixel, not how
                for k in ("lbkg", "contrast", "S", "D"):
                    ne = maps[b][k] != first[b][k]
                    assert not ne.any(), (cr, b, k, int(ne.sum()), "rows", np.unique(np.nonzero(ne)[-2])[:16])
    _check_sweep(sweep)
    _record("maps_%s_%dx%d_P%d" % (display, H, W, P), dict(bands=got, S_row=[[float(v) for v in row] for row in sens["S_row"]]))
    tol = MAP_TOL[display]
    # a fifth of what the oracle's own S of band 0 moves by, on average, under a one-row shift of the gaze
    assert tol["S_mean"][0] <= np.min(sens["S_row"][0]) / 5, sens["S_row"][0]       # smallest S_row of band 0 over the cases: 1.0e-3
    for b in range(nb):
        for k, v in got[b].items():
            assert v <= tol[k][b], (b, k, v, tol[k][b])


# ------------------------------------------------------------------------------------------------------------------------------
# b. the pooling variants band_kernel<P, false, 1 | 2 | 3>
# ------------------------------------------------------------------------------------------------------------------------------
# Q tolerances per variant and band (finest first), |Q - Q64| / Q64 over every frame, channel, shape and chunk height: 3x measured on
# MI355X.  All under Q_CAP; at band 0 the smallest one-row / one-column / one-frame sensitivity of a case is 0.26 (4k), 1.2e-2 (hmd)
# and 6.8e-3 (custom), a fifth of which is 40 times the tolerance or more.  The exported levels: worst 2.98e-7 against LEVEL_TOL.
Q_TOL = {
    "4k": [3.5e-5, 1.8e-5, 5.8e-5, 1.2e-4, 1.1e-4],           # band_kernel<P, false, 1>; measured 1.17e-5 6.08e-6 1.96e-5 4.24e-5 3.94e-5
    "hmd": [9.7e-6, 2.1e-5, 4.5e-5, 2.5e-4, 1.8e-4],          # band_kernel<P, false, 2>; measured 3.25e-6 7.22e-6 1.50e-5 8.39e-5 6.04e-5
    "custom": [4.0e-6, 1.5e-5, 1.2e-4, 1.2e-4, 4.0e-4],       # band_kernel<P, false, 3>; measured 1.36e-6 5.11e-6 4.15e-5 4.26e-5 1.34e-4
}


@pytest.mark.parametrize("display,H,W,P", CASES)
def test_pooled_q_and_levels(monkeypatch, capfd, display, H, W, P):
    R, fp, ref = fr.case(display, H, W, P)
    nb, tc = ref["n_bands"], P // 2
    sens = fr.discrimination(display, H, W, P)
    floor0 = float(min(np.min(sens[k][0]) for k in ("row", "col", "frame")))
    sweep = dict(lengths=set(), ragged=False)
    worst, worst_lv = np.zeros(nb), 0.0
    for cr in fr.CRS:
        Q, _, levels, plans = _run(monkeypatch, capfd, display, H, W, P, cr, False)
        _check_plans(plans, H, W, P, cr, nb, False, fr.DISPLAYS[display], sweep)
        worst_lv = max(worst_lv, _check_levels(levels, H, W, P, (display, cr)))
        e = _rel(Q[:, :tc], ref["Q"][:, :tc])
        assert not Q[:, tc:].any()
        worst = np.maximum(worst, e.max(axis=(1, 2)))
    _check_sweep(sweep)
    _record("q_%s_%dx%d_P%d" % (display, H, W, P), dict(Q=[float(v) for v in worst], levels=worst_lv, sensitivity_band0=floor0))
    tol = Q_TOL[display]
    assert all(t <= Q_CAP for t in tol) and tol[0] <= floor0 / 5, (tol, floor0)
    for b in range(nb):
        assert worst[b] <= tol[b], (b, worst[b], tol[b])


# ------------------------------------------------------------------------------------------------------------------------------
# c. many gazes
# ------------------------------------------------------------------------------------------------------------------------------
GROUPS = {1: [1], 7: [4, 2, 1], 9: [8, 1]}


def _traces(G, n, H, W):
    """[G, n, 2]: the case's gaze trace, rolled by g frames and moved by 7 g pixels."""
    base = fr.gazes(n, H, W) if n == N else np.resize(fr.gazes(N, H, W), (n, 2))
    return np.ascontiguousarray(np.stack([np.roll(base, g, axis=0) + np.float32([7 * g, -3 * g]) for g in range(G)]).astype(np.float32))


def _gaze_lines(plans, P, G, lut_lds_levels, n):
    """The launches of one predict_gazes call: per level the groups 8 / 4 / 2 / 1 with only the first storing the next level, or,
    where the slice does not fit the LDS, band_kernel<P, false, 2> once per gaze."""
    by = {}
    for p in plans:
        by.setdefault(p["level"], []).append(p)
    for lv, ps in by.items():
        assert all(p["P"] == P and p["n"] == n for p in ps)
        if lv in lut_lds_levels:
            assert [p["kernel"] for p in ps] == ["multigaze"] * len(GROUPS[G]) and [p["ng"] for p in ps] == GROUPS[G], ps
            assert [p["store_coarse"] for p in ps] == [1] + [0] * (len(ps) - 1), ps
        else:
            assert len(ps) == G and all(p["kernel"] == "band" and p["fovm"] == 2 and not p["dbg"] for p in ps), ps
    return by


@pytest.mark.parametrize("display", ["standard_4k", "standard_hmd"])
@pytest.mark.parametrize("H,W", [(67, 365), (46, 246)])
def test_gazes_bit_identical_to_predict_loop(monkeypatch, capfd, display, H, W):
    import fovvideovdp_amd as fv
    from fovvideovdp_amd.synth import synth_video_pair
    t, r = synth_video_pair(N, H, W, pair=7)
    t, r = t.cuda(), r.cuda()
    fp = _traces(9, N, H, W)
    sweep = dict(lengths=set(), ragged=False)
    for cr in fr.CRS:
        _env(monkeypatch, cr)
        m_loop = fv.fvvdp(display_name=display, foveated=True)
        m_gaze = fv.fvvdp(display_name=display, foveated=True)
        capfd.readouterr()
        jod, Q = [], []
        for g in range(9):
            q, st = m_loop.predict(t, r, frames_per_second=30, fixation_point=fp[g])
            jod.append(q.clone())
            Q.append(st["Q_per_ch"].copy())
        jod, Q = torch.stack(jod), np.stack(Q)
        nb = Q.shape[1]
        loop = fr.parse_plans(capfd.readouterr().err)
        assert len(loop) == 9 * nb and all(p["kernel"] == "band" and p["fovm"] == (1 if display == "standard_4k" else 2) for p in loop)
        assert len(set(float(v) for v in jod)) >= 2
        want = fr.plan(W, H, nb, N, cr)
        for G in (1, 7, 9):
            q, st = m_gaze.predict_gazes(t, r, fp[:G], frames_per_second=30)
            plans = fr.parse_plans(capfd.readouterr().err)
            assert np.array_equal(st["Q_per_ch"], Q[:G]) and torch.equal(q, jod[:G]), (cr, G)
            by = _gaze_lines(plans, 4, G, range(nb) if display == "standard_4k" else (), N)
            assert sorted(by) == list(range(nb))
            for lv, ps in by.items():
                for p in ps:
                    assert (p["n_strips"], p["n_chunks"], p["cr"]) == (want[lv]["n_strips"], want[lv]["n_chunks"], want[lv]["cr"]), (p, want[lv])
                    sweep["ragged"] |= (p["n_strips"] * p["n_chunks"] * N) % 4 != 0
            assert by[0][0]["n_strips"] >= 3 and (cr is None or by[0][0]["cr"] == cr)
            sweep["lengths"] |= set(fr.chunk_lengths((H + 1) // 2, by[0][0]["cr"]))
        m_loop._drop_context()
        m_gaze._drop_context()
    _check_sweep(sweep)


def test_gazes_natural_plan_of_a_long_clip(monkeypatch, capfd):
    """128 gray frames of 135x364 in one batch: chunking() itself picks tall chunks (7 and 3 coarse rows at levels 0 and 1 with 4096
    resident waves, taller with fewer) -- the later loop phases of multigaze_kernel and of band_kernel<4, false, 1> without the knob."""
    import fovvideovdp_amd as fv
    _env(monkeypatch, None)
    n, H, W, G = 128, 135, 364, 9
    rng = np.random.RandomState(364)
    r = rng.randint(0, 256, (n, H, W)).astype(np.uint8)
    t = np.clip(r.astype(np.int32) + rng.randint(-12, 13, (n, H, W)), 0, 255).astype(np.uint8)
    t, r = torch.from_numpy(t).cuda(), torch.from_numpy(r).cuda()
    fp = _traces(G, n, H, W)
    m = fv.fvvdp(display_name="standard_4k", foveated=True)
    capfd.readouterr()
    q, st = m.predict_gazes(t, r, fp, dim_order="FHW", frames_per_second=30)
    plans = fr.parse_plans(capfd.readouterr().err)
    nb = st["Q_per_ch"].shape[1]
    by = _gaze_lines(plans, 4, G, range(nb), n)
    print("\nplans", [(lv, ps[0]["n_strips"], ps[0]["n_chunks"], ps[0]["cr"]) for lv, ps in sorted(by.items())])
    assert by[0][0]["n_strips"] >= 3 and by[0][0]["cr"] >= 5 and by[1][0]["cr"] >= 3, (by[0][0], by[1][0])
    m2 = fv.fvvdp(display_name="standard_4k", foveated=True)
    for g in range(G):
        q1, st1 = m2.predict(t, r, dim_order="FHW", frames_per_second=30, fixation_point=fp[g])
        assert torch.equal(q[g], q1) and np.array_equal(st["Q_per_ch"][g], st1["Q_per_ch"]), g
    loop = fr.parse_plans(capfd.readouterr().err)
    assert all(p["kernel"] == "band" and p["fovm"] == 1 for p in loop) and loop[0]["cr"] == by[0][0]["cr"] and loop[1]["cr"] == by[1][0]["cr"]
    assert len(set(float(v) for v in q)) >= 2
