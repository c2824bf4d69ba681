"""fvvdp_param_sums alone (include/fvvdp_hip_params.h), through the C ABI: the five sums per (band, temporal channel, slot) over
the maps of a real map-writing pass against float64 numpy on those same fp32 maps.

68 x 121: every level has an odd row length (121, 61, 31, 16, 8), level 0 spans three workgroups with a partial last one, levels
1 and 2 take the one-pixel path (2074 and 527 pixels), the last bands are smaller than a wave.  64 x 128: every level takes the
16-byte path.  The content (param_grad_ref.planar_content) has a half where test == reference (D = 0), a patch where the
reference contrast is exactly 0 under a faint test (M = 0 with D > 0) and a full-contrast patch (pixels at the d_max clamp)."""
import ctypes as C

import numpy as np
import pytest
import torch

import param_grad_ref as ref
from lowlevel import Pipeline

pytestmark = pytest.mark.gpu

# Worst |kernel - float64| over every sum, band, channel, slot and case, relative to the sum of the absolute pixel terms of that
# sum, measured on an MI355X: SUMS_MEASURED (7.7e-7 and 7.1e-7 for P = 2, 1.35e-6 and 1.23e-6 for P = 4).  The bound is 3 x that (the convention of test_gpu_video_grad_input.py).  The error
# is that of the fp32 pixel terms: v_log_f32 / v_exp_f32 (1 ulp) under an exponent |beta lg D| of up to 20.
SUMS_MEASURED = 1.35e-6
SUMS_BOUND = 3 * SUMS_MEASURED
D_HI = 1e4 * (1.0 - 2.0 ** -20)            # a stored D within 2^-20 of d_max counts as clamped (fvvdp_hip_params.h)


@pytest.fixture(scope="module")
def metric():
    import fovvideovdp_amd as fv
    from fovvideovdp_amd import _native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _native.lib()
    return fv.fvvdp(display_name="standard_4k", device=torch.device("cuda:0"), quiet=True)


def run_sums(metric, pipe, maps, n, P):
    from fovvideovdp_amd import _native as nat
    lib = nat.lib()
    nb = pipe.n_bands
    maps_arr = (nat.BandMaps * nb)()
    for b in range(nb):
        maps_arr[b].d_D, maps_arr[b].d_contrast = maps[b]["D"].data_ptr(), maps[b]["contrast"].data_ptr()
        maps_arr[b].d_lbkg, maps_arr[b].d_S = maps[b]["lbkg"].data_ptr(), maps[b]["S"].data_ptr()
    nbytes = C.c_size_t(0)
    nat.check(lib.fvvdp_param_sums_workspace(pipe.W, pipe.H, nb, n, C.byref(nbytes)))
    work = torch.full(((nbytes.value + 7) // 8,), float("nan"), dtype=torch.float64, device=metric.device)
    out = torch.full((nb, 2, n, 5), float("nan"), dtype=torch.float64, device=metric.device)
    prm = metric.native_params()
    nat.check(lib.fvvdp_param_sums(pipe.W, pipe.H, nb, n, P, C.byref(prm), maps_arr, C.c_void_p(out.data_ptr()),
                                   C.c_void_p(work.data_ptr()), nbytes.value, pipe.stream()))
    return out.cpu().numpy()


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("size", [(68, 121), (64, 128)])
def test_sums_against_float64_on_the_same_maps(metric, size, P):
    H, W = size
    prm = metric.native_params()
    names = ref.NAMES
    vals = dict(zip(names, [float(v) for v in metric.parameter_tensor()]))
    results = {}
    with torch.cuda.device(metric.device):
        pipe = Pipeline(metric, W, H, P, 3)
        try:
            for n in (1, 3):
                # slot 0 and slot 2 of the batch of three hold the content of the single slot
                seeds = [1] if n == 1 else [1, 2, 1]
                R = torch.from_numpy(np.stack([ref.planar_content(H, W, P, s) for s in seeds])).to(metric.device)
                pipe.load_planar(R)
                Q, maps = pipe.bands_forward(n, want_maps=True)
                a = run_sums(metric, pipe, maps, n, P)
                b = run_sums(metric, pipe, maps, n, P)
                assert np.isfinite(a).all()
                assert a.tobytes() == b.tobytes()                      # run to run
                results[n] = (a, [{k: v.cpu().numpy() for k, v in m.items()} for m in maps])
        finally:
            pipe.close()
    a1, a3 = results[1][0], results[3][0]
    assert a1[:, :, 0].tobytes() == a3[:, :, 0].tobytes()              # the batch
    assert a3[:, :, 0].tobytes() == a3[:, :, 2].tobytes()              # the slot
    assert a3[:, :, 0].tobytes() != a3[:, :, 1].tobytes()
    if P == 2:
        assert (a3[:, 1] == 0).all()

    a, maps = results[3]
    worst, where, seen = 0.0, None, dict(zero=0, clamped=0, unmasked=0)
    for b, m in enumerate(maps):
        for cc in range(P // 2):
            for k in range(3):
                D, S = m["D"][k, cc], m["S"][k, cc]
                T, Rr = m["contrast"][k, 2 * cc], m["contrast"][k, 2 * cc + 1]
                want, scale = ref.sums_from_maps(D, T, Rr, S, vals, cc, d_hi=D_HI, gain=prm.sens_gain, k_mask=prm.mask_k)
                Tp, Rp = T.astype(np.float64) * S * prm.sens_gain, Rr.astype(np.float64) * S * prm.sens_gain
                M = prm.mask_k * np.minimum(np.abs(Tp), np.abs(Rp))
                seen["zero"] += int((D == 0).sum())
                seen["clamped"] += int((D >= D_HI).sum())
                seen["unmasked"] += int(((M == 0) & (D > 0) & (D < D_HI)).sum())
                for j in range(5):
                    if scale[j] == 0:
                        assert a[b, cc, k, j] == 0, (b, cc, k, j)
                        continue
                    err = abs(a[b, cc, k, j] - want[j]) / scale[j]
                    if err > worst:
                        worst, where = err, (b, cc, k, j, a[b, cc, k, j], want[j], scale[j])
    print("param sums %dx%d P=%d: worst relative error %.3e at %s; pixels with D = 0: %d, clamped: %d, M = 0 and live: %d"
          % (W, H, P, worst, where, seen["zero"], seen["clamped"], seen["unmasked"]))
    assert seen["zero"] > 0 and seen["clamped"] > 0 and seen["unmasked"] > 0
    assert worst <= SUMS_BOUND, where
