"""Calibration: fvvdp.calibration_jod_video forward + backward (the gradient with respect to the twelve model parameters) against
fvvdp.predict (sync=False) and fvvdp.jod_video forward + backward, alternated in one process on the same resident float clip and
timed with HIP events around work that ends in an event synchronise; and fvvdp_param_sums alone on the maps of one backward batch,
against the bytes it reads (include/fvvdp_hip_params.h: 8 fp32 planes per band pixel of a video frame, nothing written per pixel).
Prints one JSON line per case: median ms per call with min .. max, the ratios, and the reduction kernel's rate.

    python tools/bench_calibration.py                       # 1920x1080x60 RGB at 30 fps
    python tools/bench_calibration.py --case 30x2160x3840
    python tools/bench_calibration.py --temporal            # also the gradients for sustained_sigma / sustained_beta

--temporal adds calibration_jod_video(temporal=phi) forward + backward with phi alone and with theta and phi requiring grad to the
alternation, and fvvdp_tap_grad alone at 8 and 15 taps against its bytes model (include/fvvdp_hip_taps.h: per tap group of 8, 16 B
of level-0 gradients and 8 B of luminance per pixel and frame).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # MI355X HBM3E, bytes/s
CASES = {"60x1080x1920": (60, 1080, 1920), "30x2160x3840": (30, 2160, 3840)}


def run_case(key, a):
    import fovvideovdp_amd as fv
    from fovvideovdp_amd import _native as nat
    from fovvideovdp_amd import param_grad as pg
    from fovvideovdp_amd.fvvdp import filter_length
    N, H, W = CASES[key]
    Cc = 3
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    ref = torch.rand((1, Cc, N, H, W), device=dev, generator=g)
    test = (ref + 0.05 * torch.randn((1, Cc, N, H, W), device=dev, generator=g)).clamp(0, 1)
    m = fv.fvvdp(display_name=a.display, device=dev, quiet=True)
    stream = torch.cuda.current_stream(dev)
    theta = m.parameter_tensor()

    def fwd():
        m.predict(test, ref, frames_per_second=a.fps, sync=False)

    def calib_fwd():
        m.calibration_jod_video(test, ref, theta, frames_per_second=a.fps)

    def calib():
        th = theta.clone().requires_grad_(True)
        m.calibration_jod_video(test, ref, th, frames_per_second=a.fps).backward()

    def video_grad():
        x = test.detach().requires_grad_(True)
        m.jod_video(x, ref, frames_per_second=a.fps).backward()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    phi0 = m.temporal_parameter_tensor()

    def calib_phi():
        phi = phi0.clone().requires_grad_(True)
        m.calibration_jod_video(test, ref, theta, frames_per_second=a.fps, temporal=phi).backward()

    def calib_both():
        th, phi = theta.clone().requires_grad_(True), phi0.clone().requires_grad_(True)
        m.calibration_jod_video(test, ref, th, frames_per_second=a.fps, temporal=phi).backward()

    fns = (fwd, calib_fwd, calib, video_grad) + ((calib_phi, calib_both) if a.temporal else ())
    for _ in range(a.warmup):
        for fn in fns:
            timed(fn)
    t = [[] for _ in fns]
    for _ in range(a.steps):
        for i, fn in enumerate(fns):
            t[i].append(timed(fn))
    med = [float(np.median(x)) for x in t]

    # the reduction kernel alone, on the maps of one backward batch written by a real pass
    fl = filter_length(a.fps)
    n_bands, rho_band = m._band_count(W, H)
    batch = m._batch_size(W, H, 4, N, fl)
    gb = pg.grad_batch_size(m, W, H, n_bands, batch, 9)
    vs = fv.fvvdp_video_source_array(test, ref, a.fps, dim_order="BCFHW", display_photometry=m.display_photometry,
                                     color_space_name=m.color_space)
    with torch.cuda.device(dev):
        pl = m._clip_plan(vs)
        ctx = m._context(W, H, n_bands, 4, pl.batch, rho_band)
        sums = pg._Sums(m, W, H, n_bands, 4, gb, gb)
        st = C.c_void_p(stream.cuda_stream)
        idx = np.ascontiguousarray(pl.widx[:fl - 1 + gb])
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        pl.feeder(ctx, idx, pl.taps, fl, gb, flag, st)
        nat.check(nat.lib().fvvdp_bands_forward(ctx.handle, gb, C.c_void_p(sums.q_scratch.data_ptr()), gb, 0, None, None,
                                                sums.maps_arr, st))
        prm = m.native_params()
        ts = []
        for i in range(a.warmup + a.steps):
            ms = timed(lambda: sums.reduce(prm, 0, gb, st))
            if i >= a.warmup:
                ts.append(ms)
    band_px = sum(w * h for w, h in m._level_sizes(W, H, n_bands)[:n_bands])
    nbytes = gb * band_px * 32
    ms_k = float(np.median(ts))
    out = {"case": key, "frames": N, "height": H, "width": W, "channels": Cc, "fps": a.fps, "display": a.display,
           "n_bands": n_bands, "grad_batch": gb,
           "predict_ms": round(med[0], 3), "calibration_forward_ms": round(med[1], 3), "calibration_fwd_bwd_ms": round(med[2], 3),
           "jod_video_fwd_bwd_ms": round(med[3], 3),
           "spread_ms": [[round(min(x), 3), round(max(x), 3)] for x in t],
           "calibration_over_predict": round(med[2] / med[0], 2), "calibration_over_jod_video": round(med[2] / med[3], 2),
           "param_sums": {"frames": gb, "bytes_read": nbytes, "ms": round(ms_k, 4), "spread_ms": [round(min(ts), 4), round(max(ts), 4)],
                          "tb_per_s": round(nbytes / (ms_k * 1e-3) / 1e12, 2),
                          "hbm_peak_share": round(nbytes / (ms_k * 1e-3) / HBM_PEAK, 3),
                          "ms_per_clip": round(ms_k * N / gb, 3)}}
    if a.temporal:
        out["calibration_phi_fwd_bwd_ms"] = round(med[4], 3)
        out["calibration_theta_phi_fwd_bwd_ms"] = round(med[5], 3)
        out["phi_over_theta"] = round(med[4] / med[2], 2)
        out["tap_grad"] = [tap_grad_alone(nat, stream, timed, H, W, fl_k, a) for fl_k in (8, 15)]
    print(json.dumps(out), flush=True)


def tap_grad_alone(nat, stream, timed, H, W, fl, a, n=16):
    """fvvdp_tap_grad on n frames of random planes under a replicate window, against its bytes model."""
    dev = torch.device("cuda:0")
    HW = H * W
    g0, g0r = (torch.randn((n, 2, H, W), device=dev) for _ in range(2))
    lum = torch.rand((2, n, H, W), device=dev) * 100.0
    pos = np.ascontiguousarray(np.concatenate([np.zeros(fl - 1, np.int32), np.arange(n, dtype=np.int32)]))
    nbytes = C.c_size_t(0)
    lib = nat.lib()
    nat.check(lib.fvvdp_tap_grad_workspace(W, H, fl, C.byref(nbytes)))
    work = torch.empty((nbytes.value + 7) // 8, dtype=torch.float64, device=dev)
    out = torch.empty((2, fl), dtype=torch.float64, device=dev)
    st = C.c_void_p(stream.cuda_stream)

    def run():
        nat.check(lib.fvvdp_tap_grad(W, H, n, fl, C.c_void_p(g0.data_ptr()), C.c_void_p(g0r.data_ptr()), C.c_void_p(lum.data_ptr()),
                                     C.c_void_p(lum.data_ptr() + n * HW * 4), pos.ctypes.data_as(C.POINTER(C.c_int32)), n,
                                     C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()), nbytes.value, st))

    ts = [timed(run) for _ in range(a.warmup + a.steps)][a.warmup:]
    groups = (fl + nat.TAP_GROUP - 1) // nat.TAP_GROUP
    model = groups * n * HW * 24
    ms = float(np.median(ts))
    return {"taps": fl, "frames": n, "tap_groups": groups, "bytes_model": model, "ms": round(ms, 4),
            "spread_ms": [round(min(ts), 4), round(max(ts), 4)], "tb_per_s": round(model / (ms * 1e-3) / 1e12, 2),
            "hbm_peak_share": round(model / (ms * 1e-3) / HBM_PEAK, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=sorted(CASES), help="default: 60x1080x1920")
    ap.add_argument("--display", default="standard_4k")
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--temporal", action="store_true", help="also the gradients for the temporal filters' sigma and beta")
    a = ap.parse_args()
    for key in a.case or ["60x1080x1920"]:
        run_case(key, a)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
