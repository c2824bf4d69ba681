"""Video gradients: forward only (fvvdp.predict, sync=False) against forward + backward (fvvdp.jod_video, then backward()),
alternated in one process on the same resident float clip and timed with HIP events around work that ends in an event
synchronise.  Prints one JSON line per case: median ms per call, Gpix/s (test + reference pixels) and the ratio, plus the bytes
model of every kernel of the backward (include/fvvdp_hip_video_grad.h).

With --kernel-stats <rocprofv3 kernel_stats.csv> (from a separate `rocprofv3 --kernel-trace --stats` run of this script), each
line also gets the new kernels' mean time per launch, their bytes-model rate and its share of the 8 TB/s HBM peak.

    python tools/bench_video_grad.py                              # 1920x1080x30 and 3840x2160x60 RGB at 30 fps
    python tools/bench_video_grad.py --case 60x2160x3840 --kernel-stats prof/kernel_stats.csv
    python tools/bench_video_grad.py --wrt both                   # the gradient with respect to the reference, or to both inputs
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # MI355X HBM3E, bytes/s (MI355X_MICROARCH)
CASES = {"30x1080x1920": (30, 1080, 1920), "60x2160x3840": (60, 2160, 3840)}


def levels(W, H, n_bands):
    out = [(W, H)]
    for _ in range(n_bands):
        w, h = out[-1]
        out.append(((w + 1) // 2, (h + 1) // 2))
    return out


def bytes_model(N, C, H, W, n_bands, fl, wrt="test"):
    """Bytes each kernel of one backward call must move (fp32; neighbour re-reads served by caches are not counted).  The sweep,
    level 0 and the transpose run once per differentiated input (wrt="both": twice)."""
    lv = levels(W, H, n_bands)
    band_px = sum(w * h for w, h in lv[:n_bands])            # band-pass levels 0 .. n_bands - 1
    sweep_px = sum(w * h for w, h in lv[1:])                 # levels 1 .. n_bands
    out = _bytes_model_test(N, C, H, W, fl, band_px, sweep_px)
    if wrt != "test":
        # 11 map values read (D 2, contrast 4, L_bkg 1, S 2, slope 2), GLR and GX of both channels written
        out["ref_layer_kernel"] = N * band_px * 60
        out["maps_written"] = N * band_px * 44              # the slope planes on top of the 9 maps
    if wrt == "reference":
        del out["video_layer_kernel"]
    if wrt == "both":
        for k in ("adj_sweep_kernel", "video_level0_kernel", "video_input_kernel"):
            out[k] *= 2
    return out


def _bytes_model_test(N, C, H, W, fl, band_px, sweep_px):
    return {
        # 9 map values read (D 2, contrast 4, L_bkg 1, S 2), 2 layer gradients written
        "video_layer_kernel": N * band_px * 44,
        # per plane as for images: layer gradient of the level and of the finer one, coarser sweep gradient (1/4), 4 B written
        "adj_sweep_kernel": N * 2 * sweep_px * (4 + 16 + 1 + 4),
        # per plane: layer gradient of level 0, sweep gradient of level 1 (1/4), g0 written
        "video_level0_kernel": N * 2 * H * W * (4 + 1 + 4),
        # g0 read once (8 B), test samples read and gradient written once (8 C B) per pixel and frame; the head's side buffer
        # written and read once per clip
        "video_input_kernel": N * H * W * (8 + 8 * C) + fl * H * W * 8,
        # what the backward's re-run of the forward adds: the 9 maps written by the pyramid kernels
        "maps_written": N * band_px * 36,
    }


def kernel_stats(path):
    """rocprofv3 kernel_stats.csv -> {kernel base name: (calls, mean ns)}"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            base = name.split("(")[0].split("<")[0].strip()
            if base.startswith("void "):
                base = base[5:]
            calls = int(float(row.get("Calls", 0)))
            mean = float(row.get("AverageNs", row.get("Average", 0)))
            if base:
                c0, m0 = out.get(base, (0, 0.0))
                out[base] = (c0 + calls, (m0 * c0 + mean * calls) / max(c0 + calls, 1))
    return out


def run_case(key, a, stats):
    import fovvideovdp_amd as fv
    from fovvideovdp_amd.fvvdp import band_frequencies
    from fovvideovdp_amd.video_grad import filter_length, grad_batch_size, video_grad_planes
    N, H, W = CASES[key]
    C = 3
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    ref = torch.rand((1, C, N, H, W), device=dev, generator=g)
    test = (ref + 0.05 * torch.randn((1, C, N, H, W), device=dev, generator=g)).clamp(0, 1)
    m = fv.fvvdp(display_name=a.display, device=dev, quiet=True)
    stream = torch.cuda.current_stream(dev)

    def fwd():
        m.predict(test, ref, frames_per_second=a.fps, sync=False)

    def fwd_bwd():
        x = test.detach().requires_grad_(a.wrt != "reference")
        y = ref.detach().requires_grad_(a.wrt != "test")
        m.jod_video(x, y, frames_per_second=a.fps, wrt=a.wrt).backward()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        timed(fwd)
        timed(fwd_bwd)
    tf, tg = [], []
    for _ in range(a.steps):
        tf.append(timed(fwd))
        tg.append(timed(fwd_bwd))
    ms_f, ms_g = float(np.median(tf)), float(np.median(tg))
    n_bands = band_frequencies(W, H, m.pix_per_deg)[0]
    fl = filter_length(a.fps)
    bm = bytes_model(N, C, H, W, n_bands, fl, a.wrt)
    gb = grad_batch_size(m, W, H, n_bands, m._batch_size(W, H, 4, N, fl), video_grad_planes(a.wrt))
    px = 2.0 * N * H * W
    out = {"case": key, "frames": N, "height": H, "width": W, "channels": C, "fps": a.fps, "taps": fl, "display": a.display,
           "n_bands": n_bands, "grad_batch": gb, "wrt": a.wrt,
           "forward_ms": round(ms_f, 3), "forward_gpix_per_s": round(px / (ms_f * 1e-3) / 1e9, 2),
           "fwd_bwd_ms": round(ms_g, 3), "fwd_bwd_gpix_per_s": round(px / (ms_g * 1e-3) / 1e9, 2),
           "fwd_bwd_over_forward": round(ms_g / ms_f, 2), "bytes_model": bm,
           "forward_ms_spread": [round(min(tf), 3), round(max(tf), 3)],
           "fwd_bwd_ms_spread": [round(min(tg), 3), round(max(tg), 3)]}
    if stats:
        n_batches = (N + gb - 1) // gb
        sides = 2 if a.wrt == "both" else 1
        calls_per_bwd = {"video_layer_kernel": n_batches, "ref_layer_kernel": n_batches, "video_coef_kernel": sides * n_batches,
                         "adj_sweep_kernel": sides * n_bands * n_batches, "video_level0_kernel": sides * n_batches,
                         "video_input_kernel": sides}
        kern = {}
        for k, per in calls_per_bwd.items():
            if k in stats:
                calls, mean_ns = stats[k]
                t_bwd = mean_ns * per * 1e-9                  # seconds per backward call
                kern[k] = {"calls": calls, "mean_us": round(mean_ns / 1e3, 2), "us_per_backward": round(t_bwd * 1e6, 1)}
                if k in bm:
                    kern[k].update({"tb_per_s": round(bm[k] / t_bwd / 1e12, 2), "hbm_peak_share": round(bm[k] / t_bwd / HBM_PEAK, 3)})
        out["kernels"] = kern
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=sorted(CASES), help="default: every case")
    ap.add_argument("--display", default="standard_4k")
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--wrt", default="test", choices=["test", "reference", "both"], help="the input(s) the backward differentiates")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run")
    a = ap.parse_args()
    stats = kernel_stats(a.kernel_stats) if a.kernel_stats else None
    for key in a.case or sorted(CASES):
        run_case(key, a, stats)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
