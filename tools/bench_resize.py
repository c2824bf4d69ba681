"""Gradients of a clip that is shown resized: three ways to get them, alternated in one process on the same resident clips and
timed with HIP events around work that ends in an event synchronise.

  (a) fvvdp.jod_video_resized(...).backward() on the small test clip;
  (b) what a caller writes without it: torch.nn.functional.interpolate(...).clip(0, 1) under autograd, jod_video on the clip at the
      target size, backward() -- the baseline;
  (c) jod_video + backward() on a resident float32 clip already at the target size: the floor of everything behind the ingest.

Prints one JSON line per case and mode: median ms of 7 per variant, the spread, the peak device memory of each variant above the
resident clips, and the prediction of the bytes model.  Run it twice and compare: the medians of two runs are
what the document quotes.

    python tools/bench_resize.py                         # 960x540 -> 1920x1080 x 60 and 1920x1080 -> 3840x2160 x 60, both modes
    python tools/bench_resize.py --case 60x1080x1920 --mode bicubic
    python tools/bench_resize.py --case 60x540x960 --mode area          # x2: windows of one sample, the cost of the index arithmetic
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# frames x source height x source width; the target is twice the source in each axis
CASES = {"60x540x960": (60, 540, 960), "60x1080x1920": (60, 1080, 1920)}


def run_case(key, mode, a):
    import fovvideovdp_amd as fv
    N, h, w = CASES[key]
    H, W = 2 * h, 2 * w
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    test = torch.rand((1, 3, N, h, w), device=dev, generator=g) * 1.1 - 0.05          # some samples beyond [0, 1]: the clip binds
    with torch.no_grad():
        ref = torch.nn.functional.interpolate(test[0].permute(1, 0, 2, 3), size=(H, W), mode="bilinear").clip(0, 1)
        ref = (ref + 0.02 * torch.randn(ref.shape, device=dev, generator=g)).clip(0, 1).permute(1, 0, 2, 3)[None].contiguous()
        test_full = (ref + 0.02 * torch.randn(ref.shape, device=dev, generator=g)).clip(0, 1)
    m = fv.fvvdp(display_name=a.display, device=dev, quiet=True)
    stream = torch.cuda.current_stream(dev)

    def va():
        t = test.detach().requires_grad_(True)
        m.jod_video_resized(t, ref, full_screen_resize=mode, resize_resolution=(W, H), frames_per_second=a.fps).backward()

    def vb():
        t = test.detach().requires_grad_(True)
        up = torch.nn.functional.interpolate(t[0].permute(1, 0, 2, 3), size=(H, W), mode=mode).clip(0, 1).permute(1, 0, 2, 3)[None]
        m.jod_video(up, ref, frames_per_second=a.fps).backward()

    def vc():
        m.jod_video(test_full.detach().requires_grad_(True), ref, frames_per_second=a.fps).backward()

    variants = {"a_jod_video_resized": va, "b_torch_interpolate_jod_video": vb, "c_jod_video_at_target": vc}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    times = {k: [] for k in variants}
    peak = {}
    for _ in range(a.warmup):
        for k, fn in variants.items():
            timed(fn)
    for k, fn in variants.items():                  # peak memory above what is resident, one variant at a time
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        timed(fn)
        peak[k] = round((torch.cuda.max_memory_allocated(dev) - base) / 1e9, 3)
    for _ in range(a.steps):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = {"case": key, "mode": mode, "frames": N, "source": [w, h], "target": [W, H], "fps": a.fps, "display": a.display,
           "median_ms": {k: round(v, 3) for k, v in med.items()},
           "spread_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
           "peak_gb_above_resident": peak,
           "a_over_c": round(med["a_jod_video_resized"] / med["c_jod_video_at_target"], 3),
           "a_over_b": round(med["a_jod_video_resized"] / med["b_torch_interpolate_jod_video"], 3),
           "bytes_model": {"ingest_bytes_per_target_px_frame": {"a_small_stream": "3 (x2 bilinear)", "c": 12},
                           "backward_tail_bytes_per_target_px_frame": {"a": "4 + 12 + 12 + 12 / f^2", "c": 32},
                           "prediction": "a / c = 0.98 ... 1.00, a / b = 0.7 ... 0.8 or lower"}}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=sorted(CASES), help="default: every case")
    ap.add_argument("--mode", action="append", choices=("bilinear", "bicubic", "nearest", "area"), help="default: bilinear and bicubic")
    ap.add_argument("--display", default="standard_4k")
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    a = ap.parse_args()
    for key in a.case or sorted(CASES):
        for mode in a.mode or ("bilinear", "bicubic"):
            run_case(key, mode, a)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
