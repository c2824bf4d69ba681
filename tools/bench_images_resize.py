"""Gradients of a mini-batch of stills that are shown resized: three ways to get them, alternated in one process on the same
resident stacks and timed with HIP events around work that ends in an event synchronise.

  (a) fvvdp.jod_images_resized(...).sum().backward() on the small test stack;
  (b) what a caller writes without it: torch.nn.functional.interpolate(...).clip(0, 1) under autograd, jod_images on the stack at
      the target size, backward() -- the baseline;
  (c) jod_images + backward() on a resident float32 stack already at the target size: the floor of everything behind the ingest.

Prints one JSON line per case and mode: median ms of 7 per variant, the spread, the peak device memory of each variant above the
resident stacks, and the prediction of the bytes model.  Run it twice and compare: the medians of two runs
are what the document quotes.

    python tools/bench_images_resize.py                       # 960x540 -> 1920x1080 x 8 and 1920x1080 -> 3840x2160 x 8, both modes
    python tools/bench_images_resize.py --case 8x1080x1920 --mode bicubic
    python tools/bench_images_resize.py --wrt both            # the reference resized from the test's size as well, both gradients
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# pairs x source height x source width; the target is twice the source in each axis
CASES = {"8x540x960": (8, 540, 960), "8x1080x1920": (8, 1080, 1920)}


def run_case(key, mode, a):
    import fovvideovdp_amd as fv
    B, h, w = CASES[key]
    H, W = 2 * h, 2 * w
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    test = torch.rand((B, 3, h, w), device=dev, generator=g) * 1.1 - 0.05                # some samples beyond [0, 1]: the clip binds
    with torch.no_grad():
        ref = torch.nn.functional.interpolate(test, size=(H, W), mode="bilinear").clip(0, 1)
        ref = (ref + 0.02 * torch.randn(ref.shape, device=dev, generator=g)).clip(0, 1).contiguous()
        test_full = (ref + 0.02 * torch.randn(ref.shape, device=dev, generator=g)).clip(0, 1)
        ref_small = torch.nn.functional.avg_pool2d(ref, 2)
    both = a.wrt == "both"
    m = fv.fvvdp(display_name=a.display, device=dev, quiet=True)
    stream = torch.cuda.current_stream(dev)

    def show(x):
        return torch.nn.functional.interpolate(x, size=(H, W), mode=mode).clip(0, 1)

    def va():
        t = test.detach().requires_grad_(True)
        r = ref_small.detach().requires_grad_(True) if both else ref
        m.jod_images_resized(t, r, full_screen_resize=mode, resize_resolution=(W, H), wrt=a.wrt).sum().backward()

    def vb():
        t = test.detach().requires_grad_(True)
        r = show(ref_small.detach().requires_grad_(True)) if both else ref
        m.jod_images(show(t), r, wrt=a.wrt).sum().backward()

    def vc():
        r = ref.detach().requires_grad_(True) if both else ref
        m.jod_images(test_full.detach().requires_grad_(True), r, wrt=a.wrt).sum().backward()

    variants = {"a_jod_images_resized": va, "b_torch_interpolate_jod_images": vb, "c_jod_images_at_target": vc}

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
    out = {"case": key, "mode": mode, "wrt": a.wrt, "pairs": B, "source": [w, h], "target": [W, H], "display": a.display,
           "median_ms": {k: round(v, 3) for k, v in med.items()},
           "spread_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
           "peak_gb_above_resident": peak,
           "a_over_c": round(med["a_jod_images_resized"] / med["c_jod_images_at_target"], 3),
           "a_over_b": round(med["a_jod_images_resized"] / med["b_torch_interpolate_jod_images"], 3),
           "bytes_model": {"ingest_bytes_per_target_px_pair": {"a": "12 / f^2 + 12 + 8 = 23", "c": 32},
                           "backward_tail_bytes_per_target_px_pair": {"a": "9 + 19 + 12 + 12 / f^2 = 43", "c": 29},
                           "prediction": "a / c = 0.99 ... 1.00, a / b = 0.7 ... 0.8 or lower (wrt=test, f = 2)"}}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=sorted(CASES), help="default: every case")
    ap.add_argument("--mode", action="append", choices=("bilinear", "bicubic", "nearest", "area"), help="default: bilinear and bicubic")
    ap.add_argument("--wrt", default="test", choices=("test", "both"))
    ap.add_argument("--display", default="standard_4k")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    a = ap.parse_args()
    for key in a.case or sorted(CASES):
        for mode in a.mode or ("bilinear", "bicubic"):
            run_case(key, mode, a)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
