"""Gradients of a clip shown by sample-and-hold: three ways to get them, alternated in one process on the same resident clips and
timed with HIP events around work that ends in an event synchronise.

  (a) fvvdp.jod_video_held(test, ref, test_frames=k).backward() on the test clip of N / k frames;
  (b) what a caller writes without it: test.repeat_interleave(k, dim=frames) under autograd, jod_video on the expanded clip,
      backward() -- torch adds the gradients of the copies back together;
  (c) jod_video + backward() on a clip expanded beforehand: the floor (its gradient has the expanded clip's size).

Prints one JSON line per case: median ms of 7 per variant, the spread, the peak device memory of each variant above the resident
clips, and the bytes model's prediction: the ingest moves what (c)'s moves, the last backward kernel
8 + 8C / k against 8 + 8C bytes per pixel and display frame, (b) writes and re-reads the expanded clip and its gradient on top.

    python tools/bench_held.py                       # k = 2 and 4 at 1920x1080x60 and 3840x2160x60, float32 RGB, 60 fps
    python tools/bench_held.py --case 60x2160x3840 --hold 4
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"60x1080x1920": (60, 1080, 1920), "60x2160x3840": (60, 2160, 3840)}


def run_case(key, k, a):
    import fovvideovdp_amd as fv
    N, H, W = CASES[key]
    assert N % k == 0
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    ref = torch.rand((1, 3, N, H, W), device=dev, generator=g)
    test = (ref[:, :, ::k] + 0.05 * torch.randn((1, 3, N // k, H, W), device=dev, generator=g)).clamp_(0.02, 0.98).contiguous()
    expanded = test.repeat_interleave(k, dim=2).contiguous()
    m = fv.fvvdp(display_name=a.display, device=dev, quiet=True)
    stream = torch.cuda.current_stream(dev)
    jods = {}

    def va():
        t = test.detach().requires_grad_(True)
        q = m.jod_video_held(t, ref, frames_per_second=a.fps, test_frames=k)
        q.backward()
        jods["a"] = q.detach()

    def vb():
        t = test.detach().requires_grad_(True)
        q = m.jod_video(t.repeat_interleave(k, dim=2), ref, frames_per_second=a.fps)
        q.backward()
        jods["b"] = q.detach()

    def vc():
        q = m.jod_video(expanded.detach().requires_grad_(True), ref, frames_per_second=a.fps)
        q.backward()
        jods["c"] = q.detach()

    variants = {"a_jod_video_held": va, "b_repeat_interleave_jod_video": vb, "c_jod_video_expanded": vc}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    times = {n: [] for n in variants}
    peak = {}
    for _ in range(a.warmup):
        for n, fn in variants.items():
            timed(fn)
    for n, fn in variants.items():                  # peak memory above what is resident, one variant at a time
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        timed(fn)
        peak[n] = round((torch.cuda.max_memory_allocated(dev) - base) / 1e9, 3)
    for _ in range(a.steps):
        for n, fn in variants.items():
            times[n].append(timed(fn))
    med = {n: float(np.median(v)) for n, v in times.items()}
    same = float(jods["a"]).hex() == float(jods["b"]).hex() == float(jods["c"]).hex()
    out = {"case": key, "hold": k, "display_frames": N, "test_frames": N // k, "height": H, "width": W, "fps": a.fps, "display": a.display,
           "jod": float(jods["a"]).hex(), "jod_bits_equal": same,
           "median_ms": {n: round(v, 3) for n, v in med.items()},
           "spread_ms": {n: [round(min(v), 3), round(max(v), 3)] for n, v in times.items()},
           "peak_gb_above_resident": peak,
           "a_over_c": round(med["a_jod_video_held"] / med["c_jod_video_expanded"], 3),
           "a_over_b": round(med["a_jod_video_held"] / med["b_repeat_interleave_jod_video"], 3),
           "bytes_model": {"last_backward_kernel_bytes_per_px_display_frame": {"a": 8 + 24 / k, "c": 32},
                           "b_extra_bytes_per_px_display_frame": 24 + 24 / k,
                           "prediction": "a / c = 0.96 ... 1.00, a / b = 0.90 ... 0.95, peak memory of a below b"}}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=sorted(CASES), help="default: every case")
    ap.add_argument("--hold", action="append", type=int, choices=(2, 4), help="default: 2 and 4")
    ap.add_argument("--display", default="standard_4k")
    ap.add_argument("--fps", type=float, default=60.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    a = ap.parse_args()
    for key in a.case or sorted(CASES):
        for k in a.hold or (2, 4):
            run_case(key, k, a)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
