"""Gradients of a small clip shown full screen AND by sample-and-hold: three ways to get them, alternated in one process on the same
resident clips and timed with HIP events around work that ends in an event synchronise.

  (a) fvvdp.jod_video_resized(test, ref, test_frames=k).backward() on the test clip of N / k small frames;
  (b) what a caller writes without it: test.repeat_interleave(k, dim=frames) under autograd, jod_video_resized on the expanded
      clip, backward() -- torch adds the gradients of the copies back together;
  (c) jod_video_resized + backward() on a small clip expanded beforehand (its gradient has the expanded clip's frame count).

Prints one JSON line per case: median ms of 7 per variant, the spread, the peak device memory of each variant above the resident
clips, and the work model's prediction: in both ingests the test stream is interpolated and sent through the
display model for 1 / k of the display frames, the two stages of the resize's adjoint run on N / k frames (plus the run sum's 4 B
per target pixel and display frame), and neither an expanded clip nor its gradient exists.

    python tools/bench_resize_held.py                # k = 2 and 4, bilinear and bicubic, 960x540 -> 1920x1080 and 1920x1080 -> 3840x2160, 60 frames
    python tools/bench_resize_held.py --case 1080to2160 --hold 2 --mode bilinear
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name: (display frames, (source h, w), (target h, w))
CASES = {"540to1080": (60, (540, 960), (1080, 1920)), "1080to2160": (60, (1080, 1920), (2160, 3840))}


def run_case(key, k, mode, a):
    import fovvideovdp_amd as fv
    N, (h, w), (H, W) = CASES[key]
    assert N % k == 0
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    ref = torch.rand((1, 3, N, H, W), device=dev, generator=g)
    small = torch.nn.functional.interpolate(ref[0, :, ::k].permute(1, 0, 2, 3), size=(h, w), mode="area").permute(1, 0, 2, 3)[None]
    test = (small + 0.05 * torch.randn(small.shape, device=dev, generator=g)).clamp_(0.02, 0.98).contiguous()
    expanded = test.repeat_interleave(k, dim=2).contiguous()
    m = fv.fvvdp(display_name=a.display, device=dev, quiet=True)
    kw = dict(full_screen_resize=mode, resize_resolution=(W, H), frames_per_second=a.fps)
    stream = torch.cuda.current_stream(dev)
    jods = {}

    def va():
        t = test.detach().requires_grad_(True)
        q = m.jod_video_resized(t, ref, test_frames=k, **kw)
        q.backward()
        jods["a"] = q.detach()

    def vb():
        t = test.detach().requires_grad_(True)
        q = m.jod_video_resized(t.repeat_interleave(k, dim=2), ref, **kw)
        q.backward()
        jods["b"] = q.detach()

    def vc():
        q = m.jod_video_resized(expanded.detach().requires_grad_(True), ref, **kw)
        q.backward()
        jods["c"] = q.detach()

    variants = {"a_test_frames": va, "b_repeat_interleave": vb, "c_expanded_beforehand": vc}

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
    out = {"case": key, "hold": k, "mode": mode, "display_frames": N, "test_frames": N // k, "source": [w, h], "target": [W, H],
           "fps": a.fps, "display": a.display, "jod": float(jods["a"]).hex(), "jod_bits_equal": same,
           "median_ms": {n: round(v, 3) for n, v in med.items()},
           "spread_ms": {n: [round(min(v), 3), round(max(v), 3)] for n, v in times.items()},
           "peak_gb_above_resident": peak,
           "a_over_b": round(med["a_test_frames"] / med["b_repeat_interleave"], 3),
           "a_over_c": round(med["a_test_frames"] / med["c_expanded_beforehand"], 3),
           "peak_a_below_b": peak["a_test_frames"] < peak["b_repeat_interleave"],
           "work_model": {"test_stream_conversions_per_display_frame": 1.0 / k, "adjoint_frames": N // k,
                          "run_sum_bytes_per_target_px_display_frame": 4,
                          "prediction": "a faster than c by the saved share of the ingests and of the adjoint, b slower than c by "
                                        "the expanded clip and its gradient; peak memory of a below b"}}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=sorted(CASES), help="default: every case")
    ap.add_argument("--hold", action="append", type=int, choices=(2, 4), help="default: 2 and 4")
    ap.add_argument("--mode", action="append", choices=("bilinear", "bicubic", "nearest", "area"), help="default: bilinear and bicubic")
    ap.add_argument("--display", default="standard_4k")
    ap.add_argument("--fps", type=float, default=60.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    a = ap.parse_args()
    for key in a.case or sorted(CASES):
        for mode in a.mode or ("bilinear", "bicubic"):
            for k in a.hold or (2, 4):
                run_case(key, k, mode, a)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
