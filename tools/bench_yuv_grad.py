"""Gradients of a planar YUV clip: three ways to get them, alternated in one process on the same resident 4:2:0 clip and timed
with HIP events around work that ends in an event synchronise.

  (a) fvvdp.jod_video_yuv(...).backward() on the float planes;
  (b) what a caller writes without it: the torch ops of fvvdp_video_source_yuv_frames.unpack under autograd on the float planes,
      jod_video on the RGB clip, backward();
  (c) jod_video + backward() on a resident float32 RGB clip of the same size: the floor.

Prints one JSON line per case: median ms of 7 per variant, the spread, the peak device memory of each variant above the resident
clip, and the bytes model's prediction -- ingest 6 B against 12 B per pixel and frame, a backward tail of 8 + 4 + 4 + 6 + 6 = 28 B
against 32 B -- of (a) about equal to (c) or slightly below.

    python tools/bench_yuv_grad.py                       # 1920x1080x60 and 3840x2160x60, sRGB, 8 bit
    python tools/bench_yuv_grad.py --case 60x2160x3840
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"60x1080x1920": (60, 1080, 1920), "60x2160x3840": (60, 2160, 3840)}


def unpack_rgb(Y, U, V, M):
    """fvvdp_video_source_yuv_frames.unpack on [N, H, W] + 2 x [N, H/2, W/2] planes of 8-bit code values -> [1, 3, N, H, W]."""
    Yf = torch.clip(Y * (1 / 219) - 16 / 219, 0, 1)
    uv = torch.clip(torch.stack((U, V), 1) * (1 / 224) - 128 / 224, -0.5, 0.5)
    uv = torch.nn.functional.interpolate(uv, scale_factor=2, mode='bilinear')
    Yuv = torch.cat((Yf[:, None], uv), 1).permute(0, 2, 3, 1)
    return (Yuv @ M.transpose(1, 0)).clip(0, 1).permute(3, 0, 1, 2)[None]


def run_case(key, a):
    import fovvideovdp_amd as fv
    from fovvideovdp_amd.video_source_yuv import YCBCR2RGB
    N, H, W = CASES[key]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)

    def planes(noise):
        out = []
        for shape, lo, hi in (((N, H, W), 16.0, 235.0), ((N, H // 2, W // 2), 64.0, 192.0), ((N, H // 2, W // 2), 64.0, 192.0)):
            out.append(torch.rand(shape, device=dev, generator=g) * (hi - lo) + lo + noise * torch.randn(shape, device=dev, generator=g))
        return out
    ref = planes(0.0)
    test = [r + 3.0 * torch.randn(r.shape, device=dev, generator=g) for r in ref]
    M = torch.tensor(YCBCR2RGB["bt709"], dtype=torch.float32, device=dev)
    with torch.no_grad():
        ref_rgb = unpack_rgb(*ref, M).contiguous()
        test_rgb = unpack_rgb(*test, M).contiguous()
    m = fv.fvvdp(display_name=a.display, device=dev, quiet=True)
    stream = torch.cuda.current_stream(dev)

    def va():
        t = [p.detach().requires_grad_(True) for p in test]
        m.jod_video_yuv(tuple(t), tuple(ref), frames_per_second=a.fps).backward()

    def vb():
        t = [p.detach().requires_grad_(True) for p in test]
        m.jod_video(unpack_rgb(*t, M), ref_rgb, frames_per_second=a.fps).backward()

    def vc():
        m.jod_video(test_rgb.detach().requires_grad_(True), ref_rgb, frames_per_second=a.fps).backward()

    variants = {"a_jod_video_yuv": va, "b_torch_unpack_jod_video": vb, "c_jod_video_rgb": vc}

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
    out = {"case": key, "frames": N, "height": H, "width": W, "fps": a.fps, "display": a.display, "chroma": "420", "bit_depth": 8,
           "median_ms": {k: round(v, 3) for k, v in med.items()},
           "spread_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
           "peak_gb_above_resident": peak,
           "a_over_c": round(med["a_jod_video_yuv"] / med["c_jod_video_rgb"], 3),
           "b_over_c": round(med["b_torch_unpack_jod_video"] / med["c_jod_video_rgb"], 3),
           "bytes_model": {"ingest_bytes_per_px_frame": {"a": 6, "c": 12}, "backward_tail_bytes_per_px_frame": {"a": 28, "c": 32},
                           "prediction": "a about equal to c or slightly below, b well above both"}}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=sorted(CASES), help="default: every case")
    ap.add_argument("--display", default="standard_4k")
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    a = ap.parse_args()
    for key in a.case or sorted(CASES):
        run_case(key, a)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
