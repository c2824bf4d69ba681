"""Half-precision sources: what float16 / bfloat16 input buys over float32 on one resident RGB clip behind sRGB, the variants
alternated inside one process, medians of --steps (7) timed calls, the whole measurement made --runs (2) times.  One JSON line per
measurement:

  k1       the ingest kernel alone (fvvdp_ctx_timing_*: HIP events around fvvdp_temporal_channels), microseconds per frame, for the
           clip as float32, float16 and bfloat16;
  fwd_bwd  fvvdp.jod_video forward + backward() in milliseconds and torch.cuda.max_memory_allocated in GB for
             half        the half clip as it is,
             float32     a float32 clip,
             upcast      the half clip converted with .float() inside the timed region -- what callers had to do before.

    python tools/bench_half.py                         # k1 at 3840x2160x60; fwd_bwd at 1920x1080x60 and 3840x2160x60
    python tools/bench_half.py --only k1 --frames 30
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def make_clip(N, H, W, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    ref = torch.rand((1, 3, N, H, W), device=dev, generator=g)
    test = (ref + 0.05 * torch.randn((1, 3, N, H, W), device=dev, generator=g)).clamp(0, 1)
    return test, ref


def k1_us_per_frame(m, test, ref, fps, steps):
    from fovvideovdp_amd import _native as nat
    N = test.shape[2]
    ms, cnt = (C.c_float * 18)(), (C.c_int32 * 18)()
    m.predict(test, ref, frames_per_second=fps)                     # warm-up: context, tables
    nat.check(nat.lib().fvvdp_ctx_timing_read(m._ctx.handle, ms, cnt, 18, 1))
    out = []
    for _ in range(steps):
        m.predict(test, ref, frames_per_second=fps)
        nat.check(nat.lib().fvvdp_ctx_timing_read(m._ctx.handle, ms, cnt, 18, 1))
        out.append(ms[0] / N * 1e3)
    return out


def run_k1(a, dev, run):
    import fovvideovdp_amd as fv
    N, H, W = a.frames, 2160, 3840
    test, ref = make_clip(N, H, W, dev)
    clips = {k: (test.to(d), ref.to(d)) for k, d in DTYPES.items()}
    del test, ref
    m = fv.fvvdp(display_name="standard_4k", device=dev, quiet=True)
    m.timing = True
    res = {k: [] for k in DTYPES}
    for _ in range(a.steps):                                        # alternated: one timed call per variant and round
        for k in DTYPES:
            res[k] += k1_us_per_frame(m, clips[k][0], clips[k][1], a.fps, 1)
    print(json.dumps({"measure": "k1", "run": run, "frames": N, "height": H, "width": W, "fps": a.fps,
                      "us_per_frame": {k: {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                       for k, v in res.items()}}), flush=True)


def run_fwd_bwd(a, dev, run, N, H, W, half):
    import fovvideovdp_amd as fv
    test, ref = make_clip(N, H, W, dev)
    t16, r16 = test.to(half), ref.to(half)
    m = fv.fvvdp(display_name="standard_4k", device=dev, quiet=True)
    stream = torch.cuda.current_stream(dev)

    def step(variant):
        if variant == "half":
            x, y = t16.detach().requires_grad_(True), r16
        elif variant == "float32":
            x, y = test.detach().requires_grad_(True), ref
        else:
            x16 = t16.detach().requires_grad_(True)
            x, y = x16.float(), r16.float()
        m.jod_video(x, y, frames_per_second=a.fps).backward()

    def timed(variant):
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        step(variant)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), (torch.cuda.max_memory_allocated(dev) - base) / 1e9

    variants = ("half", "float32", "upcast")
    for v in variants:
        timed(v)
    ms = {v: [] for v in variants}
    mem = {v: 0.0 for v in variants}
    for _ in range(a.steps):
        for v in variants:
            t, g = timed(v)
            ms[v].append(t)
            mem[v] = max(mem[v], g)
    print(json.dumps({"measure": "fwd_bwd", "run": run, "half": str(half), "frames": N, "height": H, "width": W, "fps": a.fps,
                      "resident_clips_gb": {"half": round(2 * t16.numel() * 2 / 1e9, 2), "float32": round(2 * test.numel() * 4 / 1e9, 2)},
                      "ms": {v: {"median": round(float(np.median(x)), 2), "min": round(min(x), 2), "max": round(max(x), 2)}
                             for v, x in ms.items()},
                      "peak_gb_above_resident": {v: round(g, 2) for v, g in mem.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--only", choices=["k1", "fwd_bwd"], default=None)
    ap.add_argument("--half", choices=["float16", "bfloat16"], default="float16")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for run in range(a.runs):
        if a.only in (None, "k1"):
            run_k1(a, dev, run)
            torch.cuda.empty_cache()
        if a.only in (None, "fwd_bwd"):
            for H, W in ((1080, 1920), (2160, 3840)):
                run_fwd_bwd(a, dev, run, a.frames, H, W, DTYPES[a.half])
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
