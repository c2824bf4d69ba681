"""Batched still-image throughput: `pairs` image pairs of H x W through fvvdp.predict_images (one batch call, sync=False,
timed with HIP events), alternated in the same process with the same pairs through a loop of predict(..., sync=False)
calls.  Prints one JSON line: median ms per batch call, Gpix/s (test + reference pixels), the loop's median ms and the
speedup, and the ingest kernel's bytes per pair from its model (2 * C * sizeof(sample) read + 8 written per pixel).

    python tools/bench_images.py --pairs 256 --height 512 --width 512 --dtype uint8
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--dtype", default="uint8", choices=["uint8", "uint16", "float32"])
    ap.add_argument("--display", default="standard_fhd")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--no-loop", action="store_true", help="skip the loop of predict() calls")
    a = ap.parse_args()

    import fovvideovdp_amd as fv
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    B, C, H, W = a.pairs, a.channels, a.height, a.width
    ref = torch.rand((B, C, H, W), device=dev, generator=g)
    test = (ref + 0.05 * torch.randn((B, C, H, W), device=dev, generator=g)).clamp(0, 1)
    if a.dtype == "uint8":
        ref, test = (ref * 255).round().to(torch.uint8), (test * 255).round().to(torch.uint8)
    elif a.dtype == "uint16":
        ref = (ref * 65535).round().to(torch.int32).to(torch.int16)
        test = (test * 65535).round().to(torch.int32).to(torch.int16)
    m = fv.fvvdp(display_name=a.display, device=dev)
    ml = fv.fvvdp(display_name=a.display, device=dev)
    stream = torch.cuda.current_stream(dev)

    def batched():
        return m.predict_images(test, ref, sync=False)

    def loop():
        return [ml.predict(test[k], ref[k], dim_order="CHW", sync=False) for k in range(B)]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        timed(batched)
        if not a.no_loop:
            timed(loop)
    tb, tl = [], []
    for _ in range(a.steps):
        tb.append(timed(batched))
        if not a.no_loop:
            tl.append(timed(loop))
    ms = float(np.median(tb))
    es = test.element_size()
    out = {"pairs": B, "height": H, "width": W, "channels": C, "dtype": a.dtype, "display": a.display,
           "batch_ms": round(ms, 4), "ms_per_pair": round(ms / B, 5),
           "gpix_per_s": round(2.0 * B * H * W / (ms * 1e-3) / 1e9, 2),
           "ingest_bytes_per_pair": int(H * W * (2 * C * es + 8))}
    if tl:
        ml_ms = float(np.median(tl))
        out.update({"loop_ms": round(ml_ms, 4), "speedup": round(ml_ms / ms, 2)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
