"""Difference-map gradients against JOD gradients: fvvdp.diff_map_images / diff_map_video followed by backward() of a per-pixel
loss, against fvvdp.jod_images / jod_video followed by backward(), alternated in one process on the same resident float32
sources and timed with HIP events around work that ends in an event synchronise.  Prints one JSON line per case: the medians
of --steps calls of each variant, their ratio, and next to it the ratio the byte counts below predict.

The expectation under test: the map variants cost the scalar variants plus the traffic of the two reconstructions (forward, and
again without the power in the backward for units="jod"), of the D maps the forward now writes and of the A chain -- each about
4/3 of a level-0 plane read and written per entry.  extra_bytes() counts that traffic; the tool measures the rate of a plain
device-to-device copy in the same process and predicts  ratio = 1 + extra_bytes / copy_rate / scalar_ms.

    python tools/bench_diff_map.py                     # 8 x 1080p pairs, 60 x 1080p and 60 x 2160p clips, units="jod"
    python tools/bench_diff_map.py --case v60x2160x3840 --units linear
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name: (kind, entries, H, W)
CASES = {"i8x1080x1920": ("images", 8, 1080, 1920), "v60x1080x1920": ("video", 60, 1080, 1920),
         "v60x2160x3840": ("video", 60, 2160, 3840)}


def levels(W, H, n_bands):
    out = [(W, H)]
    for _ in range(n_bands - 1):
        w, h = out[-1]
        out.append(((w + 1) // 2, (h + 1) // 2))
    return out


def extra_bytes(n, H, W, n_bands, nc, units):
    """Bytes the map variant moves on top of the scalar variant, for n entries with nc temporal channels (fp32; neighbour
    re-reads served by caches are not counted)."""
    px = [w * h for w, h in levels(W, H, n_bands)]
    band_px, HW = sum(px), px[0]
    # one reconstruction: D of nc channels read and v written per band pixel, every level but level 0 read once by the finer one
    recon = band_px * (4 * nc + 4) + (band_px - HW) * 4
    out = {
        "forward_d_maps_written": n * band_px * 4 * nc,
        "forward_reconstruction": n * recon,
        "backward_reconstruction": n * recon if units == "jod" else 0,
        # G (and v_0) read at level 0, A written per band pixel, every A but the coarsest read once by the coarser level
        "a_chain": n * (HW * (8 if units == "jod" else 4) + band_px * 4 + (band_px - px[-1]) * 4),
        # the cotangent itself: the loss writes it, the backward reads it
        "result_and_cotangent": n * HW * 8,
    }
    out["total"] = sum(out.values())
    out["level0_planes_per_entry"] = round(out["total"] / (n * HW * 4), 2)
    return out


def copy_rate(dev, stream):
    """Bytes per second (read + written) of a device-to-device copy of 1 GiB, the median of 5."""
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    ts = []
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        dst.copy_(src)
        e1.record(stream)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return 2.0 * src.numel() * 4 / (float(np.median(ts[1:])) * 1e-3)


def run_case(key, a):
    import fovvideovdp_amd as fv
    from fovvideovdp_amd.fvvdp import band_frequencies
    kind, n, H, W = CASES[key]
    C = 3
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    shape = (n, C, H, W) if kind == "images" else (1, C, n, H, W)
    ref = torch.rand(shape, device=dev, generator=g)
    test = (ref + 0.05 * torch.randn(shape, device=dev, generator=g)).clamp(0, 1)
    weight = torch.rand((n, H, W), device=dev, generator=g)
    m = fv.fvvdp(display_name=a.display, device=dev, quiet=True)
    stream = torch.cuda.current_stream(dev)
    kw = {} if kind == "images" else {"frames_per_second": a.fps}
    jod_fn = m.jod_images if kind == "images" else m.jod_video
    map_fn = m.diff_map_images if kind == "images" else m.diff_map_video

    def scalar():
        x = test.detach().requires_grad_(True)
        jod_fn(x, ref, **kw).sum().backward()

    def per_pixel():
        x = test.detach().requires_grad_(True)
        map_fn(x, ref, units=a.units, **kw).backward(weight)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        timed(scalar)
        timed(per_pixel)
    ts, tm = [], []
    for _ in range(a.steps):                       # the variants alternate: drift of the clocks hits both alike
        ts.append(timed(scalar))
        tm.append(timed(per_pixel))
    ms_s, ms_m = float(np.median(ts)), float(np.median(tm))
    n_bands = band_frequencies(W, H, m.pix_per_deg)[0]
    eb = extra_bytes(n, H, W, n_bands, 1 if kind == "images" else 2, a.units)
    rate = copy_rate(dev, stream)
    print(json.dumps({
        "case": key, "kind": kind, "entries": n, "height": H, "width": W, "channels": C, "units": a.units, "display": a.display,
        "n_bands": n_bands, "jod_fwd_bwd_ms": round(ms_s, 3), "map_fwd_bwd_ms": round(ms_m, 3),
        "measured_ratio": round(ms_m / ms_s, 3), "extra_bytes": eb, "copy_tb_per_s": round(rate / 1e12, 2),
        "expected_ratio": round(1.0 + eb["total"] / rate / (ms_s * 1e-3), 3),
        "jod_ms_spread": [round(min(ts), 3), round(max(ts), 3)], "map_ms_spread": [round(min(tm), 3), round(max(tm), 3)]}),
        flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=sorted(CASES), help="default: every case")
    ap.add_argument("--display", default="standard_4k")
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--units", default="jod", choices=["jod", "linear"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    a = ap.parse_args()
    for key in a.case or sorted(CASES):
        run_case(key, a)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
