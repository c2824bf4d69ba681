"""Display gradients: fvvdp.display_jod_video with a psi that requires grad (forward with the sums, then backward(), which is host
arithmetic on six doubles) against its comparator, forward + backward of fvvdp.jod_video(wrt="both") -- the call
tools/bench_video_grad.py --wrt both times -- and the plain forward (fvvdp.predict, sync=False).  The display call makes the
comparator's passes without its two gradient-writing launches (video_input_kernel) and with two reductions in their place; it
is also timed without its backward(), which makes no launch but reads the sums back and so waits for the device.  The four are
alternated in one process on the same resident float clip and timed with HIP events around work that ends in an event
synchronise.  Prints one JSON line per case: median ms per call with the spread (min, max), Gpix/s (test + reference pixels)
and the ratios.

    python tools/bench_display.py                                 # 1920x1080x60 and 3840x2160x60 RGB at 30 fps
    python tools/bench_display.py --case 60x2160x3840 --steps 9
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"60x1080x1920": (60, 1080, 1920), "60x2160x3840": (60, 2160, 3840)}


def run_case(key, a):
    import fovvideovdp_amd as fv
    N, H, W = CASES[key]
    C = 3
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    ref = torch.rand((1, C, N, H, W), device=dev, generator=g)
    test = (ref + 0.05 * torch.randn((1, C, N, H, W), device=dev, generator=g)).clamp(0, 1)
    m = fv.fvvdp(display_name=a.display, device=dev, quiet=True)
    psi0 = m.display_parameter_tensor()
    stream = torch.cuda.current_stream(dev)

    def fwd():
        m.predict(test, ref, frames_per_second=a.fps, sync=False)

    def video_both():
        x, y = test.detach().requires_grad_(True), ref.detach().requires_grad_(True)
        m.jod_video(x, y, frames_per_second=a.fps, wrt="both").backward()

    def display():
        psi = psi0.clone().requires_grad_(True)
        m.display_jod_video(test, ref, psi, frames_per_second=a.fps).backward()

    def display_sums_only():
        # the same launches without backward(): what is left is the read-back of six doubles and the chain, which run after
        # the device has drained
        m.display_jod_video(test, ref, psi0.clone().requires_grad_(True), frames_per_second=a.fps)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    fns = (fwd, video_both, display, display_sums_only)
    for _ in range(a.warmup):
        for fn in fns:
            timed(fn)
    times = [[] for _ in fns]
    for _ in range(a.steps):
        for t, fn in zip(times, fns):
            t.append(timed(fn))
    ms = [float(np.median(t)) for t in times]
    px = 2.0 * N * H * W
    out = {"case": key, "frames": N, "height": H, "width": W, "channels": C, "fps": a.fps, "display": a.display}
    for name, t, med in zip(("forward", "jod_video_both", "display", "display_without_backward"), times, ms):
        out[name + "_ms"] = round(med, 3)
        out[name + "_ms_spread"] = [round(min(t), 3), round(max(t), 3)]
        out[name + "_gpix_per_s"] = round(px / (med * 1e-3) / 1e9, 2)
    out["display_over_jod_video_both"] = round(ms[2] / ms[1], 3)
    out["display_without_backward_over_jod_video_both"] = round(ms[3] / ms[1], 3)
    out["display_over_forward"] = round(ms[2] / ms[0], 2)
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
