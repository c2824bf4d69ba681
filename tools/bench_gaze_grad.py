#!/usr/bin/env python3
"""jod_gazes(...).sum().backward() against the loop of jod_video forward + backward calls, same process, alternated
("Gradients under many gazes").

Workload: 1920x1080, 30 frames at 30 frames per second, foveated standard_4k, moving gazes, float32 inputs resident on the
device.  For every G the two ways of getting the gradient of sum_g JOD_g are timed in turns --
    loop:   G x jod_video(x, ref, fixation_point=trace[g]).backward()      (the gradients accumulate in x.grad)
    gazes:  jod_gazes(x, ref, traces).sum().backward()
-- `--reps` times each with HIP events around forward + backward; the medians and the spread (min .. max) of the alternated
readings are printed, one JSON line per G and a summary line at the end.  The two gradients are compared on the way
(max|difference| / max|gradient|).

    python tools/bench_gaze_grad.py                       # G = 1 2 4 8 16
    python tools/bench_gaze_grad.py --gazes 8 --reps 3    # e.g. under a profiler
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fovvideovdp_amd as fv                                   # noqa: E402
from fovvideovdp_amd.synth import synth_video_pair              # noqa: E402
from bench_gazes import timed, traces                           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gazes", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--display", default="standard_4k")
    args = ap.parse_args()
    N, H, W = args.frames, args.height, args.width
    t8, r8 = synth_video_pair(N, H, W, device="cuda")
    test, ref = t8.to(torch.float32) / 255, r8.to(torch.float32) / 255
    del t8, r8
    m = fv.fvvdp(display_name=args.display, foveated=True)
    rows = []
    for G in args.gazes:
        fp = traces(G, N, H, W)

        def loop():
            x = test.detach().requires_grad_(True)
            for g in range(G):
                m.jod_video(x, ref, frames_per_second=args.fps, fixation_point=fp[g]).backward()
            return x.grad

        def gazes():
            x = test.detach().requires_grad_(True)
            m.jod_gazes(x, ref, fp, frames_per_second=args.fps).sum().backward()
            return x.grad

        loop()
        gazes()
        torch.cuda.synchronize()
        t_loop, t_gaze = [], []
        for _ in range(args.reps):                      # alternated: both see the same state of the box
            ms, g_loop = timed(loop)
            t_loop.append(ms)
            ms, g_gaze = timed(gazes)
            t_gaze.append(ms)
        rel = float((g_gaze - g_loop).abs().max() / g_loop.abs().max())
        row = dict(G=G, frames=N, loop_ms=float(np.median(t_loop)), loop_ms_range=[min(t_loop), max(t_loop)],
                   gazes_ms=float(np.median(t_gaze)), gazes_ms_range=[min(t_gaze), max(t_gaze)], rel_diff=rel)
        row["speedup"] = row["loop_ms"] / row["gazes_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(dict(tool="bench_gaze_grad", width=W, height=H, frames=N, fps=args.fps, display=args.display,
                          reps=args.reps, rows=rows)), flush=True)


if __name__ == "__main__":
    main()
