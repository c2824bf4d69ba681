#!/usr/bin/env python3
"""predict_gazes against the loop of predict calls, same process, alternated ("Many gazes per clip").

Workload: the geometry of bench.py --config 3 (3840x2160, foveated, standard_hdr_pq, moving gaze) on a shorter clip, inputs
resident on the device.  For every G the two ways of scoring the clip under G gaze traces are timed in turns --
    loop:   G x predict(test, ref, fixation_point=trace[g], sync=False)
    gazes:  predict_gazes(test, ref, traces)
-- `--reps` times each with HIP events around the call; the medians, the spread (min .. max) of the alternated readings and
the time per gaze-frame are printed, one JSON line per G and a summary line at the end.  The results of both ways are compared
bit for bit on the way.

    python tools/bench_gazes.py                       # G = 1 2 4 8 16 32, 30 frames at 120 fps
    python tools/bench_gazes.py --gazes 16 --reps 7
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


def traces(G, N, H, W, seed=1):
    """G gaze traces [G, N, 2]: each drifts linearly between two seeded points of the frame."""
    rng = np.random.RandomState(seed)
    a = rng.uniform(0, 1, (G, 1, 2)) * [W - 1, H - 1]
    b = rng.uniform(0, 1, (G, 1, 2)) * [W - 1, H - 1]
    w = np.linspace(0.0, 1.0, N)[None, :, None]
    return np.ascontiguousarray(a * (1 - w) + b * w, dtype=np.float32)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gazes", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32])
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--fps", type=float, default=120.0)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--display", default="standard_hdr_pq")
    args = ap.parse_args()
    N, H, W = args.frames, args.height, args.width
    test, ref = synth_video_pair(N, H, W, device="cuda")
    m = fv.fvvdp(display_name=args.display, foveated=True)
    rows = []
    for G in args.gazes:
        fp = traces(G, N, H, W)

        def loop():
            return [m.predict(test, ref, frames_per_second=args.fps, fixation_point=fp[g], sync=False) for g in range(G)]

        def gazes():
            return m.predict_gazes(test, ref, fp, frames_per_second=args.fps)

        loop()
        gazes()
        torch.cuda.synchronize()
        t_loop, t_gaze = [], []
        for _ in range(args.reps):                      # alternated: both see the same state of the box
            ms, res = timed(loop)
            t_loop.append(ms)
            ms, (q, st) = timed(gazes)
            t_gaze.append(ms)
        same = all(torch.equal(res[g][0], q[g]) and np.array_equal(res[g][1]["Q_per_ch"].cpu().numpy(), st["Q_per_ch"][g])
                   for g in range(G))
        row = dict(G=G, frames=N, loop_ms=float(np.median(t_loop)), loop_ms_range=[min(t_loop), max(t_loop)],
                   gazes_ms=float(np.median(t_gaze)), gazes_ms_range=[min(t_gaze), max(t_gaze)],
                   loop_us_per_gaze_frame=1e3 * float(np.median(t_loop)) / (G * N),
                   gazes_us_per_gaze_frame=1e3 * float(np.median(t_gaze)) / (G * N), bit_identical=bool(same))
        row["speedup"] = row["loop_ms"] / row["gazes_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(dict(tool="bench_gazes", width=W, height=H, frames=N, fps=args.fps, display=args.display, reps=args.reps,
                          rows=rows)), flush=True)


if __name__ == "__main__":
    main()
