#!/usr/bin/env python3
"""predict_tests_foveated against the loop of predict calls under the same gaze, same process, alternated (DESIGN.md section 4,
"Many tests per reference under a gaze").

Workload: uint8 RGB clips behind standard_4k, foveated, a gaze that moves across the frame, inputs resident on the device, one
reference and T degraded copies of it.  For every T the two ways of scoring the T tests are timed in turns --
    loop:   T x predict(tests[k], ref, fixation_point=gaze, sync=False)
    tests:  predict_tests_foveated(tests, ref, fixation_point=gaze)
-- `--reps` times each with HIP events around the call; the medians, the spread (min .. max) of the alternated readings and
the time per test-frame are printed, one JSON line per T and a summary line at the end.  The whole series runs `--runs` times
(the largest T first, so that every step runs in the scratch of the largest context).  The results of both ways are compared
bit for bit on the way; the first step that differs ends the tool.  FVVDP_TESTS_GROUP=2 in the environment caps the launch
groups at two quads (the A/B of the three-quad kernel).

    python tools/bench_tests_fov.py                                         # 3840x2160 x 60, T = 1 2 3 5 8
    python tools/bench_tests_fov.py --width 256 --height 256 --frames 16    # launch-bound
    python tools/bench_tests_fov.py --width 1920 --height 1080
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
from bench_multitest import degraded, timed                     # noqa: E402


def moving_gaze(N, H, W):
    """[N, 2]: from the upper left quarter to the lower right corner and a little beyond it."""
    w = np.linspace(0.0, 1.0, N, dtype=np.float32)[:, None]
    return np.ascontiguousarray(np.float32([[0.25 * W, 0.25 * H]]) * (1 - w) + np.float32([[W + 20, H + 20]]) * w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tests", type=int, nargs="+", default=[1, 2, 3, 5, 8])
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--display", default="standard_4k")
    args = ap.parse_args()
    N, H, W = args.frames, args.height, args.width
    test, ref = synth_video_pair(N, H, W, device="cuda")
    clips = [degraded(test, ref, k) for k in range(max(args.tests))]
    gaze = moving_gaze(N, H, W)
    m = fv.fvvdp(display_name=args.display, foveated=True)
    rows = []
    for run in range(args.runs):
        for T in sorted(args.tests, reverse=True):
            tests = clips[:T]

            def loop():
                return [m.predict(t, ref, frames_per_second=args.fps, fixation_point=gaze, sync=False) for t in tests]

            def many():
                return m.predict_tests_foveated(tests, ref, frames_per_second=args.fps, fixation_point=gaze)

            many()                                          # the larger context first: the loop then runs in the same scratch
            loop()
            torch.cuda.synchronize()
            t_loop, t_many = [], []
            for _ in range(args.reps):                      # alternated: both see the same state of the box
                ms, res = timed(loop)
                t_loop.append(ms)
                ms, (q, st) = timed(many)
                t_many.append(ms)
            Ql = np.stack([res[k][1]["Q_per_ch"].cpu().numpy() for k in range(T)])
            same = all(torch.equal(res[k][0], q[k]) for k in range(T)) and np.array_equal(Ql, st["Q_per_ch"])
            row = dict(run=run, T=T, frames=N, shared_pass=bool(st["shared_pass"]), group_cap=os.environ.get("FVVDP_TESTS_GROUP", ""),
                       loop_ms=float(np.median(t_loop)), loop_ms_range=[min(t_loop), max(t_loop)],
                       tests_ms=float(np.median(t_many)), tests_ms_range=[min(t_many), max(t_many)],
                       loop_us_per_test_frame=1e3 * float(np.median(t_loop)) / (T * N),
                       tests_us_per_test_frame=1e3 * float(np.median(t_many)) / (T * N), bit_identical=bool(same))
            row["speedup"] = row["loop_ms"] / row["tests_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            if not same:
                print(json.dumps(dict(tool="bench_tests_fov", error="rows differ from predict at T=%d" % T)), flush=True)
                sys.exit(1)
    print(json.dumps(dict(tool="bench_tests_fov", width=W, height=H, frames=N, fps=args.fps, display=args.display, reps=args.reps,
                          runs=args.runs, rows=rows)), flush=True)


if __name__ == "__main__":
    main()
