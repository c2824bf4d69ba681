#!/usr/bin/env python3
"""jod_tests(...).sum().backward() against the loop of jod_video forward + backward calls, same process, alternated
("Gradients of many tests per reference").

Workload: T degraded copies of one synthetic clip against it, non-foveated standard_4k, float32 clips resident on the device.
For every T and every `wrt` the two ways of getting the gradient of sum_k JOD_k are timed in turns --
    loop:   T x jod_video(tests[k], ref, wrt=...).backward()      (with the reference differentiated autograd adds the T gradients)
    tests:  jod_tests(tests, ref, wrt=...).sum().backward()
-- `--reps` times each with HIP events around forward + backward, in `--runs` runs; the median and the spread (min .. max) of
the alternated readings are printed per run, with the peak device memory above the resident clips of either variant, one JSON
line per (T, wrt, run) and a summary line at the end.  The reference gradients are compared on the way (max|difference| /
max|gradient|).

    python tools/bench_tests_grad.py                                          # 1920x1080 x 60, T = 3 5 8
    python tools/bench_tests_grad.py --width 3840 --height 2160 --tests 3 5
    python tools/bench_tests_grad.py --tests 5 --wrt reference --reps 3 --runs 1    # e.g. under a profiler
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
from bench_gazes import timed                                   # noqa: E402

ONE = {"tests": "test", "reference": "reference", "both": "both"}      # jod_video's word for jod_tests' wrt


def degraded(ref, test, k):
    """Test k: the generator's noisy test, then the reference under seeded noise of growing amplitude."""
    if k == 0:
        return test
    g = torch.Generator(device=ref.device).manual_seed(100 + k)
    return (ref + (0.004 * k) * torch.randn(ref.shape, generator=g, device=ref.device)).clamp_(0, 1)


def peak_of(fn, base):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tests", type=int, nargs="+", default=[3, 5, 8])
    ap.add_argument("--wrt", nargs="+", default=["tests", "reference", "both"], choices=list(ONE))
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--display", default="standard_4k")
    args = ap.parse_args()
    N, H, W = args.frames, args.height, args.width
    t8, r8 = synth_video_pair(N, H, W, device="cuda")
    test, ref = t8.to(torch.float32) / 255, r8.to(torch.float32) / 255
    del t8, r8
    clips = [degraded(ref, test, k) for k in range(max(args.tests))]
    m = fv.fvvdp(display_name=args.display)
    rows = []
    for T in args.tests:
        for wrt in args.wrt:
            need_t, need_r = wrt != "reference", wrt != "tests"

            def leaves():
                return [c.detach().requires_grad_(need_t) for c in clips[:T]], ref.detach().requires_grad_(need_r)

            def loop():
                xs, y = leaves()
                for x in xs:
                    m.jod_video(x, y, frames_per_second=args.fps, wrt=ONE[wrt]).backward()
                return y.grad if need_r else xs[-1].grad

            def tests():
                xs, y = leaves()
                m.jod_tests(xs, y, frames_per_second=args.fps, wrt=wrt).sum().backward()
                return y.grad if need_r else xs[-1].grad

            loop()
            tests()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()            # the resident clips (and the metric's context)
            peak_loop, peak_tests = peak_of(loop, base), peak_of(tests, base)
            for run in range(args.runs):
                t_loop, t_tests = [], []
                for _ in range(args.reps):                  # alternated: both see the same state of the box
                    ms, g_loop = timed(loop)
                    t_loop.append(ms)
                    ms, g_tests = timed(tests)
                    t_tests.append(ms)
                rel = float((g_tests - g_loop).abs().max() / g_loop.abs().max())
                row = dict(T=T, wrt=wrt, run=run, frames=N, loop_ms=float(np.median(t_loop)), loop_ms_range=[min(t_loop), max(t_loop)],
                           tests_ms=float(np.median(t_tests)), tests_ms_range=[min(t_tests), max(t_tests)], rel_diff=rel,
                           peak_loop_gb=peak_loop / 1e9, peak_tests_gb=peak_tests / 1e9)
                row["speedup"] = row["loop_ms"] / row["tests_ms"]
                rows.append(row)
                print(json.dumps(row), flush=True)
    print(json.dumps(dict(tool="bench_tests_grad", width=W, height=H, frames=N, fps=args.fps, display=args.display,
                          reps=args.reps, runs=args.runs, rows=rows)), flush=True)


if __name__ == "__main__":
    main()
