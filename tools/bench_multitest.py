#!/usr/bin/env python3
"""predict_tests against the loop of predict calls, same process, alternated ("Many tests per reference").

Workload: uint8 RGB clips behind standard_4k, inputs resident on the device, one reference and T degraded copies of it.  For
every T the two ways of scoring the T tests are timed in turns --
    loop:   T x predict(tests[k], ref, sync=False)
    tests:  predict_tests(tests, ref)
-- `--reps` times each with HIP events around the call; the medians, the spread (min .. max) of the alternated readings and
the time per test-frame are printed, one JSON line per T and a summary line at the end.  The whole series runs `--runs` times.
The results of both ways are compared bit for bit on the way; the first step that fails ends the tool (`--compare report`
counts the differing Q entries and their largest relative difference per T instead and goes on: a diagnostic).

    python tools/bench_multitest.py                                         # 3840x2160 x 60, T = 1 2 3 4 5 7 8
    python tools/bench_multitest.py --width 256 --height 256 --frames 16    # launch-bound
    python tools/bench_multitest.py --width 1920 --height 1080
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


def degraded(test, ref, k):
    """Test k: the generator's noisy test, then the reference under seeded noise of growing amplitude (made on the device)."""
    if k == 0:
        return test
    g = torch.Generator(device=ref.device).manual_seed(100 + k)
    noise = torch.randint(-2 * k, 2 * k + 1, ref.shape, generator=g, device=ref.device, dtype=torch.int16)
    return (ref.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tests", type=int, nargs="+", default=[1, 2, 3, 4, 5, 7, 8])
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--display", default="standard_4k")
    ap.add_argument("--compare", choices=["bits", "report"], default="bits")
    args = ap.parse_args()
    N, H, W = args.frames, args.height, args.width
    test, ref = synth_video_pair(N, H, W, device="cuda")
    clips = [degraded(test, ref, k) for k in range(max(args.tests))]
    m = fv.fvvdp(display_name=args.display)
    rows = []
    for run in range(args.runs):
        for T in args.tests:
            tests = clips[:T]

            def loop():
                return [m.predict(t, ref, frames_per_second=args.fps, sync=False) for t in tests]

            def many():
                return m.predict_tests(tests, ref, frames_per_second=args.fps)

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
            jod_same = all(torch.equal(res[k][0], q[k]) for k in range(T))
            same = jod_same and np.array_equal(Ql, st["Q_per_ch"])
            ne = Ql != st["Q_per_ch"]
            row = dict(run=run, T=T, frames=N, loop_ms=float(np.median(t_loop)), loop_ms_range=[min(t_loop), max(t_loop)],
                       tests_ms=float(np.median(t_many)), tests_ms_range=[min(t_many), max(t_many)],
                       loop_us_per_test_frame=1e3 * float(np.median(t_loop)) / (T * N),
                       tests_us_per_test_frame=1e3 * float(np.median(t_many)) / (T * N), bit_identical=bool(same), jod_identical=bool(jod_same),
                       q_entries_differing=int(ne.sum()), q_entries=int(ne.size), bands_differing=sorted(set(np.nonzero(ne)[1].tolist())),
                       q_max_relative=float((np.abs(Ql - st["Q_per_ch"]) / np.maximum(np.abs(Ql), 1e-30)).max()))
            row["speedup"] = row["loop_ms"] / row["tests_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            if not same and args.compare == "bits":
                print(json.dumps(dict(tool="bench_multitest", error="rows differ from predict at T=%d" % T)), flush=True)
                sys.exit(1)
    print(json.dumps(dict(tool="bench_multitest", width=W, height=H, frames=N, fps=args.fps, display=args.display, reps=args.reps,
                          runs=args.runs, rows=rows)), flush=True)


if __name__ == "__main__":
    main()
