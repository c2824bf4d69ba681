"""One reference, five degradations of it: the rungs of a bitrate ladder scored in one pass.

    python examples/ex_bitrate_ladder.py

A full-reference metric is mostly run as one reference against many tests -- the same source through several codecs, presets or
bitrates.  fvvdp.predict_tests scores them at once: the reference is ingested once per pair of tests and everything of the
pyramid pass that depends on the reference only is computed once per group of tests; row k of its result is
bit-identical to predict(tests[k], reference).  Synthetic data (coarser and coarser quantisation stands in for the codec); needs an AMD GPU."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fovvideovdp_amd as fv                                   # noqa: E402
from fovvideovdp_amd.synth import synth_video_pair              # noqa: E402


def main():
    N, H, W, fps = 24, 540, 960, 30
    _, ref = synth_video_pair(N, H, W, device="cuda")
    steps = (4, 8, 16, 32, 64)                                   # quantisation step of every rung, finest first
    tests = [((ref.to(torch.int16) // s) * s + s // 2).clamp(0, 255).to(torch.uint8) for s in steps]
    m = fv.fvvdp(display_name="standard_4k")
    m.predict_tests(tests, ref, frames_per_second=fps)           # warm-up: the context
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    jod, stats = m.predict_tests(tests, ref, frames_per_second=fps)
    t_tests = time.perf_counter() - t0
    t0 = time.perf_counter()
    loop = [m.predict(t, ref, frames_per_second=fps)[0] for t in tests]
    t_loop = time.perf_counter() - t0
    print("step   JOD (predict_tests)   JOD (predict)")
    for s, a, b in zip(steps, jod.cpu().tolist(), loop):
        print("%4d   %.6f              %.6f" % (s, a, float(b)))
    print("Q_per_ch:", stats["Q_per_ch"].shape, "= [tests, bands, temporal channels, frames]")
    print("identical to the loop: %s; one pass %.1f ms, the loop %.1f ms" % (
        all(torch.equal(a, b) for a, b in zip(jod, loop)), 1e3 * t_tests, 1e3 * t_loop))


if __name__ == "__main__":
    main()
