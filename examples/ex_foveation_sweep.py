"""One reference render, five foveated variants of it, one moving gaze: a foveation sweep scored in one pass.

    python examples/ex_foveation_sweep.py

A foveated renderer or codec is tuned by comparing one full-quality reference with several foveated variants under the same gaze
trace.  fvvdp.predict_tests_foveated scores them at once on a foveated metric: the reference is ingested once per pair of tests
and everything of the pyramid pass that depends on the reference and the gaze only (the background luminance, the eccentricity,
the look-up of the CSF table) is computed once per group of tests; row k of its result is bit-identical to
predict(tests[k], reference, fixation_point=gaze).  Synthetic data: the periphery around the gaze is quantised the coarser the
stronger the setting (a stand-in for a lower shading rate); needs an AMD GPU."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fovvideovdp_amd as fv                                   # noqa: E402
from fovvideovdp_amd.synth import synth_video_pair              # noqa: E402


def foveate(ref, gaze, radius, step):
    """`ref` [1, C, N, H, W] uint8 with everything farther than `radius` pixels from the gaze of its frame quantised in `step`s."""
    _, _, N, H, W = ref.shape
    yy, xx = torch.meshgrid(torch.arange(H, device=ref.device), torch.arange(W, device=ref.device), indexing="ij")
    g = torch.as_tensor(gaze, device=ref.device)
    far = ((xx[None] - g[:, 0, None, None]) ** 2 + (yy[None] - g[:, 1, None, None]) ** 2) > radius ** 2          # [N, H, W]
    coarse = ((ref.to(torch.int16) // step) * step + step // 2).clamp(0, 255).to(torch.uint8)
    return torch.where(far[None, None], coarse, ref)


def main():
    N, H, W, fps = 24, 540, 960, 30
    _, ref = synth_video_pair(N, H, W, device="cuda")
    w = np.linspace(0.0, 1.0, N, dtype=np.float32)[:, None]
    gaze = np.float32([[0.2 * W, 0.3 * H]]) * (1 - w) + np.float32([[0.8 * W, 0.7 * H]]) * w        # [N, 2], frame pixels
    settings = ((400, 8), (300, 16), (200, 16), (150, 32), (100, 64))        # (radius of the full-quality region, step outside)
    tests = [foveate(ref, gaze, r, s) for r, s in settings]
    m = fv.fvvdp(display_name="standard_4k", foveated=True)
    m.predict_tests_foveated(tests, ref, frames_per_second=fps, fixation_point=gaze)      # warm-up: the context
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    jod, stats = m.predict_tests_foveated(tests, ref, frames_per_second=fps, fixation_point=gaze)
    t_tests = time.perf_counter() - t0
    t0 = time.perf_counter()
    loop = [m.predict(t, ref, frames_per_second=fps, fixation_point=gaze)[0] for t in tests]
    t_loop = time.perf_counter() - t0
    print("radius  step   JOD (predict_tests_foveated)   JOD (predict)")
    for (r, s), a, b in zip(settings, jod.cpu().tolist(), loop):
        print("%6d  %4d   %.6f                       %.6f" % (r, s, a, float(b)))
    print("Q_per_ch:", stats["Q_per_ch"].shape, "= [tests, bands, temporal channels, frames]; shared pass:", stats["shared_pass"])
    print("identical to the loop: %s; one pass %.1f ms, the loop %.1f ms" % (
        all(torch.equal(a, b) for a, b in zip(jod, loop)), 1e3 * t_tests, 1e3 * t_loop))


if __name__ == "__main__":
    main()
