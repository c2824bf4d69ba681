"""Quality as a function of where you look: the JOD of one clip under a 5 x 3 grid of fixations, in one pass.

    python examples/ex_gaze_grid.py

A foveated metric scores a (test, reference) clip for ONE gaze trace.  fvvdp.predict_gazes scores it for many at once -- the
temporal channels and everything of the pyramid pass that does not depend on the gaze are computed once per group of gazes --
and row g of its result is bit-identical to predict(..., fixation_point=fixation_points[g]).  Synthetic data; needs an AMD GPU."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fovvideovdp_amd as fv                                   # noqa: E402
from fovvideovdp_amd.synth import synth_video_pair              # noqa: E402


def main():
    N, H, W, fps = 12, 540, 960, 30
    test, ref = synth_video_pair(N, H, W, device="cuda")
    # distort the right half only: looking there should cost more quality than looking left
    test = test.clone()
    test[..., W // 2:] = (test[..., W // 2:].to(torch.int16) // 24 * 24).to(torch.uint8)
    xs = np.linspace(0, W - 1, 5)
    ys = np.linspace(0, H - 1, 3)
    grid = np.array([[x, y] for y in ys for x in xs], dtype=np.float32)          # [15, 2], one fixed gaze per row
    m = fv.fvvdp(display_name="standard_4k", foveated=True)
    jod, stats = m.predict_gazes(test, ref, grid, frames_per_second=fps)
    jod = jod.cpu().numpy().reshape(len(ys), len(xs))
    print("JOD by fixation (rows: y = %s; columns: x = %s)" % (ys.round().astype(int).tolist(), xs.round().astype(int).tolist()))
    for row in jod:
        print("  " + "  ".join("%6.3f" % v for v in row))
    print("Q_per_ch:", stats["Q_per_ch"].shape, "= [gazes, bands, temporal channels, frames]")
    # the same number as one predict call with that gaze
    q, _ = m.predict(test, ref, frames_per_second=fps, fixation_point=grid[7])
    print("centre: predict_gazes %.6f, predict %.6f" % (jod[1, 2], float(q)))


if __name__ == "__main__":
    main()
