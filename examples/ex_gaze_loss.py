#!/usr/bin/env python3
"""Optimise a clip for the expected quality over a grid of fixations (fvvdp.jod_gazes): a few steps of gradient ascent on the
mean JOD of a distorted clip under 3 x 3 gazes, all on the GPU, synthetic data.

    python examples/ex_gaze_loss.py

One backward serves all gazes: what does not depend on the gaze runs once.  The worst case over the grid is a loss as well
(`jods.min()`: the gradient of the gaze that is worst).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fovvideovdp_amd as pyfvvdp


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    N, H, W, fps = 8, 216, 384, 30
    f, y, x = torch.meshgrid(torch.arange(N, device=dev), torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    ref = torch.stack([0.5 + 0.3 * torch.sin((x + 3.0 * f) / (9.0 + 4 * c)) * torch.cos(y / 13.0) for c in range(3)], dim=-1)
    clip = (ref + 0.08 * torch.randn(ref.shape, device=dev, generator=g)).clamp(0, 1).requires_grad_(True)
    grid = np.float32([(gx, gy) for gy in (H * 0.2, H * 0.5, H * 0.8) for gx in (W * 0.2, W * 0.5, W * 0.8)])     # [9, 2]

    metric = pyfvvdp.fvvdp(display_name="standard_fhd", foveated=True, device=dev)
    opt = torch.optim.Adam([clip], lr=3e-3)
    for step in range(10):
        opt.zero_grad()
        jods = metric.jod_gazes(clip, ref, grid, dim_order="FHWC", frames_per_second=fps)      # [9]
        loss = (10.0 - jods).mean()
        loss.backward()
        opt.step()
        with torch.no_grad():
            clip.clamp_(0, 1)
        if step % 3 == 0:
            j = jods.detach()
            print("step %2d  mean JOD %.4f  worst %.4f (gaze %d)" % (step, float(j.mean()), float(j.min()), int(j.argmin())))
    with torch.no_grad():
        j = metric.jod_gazes(clip, ref, grid, dim_order="FHWC", frames_per_second=fps)
        print("final    mean JOD %.4f  worst %.4f" % (float(j.mean()), float(j.min())))


if __name__ == "__main__":
    main()
