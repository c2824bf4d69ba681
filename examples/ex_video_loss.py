#!/usr/bin/env python3
"""Use the video JOD as a differentiable loss (fvvdp.jod_video): pull a distorted clip towards its reference by gradient ascent
on its JOD, all on the GPU.

    python examples/ex_video_loss.py

The gradient reaches the caller's own tensor (here a leaf of shape [F, H, W, 3] in "FHWC" order).  The reference is a constant.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fovvideovdp_amd as pyfvvdp


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    N, H, W, fps = 12, 192, 256, 30
    f, y, x = torch.meshgrid(torch.arange(N, device=dev), torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    ref = torch.stack([0.5 + 0.3 * torch.sin((x + 3.0 * f) / (9.0 + 4 * c)) * torch.cos(y / 13.0) for c in range(3)], dim=-1)
    clip = (ref + 0.08 * torch.randn(ref.shape, device=dev, generator=g)).clamp(0, 1).requires_grad_(True)

    metric = pyfvvdp.fvvdp(display_name="standard_fhd", device=dev)
    opt = torch.optim.Adam([clip], lr=3e-3)
    for step in range(30):
        opt.zero_grad()
        jod = metric.jod_video(clip, ref, dim_order="FHWC", frames_per_second=fps)
        loss = 10.0 - jod
        loss.backward()
        opt.step()
        with torch.no_grad():
            clip.clamp_(0, 1)
        if step % 5 == 0:
            print("step %2d  JOD %.4f" % (step, float(jod.detach())))
    with torch.no_grad():
        print("final    JOD %.4f" % float(metric.jod_video(clip, ref, dim_order="FHWC", frames_per_second=fps)))


if __name__ == "__main__":
    main()
