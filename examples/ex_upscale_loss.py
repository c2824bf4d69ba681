#!/usr/bin/env python3
"""Train a tiny "network" whose output has HALF the resolution the metric judges at (fvvdp.jod_video_resized): a 3x3 convolution
per channel, started as the identity, sharpens a half-resolution clip so that its bicubic full-screen upscale looks like the
full-resolution reference, all on the GPU.

    python examples/ex_upscale_loss.py

The clip at the display's resolution never exists: the metric resizes inside its ingest kernel (torch's interpolate arithmetic, then
the clip to [0, 1] and the display model), and backward() brings dJOD/d(network output) back at the network's own resolution
through the adjoint of the resize.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fovvideovdp_amd as pyfvvdp


def main():
    dev = torch.device("cuda:0")
    N, H, W, fps = 12, 192, 256, 30
    f, y, x = torch.meshgrid(torch.arange(N, device=dev), torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    lum = 0.5 + 0.35 * torch.sin((x + 3.0 * f) / 5.0) * torch.cos(y / 7.0)
    ref = torch.stack((lum, 0.9 * lum + 0.05, 1.0 - lum))[None].contiguous()               # [1, 3, N, H, W], the full-resolution clip
    small = torch.nn.functional.avg_pool2d(ref[0], 2)                                       # [3, N, H/2, W/2]: what the network sees

    kernels = torch.zeros((3, 1, 3, 3), device=dev)
    kernels[:, 0, 1, 1] = 1.0
    kernels.requires_grad_(True)

    def network():
        out = torch.nn.functional.conv2d(small.permute(1, 0, 2, 3), kernels, padding=1, groups=3)      # [N, 3, H/2, W/2]
        return out.permute(1, 0, 2, 3)[None]                                                # [1, 3, N, H/2, W/2], no copy

    metric = pyfvvdp.fvvdp(display_name="standard_fhd", device=dev)
    opt = torch.optim.Adam([kernels], lr=2e-2)
    kw = dict(full_screen_resize="bicubic", resize_resolution=(W, H), frames_per_second=fps)
    for step in range(30):
        opt.zero_grad()
        jod = metric.jod_video_resized(network(), ref, **kw)
        (10.0 - jod).backward()
        opt.step()
        if step % 5 == 0:
            print("step %2d  JOD %.4f" % (step, float(jod.detach())))
    with torch.no_grad():
        print("final    JOD %.4f" % float(metric.jod_video_resized(network(), ref, **kw)))


if __name__ == "__main__":
    main()
