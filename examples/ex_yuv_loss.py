#!/usr/bin/env python3
"""Train a post-filter on 4:2:0 planes against the JOD of its output (fvvdp.jod_video_yuv): a 3x3 convolution per plane, started
as the identity, is optimised to undo the noise of a "decoded" clip, all on the GPU.

    python examples/ex_yuv_loss.py

The planes are limited-range 8-bit code values as floats (Y in [16, 235]); the metric unpacks them exactly as it unpacks a .yuv file,
inside its ingest kernel, and backward() reaches the filter's weights through dJOD/dY, dJOD/dU and dJOD/dV.  The reference is the
integer clip.
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
    luma = (126 + 80 * torch.sin((x + 3.0 * f) / 9.0) * torch.cos(y / 13.0)).round()
    cb = (128 + 40 * torch.sin((x + 2.0 * f) / 23.0))[:, ::2, ::2].round()
    cr = (128 + 40 * torch.cos(y / 17.0 + f / 5.0))[:, ::2, ::2].round()
    ref = tuple(p.to(torch.uint8) for p in (luma, cb, cr))                                  # the codes of the source clip
    decoded = [p + 6.0 * torch.randn(p.shape, device=dev, generator=g) for p in (luma, cb, cr)]

    filters = []
    for _ in range(3):
        k = torch.zeros((1, 1, 3, 3), device=dev)
        k[0, 0, 1, 1] = 1.0
        filters.append(k.requires_grad_(True))

    def post_filter():
        return tuple(torch.nn.functional.conv2d(p[:, None], k, padding=1)[:, 0] for p, k in zip(decoded, filters))

    metric = pyfvvdp.fvvdp(display_name="standard_fhd", device=dev)
    opt = torch.optim.Adam(filters, lr=2e-2)
    for step in range(30):
        opt.zero_grad()
        jod = metric.jod_video_yuv(post_filter(), ref, frames_per_second=fps)
        (10.0 - jod).backward()
        opt.step()
        if step % 5 == 0:
            print("step %2d  JOD %.4f" % (step, float(jod.detach())))
    with torch.no_grad():
        print("final    JOD %.4f" % float(metric.jod_video_yuv(post_filter(), ref, frames_per_second=fps)))


if __name__ == "__main__":
    main()
