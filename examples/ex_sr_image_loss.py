#!/usr/bin/env python3
"""Train a tiny single-image super-resolution "network" on mini-batches of stills with the metric as its loss
(fvvdp.jod_images_resized): a 3x3 convolution per channel, started as a mild blur, learns to sharpen half-resolution images so that
their bicubic full-screen upscale looks like the full-resolution references, all on the GPU.

    python examples/ex_sr_image_loss.py

No image at the display's resolution ever exists on the test side: the metric resizes inside its ingest kernel (torch's interpolate
arithmetic, then the clip to [0, 1] and the display model), and backward() brings grad[k] dJOD_k/d(network output) back at the
network's own resolution through the adjoint of the resize.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fovvideovdp_amd as pyfvvdp


def main():
    dev = torch.device("cuda:0")
    B, H, W = 8, 192, 256
    k, y, x = torch.meshgrid(torch.arange(B, device=dev), torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    lum = 0.5 + 0.35 * torch.sin((x + 11.0 * k) / (1.5 + 0.25 * k)) * torch.cos(y / (2.0 + 0.25 * k))
    ref_full = torch.stack((lum, 0.9 * lum + 0.05, 1.0 - lum), 1).contiguous()             # [B, 3, H, W], the full-resolution stills
    x_small = torch.nn.functional.avg_pool2d(ref_full, 2)                                   # [B, 3, H/2, W/2]: what the network sees

    kernels = torch.full((3, 1, 3, 3), 0.05, device=dev)                                    # a mild blur: the untrained network
    kernels[:, 0, 1, 1] = 0.6
    kernels.requires_grad_(True)

    def net(x):
        return torch.nn.functional.conv2d(x, kernels, padding=1, groups=3)                  # [B, 3, H/2, W/2]

    metric = pyfvvdp.fvvdp(display_name="standard_fhd", device=dev)
    opt = torch.optim.Adam([kernels], lr=5e-3)
    kw = dict(full_screen_resize="bicubic", resize_resolution=(W, H))
    with torch.no_grad():
        print("before   mean JOD %.4f" % float(metric.jod_images_resized(net(x_small), ref_full, **kw).mean()))
    for step in range(40):
        opt.zero_grad()
        jod = metric.jod_images_resized(net(x_small), ref_full, **kw)
        (10.0 - jod.mean()).backward()
        opt.step()
        if step % 5 == 0:
            print("step %2d  mean JOD %.4f" % (step, float(jod.detach().mean())))
    with torch.no_grad():
        print("after    mean JOD %.4f" % float(metric.jod_images_resized(net(x_small), ref_full, **kw).mean()))


if __name__ == "__main__":
    main()
