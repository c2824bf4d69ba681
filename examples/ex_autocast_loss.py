#!/usr/bin/env python3
"""The JOD as a loss under torch.autocast: a tiny convolutional net restores a noisy image, its float16 output goes to
fvvdp.jod_images as it is -- no .float() copy -- and the gradient comes back in float16.

    python examples/ex_autocast_loss.py

float16 gradients of a JOD are small, so the loss is scaled as usual (torch.amp.GradScaler): the scale multiplies in fp32 inside
the metric's backward, before the one rounding to float16.  With dtype=torch.bfloat16 no scaling is needed.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fovvideovdp_amd as pyfvvdp


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    H, W = 128, 192
    y, x = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    ref = torch.stack([0.5 + 0.3 * torch.sin(x / (9.0 + 4 * c)) * torch.cos(y / 13.0) for c in range(3)])[None]      # [1, 3, H, W]
    noisy = (ref + 0.08 * torch.randn_like(ref)).clamp(0, 1)

    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(8, 3, 3, padding=1)).to(dev)
    metric = pyfvvdp.fvvdp(display_name="standard_fhd", device=dev)
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    ref16 = ref.half()                       # the same dtype as the net's output: the half-precision kernels read both as they are
    for step in range(3):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.float16):
            out = noisy.half() + net(noisy)          # float16: what the convolutions emit under autocast
        assert out.dtype is torch.float16
        jod = metric.jod_images(out, ref16)  # fp32 [1]
        loss = (10.0 - jod).sum()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        print("step %d  JOD %.4f" % (step, float(jod[0].detach())))


if __name__ == "__main__":
    main()
