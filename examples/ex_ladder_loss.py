#!/usr/bin/env python3
"""Train a pre-filter in front of a ladder of encoders (fvvdp.jod_tests, wrt="reference"): a few optimiser steps on the taps of a
3 x 3 filter applied to the source, scored against three fixed degradations of that source, all on the GPU, synthetic data.

    python examples/ex_ladder_loss.py

The filtered source is the REFERENCE of the call and the three degradations are its tests: one backward gives the gradient of the
mean JOD over the ladder with respect to the filtered source, and autograd carries it on into the taps.  What the reference's
backward has in common for the tests runs once.  With wrt="tests" the same call trains the three reconstructions instead, and
wrt="both" does both from one backward.
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fovvideovdp_amd as pyfvvdp


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    N, H, W, fps = 8, 216, 384, 30
    f, y, x = torch.meshgrid(torch.arange(N, device=dev), torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    src = torch.stack([0.5 + 0.3 * torch.sin((x + 3.0 * f) / (9.0 + 4 * c)) * torch.cos(y / 13.0) for c in range(3)])     # [3, N, H, W]
    src = (src + 0.03 * torch.randn(src.shape, device=dev, generator=g)).clamp(0, 1)

    def blur(v, times):
        for _ in range(times):
            v = F.avg_pool2d(F.pad(v, (1, 1, 1, 1), mode="replicate"), 3, stride=1)
        return v

    # three rungs of a ladder: what stronger and stronger low-pass "encoders" make of the source
    tests = [blur(src, k)[None].contiguous() for k in (1, 2, 4)]                  # each [1, 3, N, H, W]

    taps = torch.zeros((3, 3), device=dev)
    taps[1, 1] = 1.0                                                             # starts as the identity
    taps.requires_grad_(True)
    metric = pyfvvdp.fvvdp(display_name="standard_fhd", device=dev)
    opt = torch.optim.Adam([taps], lr=2e-2)
    for step in range(6):
        opt.zero_grad()
        k = (taps / taps.sum())[None, None]                                       # unit gain
        filtered = F.conv2d(F.pad(src.reshape(3 * N, 1, H, W), (1, 1, 1, 1), mode="replicate"), k).reshape(1, 3, N, H, W)
        jods = metric.jod_tests(tests, filtered, frames_per_second=fps, wrt="reference")          # [3]
        (10.0 - jods).mean().backward()
        opt.step()
        j = jods.detach()
        print("step %d  JOD per rung %s  mean %.4f" % (step, " ".join("%.4f" % q for q in j.tolist()), float(j.mean())))
    print("taps after training:\n%s" % (taps / taps.sum()).detach().cpu().numpy().round(3))


if __name__ == "__main__":
    main()
