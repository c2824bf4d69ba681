#!/usr/bin/env python3
"""Per-pixel losses on the difference map (fvvdp.diff_map_images / diff_map_video): a region-of-interest loss and a top-k loss
on a small synthetic pair and clip, all on the GPU.

    python examples/ex_map_loss.py

The map is a [B, H, W] (images) or [N, H, W] (clip) fp32 tensor on the device with a grad_fn, so any torch expression on it
back-propagates into the caller's tensor.  The pooled JOD lets a small, strongly visible artefact hide in a large clean frame;
the top-k mean of the map does not.  units="linear" is the map before its power (beta_jod ~ 0.59 < 1): the derivative of the
JOD-unit map grows without bound where the map goes to 0, so a loss over nearly invisible regions is better conditioned there.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fovvideovdp_amd as pyfvvdp


def pattern(H, W, dev, phase=0.0):
    y, x = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    return torch.stack([0.5 + 0.3 * torch.sin(x / (9.0 + 4 * c) + phase) * torch.cos(y / 13.0) for c in range(3)])


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    H, W = 192, 256
    metric = pyfvvdp.fvvdp(display_name="standard_fhd", device=dev)

    # ---- a still pair: noise everywhere, one strong artefact; the mask covers the artefact's half of the image -------------
    ref = pattern(H, W, dev)[None]                                           # [1, 3, H, W]
    img = ref + 0.02 * torch.randn(ref.shape, device=dev, generator=g)
    img[:, :, 40:56, 60:76] += 0.25
    img = img.clamp(0, 1).requires_grad_(True)
    mask = torch.zeros((1, H, W), device=dev)
    mask[:, :, :W // 2] = 1.0
    opt = torch.optim.Adam([img], lr=4e-3)
    for step in range(30):
        opt.zero_grad()
        dmap = metric.diff_map_images(img, ref)                               # [1, H, W], JOD units
        roi = (mask * dmap).sum() / mask.sum()                                # region-of-interest loss
        topk = dmap.flatten().topk(256).values.mean()                         # the 256 worst pixels
        (roi + topk).backward()
        opt.step()
        with torch.no_grad():
            img.clamp_(0, 1)
        if step % 5 == 0:
            print("image step %2d  masked mean %.4f  top-256 mean %.4f  worst pixel %.4f" % (
                step, float(roi.detach()), float(topk.detach()), float(dmap.detach().max())))

    # ---- a clip: the same two losses on the linear map, per frame ----------------------------------------------------------
    N = 6
    refv = torch.stack([pattern(H, W, dev, 0.2 * f) for f in range(N)], dim=1)[None]      # [1, 3, N, H, W]
    vid = (refv + 0.03 * torch.randn(refv.shape, device=dev, generator=g)).clamp(0, 1).requires_grad_(True)
    # plain steps along the gradient, scaled by its largest entry (the transient channel couples the frames of a pixel: a step
    # that keeps the gradient's proportions does not trade noise for flicker)
    for step in range(15):
        vid.grad = None
        dmap = metric.diff_map_video(vid, refv, frames_per_second=30, units="linear")     # [N, H, W]
        roi = (mask * dmap).sum() / (N * mask.sum())
        topk = dmap.flatten(1).topk(64, dim=1).values.mean()                  # the 64 worst pixels of every frame
        (roi + 0.1 * topk).backward()
        with torch.no_grad():
            vid -= 2e-3 * vid.grad / vid.grad.abs().max()
            vid.clamp_(0, 1)
        if step % 5 == 0:
            print("clip  step %2d  masked mean %.4f  top-64 mean per frame %.4f" % (step, float(roi.detach()), float(topk.detach())))
    with torch.no_grad():
        print("final clip JOD %.4f" % float(metric.jod_video(vid, refv, frames_per_second=30)))


if __name__ == "__main__":
    main()
