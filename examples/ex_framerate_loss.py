#!/usr/bin/env python3
"""Optimise a 15-frame clip that is shown at 60 Hz -- every frame held for four display refreshes -- against a 60-frame reference
(fvvdp.jod_video_held), all on the GPU.

    python examples/ex_framerate_loss.py

The 60-frame version of the test clip never exists: the metric's ingest reads each stream through its frame map, and backward()
brings dJOD/dtest back at the test's own 15 frames -- the sum over the four display frames that show a frame is taken inside the
last kernel of the backward.  What callers wrote before, test.repeat_interleave(4, dim=frames) into jod_video, builds a clip four
times the size and a gradient of the same size that torch then adds back together.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fovvideovdp_amd as pyfvvdp


def main():
    dev = torch.device("cuda:0")
    N, k, H, W, fps = 60, 4, 192, 256, 60
    f, y, x = torch.meshgrid(torch.arange(N, device=dev), torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    lum = 0.5 + 0.35 * torch.sin((x + 1.5 * f) / 5.0) * torch.cos(y / 7.0)                  # a pattern that moves 1.5 px per refresh
    ref = torch.stack((lum, 0.9 * lum + 0.05, 1.0 - lum))[None].contiguous()               # [1, 3, 60, H, W]
    # start from the reference sampled at every fourth frame: the best a 15 fps renderer could pick without looking at the metric
    test = ref[:, :, ::k].clone().requires_grad_(True)                                      # [1, 3, 15, H, W]

    metric = pyfvvdp.fvvdp(display_name="standard_fhd", device=dev)
    opt = torch.optim.Adam([test], lr=5e-3)
    kw = dict(frames_per_second=fps, test_frames=k)
    for step in range(30):
        opt.zero_grad()
        jod = metric.jod_video_held(test, ref, **kw)
        (10.0 - jod).backward()
        opt.step()
        with torch.no_grad():
            test.clamp_(0.0, 1.0)
        if step % 5 == 0:
            print("step %2d  JOD %.4f" % (step, float(jod.detach())))
    with torch.no_grad():
        q, _ = metric.predict_held(test, ref, **kw)
        print("final    JOD %.4f   (gradient shape %s, display frames %d)" % (float(q), tuple(test.grad.shape), N))


if __name__ == "__main__":
    main()
