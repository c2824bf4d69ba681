#!/usr/bin/env python3
"""A ladder rung that halves resolution AND frame rate -- 30 frames of 128x96 shown full screen on a 60 Hz panel -- scored against
the full-rate, full-size reference, with one optimiser step on the rung (fvvdp.jod_video_resized with test_frames=), all on the GPU.

    python examples/ex_rung_loss.py

Neither the resized nor the repeated version of the rung ever exists: the ingest reads the small clip through its frame map,
interpolates a held frame once, and backward() brings dJOD/dtest back at the rung's own 30 frames of 128x96 -- the luminance
gradient is summed over the two display frames that show a frame before the resize's adjoint runs.  What callers wrote before,
test.repeat_interleave(2, dim=frames) into jod_video_resized, builds a clip twice as long, interpolates every frame twice and runs
the resize's adjoint twice as often.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fovvideovdp_amd as pyfvvdp


def main():
    dev = torch.device("cuda:0")
    N, k, H, W, fps = 60, 2, 192, 256, 60
    f, y, x = torch.meshgrid(torch.arange(N, device=dev), torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    lum = 0.5 + 0.35 * torch.sin((x + 1.5 * f) / 5.0) * torch.cos(y / 7.0)                  # a pattern that moves 1.5 px per refresh
    ref = torch.stack((lum, 0.9 * lum + 0.05, 1.0 - lum))[None].contiguous()               # [1, 3, 60, H, W]
    # the rung: every second frame at half the size, the best an encoder could pick without looking at the metric
    rung = torch.nn.functional.interpolate(ref[0, :, ::k].permute(1, 0, 2, 3), size=(H // 2, W // 2), mode="area")
    test = rung.permute(1, 0, 2, 3)[None].contiguous().requires_grad_(True)                 # [1, 3, 30, H / 2, W / 2]

    metric = pyfvvdp.fvvdp(display_name="standard_fhd", device=dev)
    kw = dict(full_screen_resize="bilinear", resize_resolution=(W, H), frames_per_second=fps, test_frames=k)
    opt = torch.optim.Adam([test], lr=5e-3)
    opt.zero_grad()
    jod = metric.jod_video_resized(test, ref, **kw)
    (10.0 - jod).backward()
    opt.step()
    with torch.no_grad():
        test.clamp_(0.0, 1.0)
        q, stats = metric.predict_resized(test, ref, **kw)
    print("rung %dx%d @ %d fps on %dx%d @ %d Hz:  JOD %.4f -> %.4f after one step  (gradient shape %s, display frames %d)"
          % (W // 2, H // 2, fps // k, W, H, fps, float(jod.detach()), float(q), tuple(test.grad.shape), stats["N_frames"]))


if __name__ == "__main__":
    main()
