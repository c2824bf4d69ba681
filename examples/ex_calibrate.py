#!/usr/bin/env python3
"""Fit model parameters to quality scores (fvvdp.calibration_jod_images): synthetic "subjective" JODs are made under perturbed
parameters, then a few Adam steps on those parameters bring the loss down, all gradients from the GPU.

    python examples/ex_calibrate.py

The parameter vector is laid out as fvvdp.PARAMETER_NAMES and lives on the host; the metric's own attributes are never touched
(metric.set_parameters(theta) would adopt a fitted vector).  A real calibration replaces the synthetic scores by a dataset's.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fovvideovdp_amd as pyfvvdp


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    B, H, W = 8, 256, 384
    ref = torch.randint(0, 256, (B, 3, H, W), device=dev, generator=g, dtype=torch.uint8)       # calibration sets are 8-bit
    noise = torch.randn((B, 3, H, W), device=dev, generator=g) * torch.linspace(2.0, 24.0, B, device=dev).view(B, 1, 1, 1)
    test = (ref.float() + noise).round().clamp(0, 255).to(torch.uint8)

    metric = pyfvvdp.fvvdp(display_name="standard_fhd", device=dev)
    names = pyfvvdp.fvvdp.PARAMETER_NAMES
    theta0 = metric.parameter_tensor()
    fit = [names.index(n) for n in ("mask_c", "sensitivity_correction", "beta_sch")]

    truth = theta0.clone()
    truth[fit] += torch.tensor([-0.2, 1.5, 0.1], dtype=torch.float64)
    scores = metric.calibration_jod_images(test, ref, truth)                                   # the "subjective" data

    phi = theta0[fit].clone().requires_grad_(True)
    opt = torch.optim.Adam([phi], lr=0.05)
    for step in range(40):
        opt.zero_grad()
        theta = theta0.clone().index_put((torch.tensor(fit),), phi)
        loss = ((metric.calibration_jod_images(test, ref, theta) - scores) ** 2).mean()
        loss.backward()
        opt.step()
        if step % 5 == 0:
            print("step %2d  loss %.3e  %s" % (step, float(loss.detach()), ", ".join("%s %.4f" % (names[i], float(v)) for i, v in zip(fit, phi.detach()))))
    print("target            %s" % ", ".join("%s %.4f" % (names[i], float(truth[i])) for i in fit))


if __name__ == "__main__":
    main()
