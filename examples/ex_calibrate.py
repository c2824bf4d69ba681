#!/usr/bin/env python3
"""Fit model parameters to quality scores (fvvdp.calibration_jod_images): synthetic "subjective" JODs are made under perturbed
parameters, then a few Adam steps on those parameters bring the loss down, all gradients from the GPU.

    python examples/ex_calibrate.py

The parameter vector is laid out as fvvdp.PARAMETER_NAMES and lives on the host; the metric's own attributes are never touched
(metric.set_parameters(theta) would adopt a fitted vector).  A real calibration replaces the synthetic scores by a dataset's.

The second part re-fits the two parameters of the temporal filters, sustained_sigma and sustained_beta
(fvvdp.TEMPORAL_PARAMETER_NAMES), on two short clips with fvvdp.calibration_jod_video(temporal=phi).
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
    fit_temporal(metric, dev, g)


def fit_temporal(metric, dev, g):
    """sustained_sigma and sustained_beta from the JODs of three clips that flicker at different temporal frequencies (10, 3 and
    2 Hz: one frequency would pin only one direction of the plane); the steps are taken on ln phi (both are positive)."""
    tnames = pyfvvdp.fvvdp.TEMPORAL_PARAMETER_NAMES
    N, H, W = 12, 128, 192
    t = torch.arange(N, device=dev).view(1, 1, N, 1, 1)
    clips = []
    for fps, period in ((30, 3.0), (30, 10.0), (60, 30.0)):
        ref = torch.rand((1, 1, N, H, W), device=dev, generator=g) * 0.5 + 0.25
        flicker = 0.06 * torch.sin(2 * torch.pi * t / period) * torch.rand((1, 1, 1, H, W), device=dev, generator=g)
        clips.append(((ref + flicker).clamp(0, 1), ref, fps))
    theta = metric.parameter_tensor()
    # a nearby truth: over a wider range the JOD of a flickering clip is not monotone in sustained_beta (the filter's peak moves
    # across the flicker frequency), and a least-squares fit from far away can stop in a local minimum
    truth = metric.temporal_parameter_tensor() * torch.tensor([1.06, 0.95], dtype=torch.float64)
    scores = [metric.calibration_jod_video(a, b, theta, frames_per_second=fps, temporal=truth) for a, b, fps in clips]
    psi = torch.log(metric.temporal_parameter_tensor()).requires_grad_(True)
    opt = torch.optim.Adam([psi], lr=0.005)
    for step in range(80):
        opt.zero_grad()
        phi = torch.exp(psi)
        loss = sum((metric.calibration_jod_video(a, b, theta, frames_per_second=fps, temporal=phi) - s) ** 2
                   for (a, b, fps), s in zip(clips, scores))
        loss.backward()
        opt.step()
        if step % 10 == 0:
            print("step %2d  loss %.3e  %s" % (step, float(loss.detach()), ", ".join("%s %.4f" % (n, float(v)) for n, v in zip(tnames, phi.detach()))))
    print("target            %s" % ", ".join("%s %.4f" % (n, float(v)) for n, v in zip(tnames, truth)))


if __name__ == "__main__":
    main()
