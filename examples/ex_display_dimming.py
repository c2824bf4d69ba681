#!/usr/bin/env python3
"""Content-adaptive dimming with the display's gradient (fvvdp.display_jod_video): the reference's brightness sweep
(ex_display_brightness.py rebuilds the metric once per peak luminance and plots JOD over brightness) as one gradient-driven
search for the peak luminance at which a clip's JOD meets a target.

    python examples/ex_display_dimming.py

The display's parameters are a vector psi laid out as fvvdp.DISPLAY_PARAMETER_NAMES; the metric is built once and never
rebuilt: every evaluation passes its psi.  Newton's method on ln Y_peak uses dJOD/dln Y_peak = Y_peak dJOD/dY_peak from
backward().  Which side of the crossing keeps the JOD above the target follows from the slope's sign: for noise-like distortions
the JOD falls as the display gets brighter (the distortion becomes visible), so the crossing is the brightest setting that still
meets the target; where the slope is positive it is the dimmest.  Synthetic data: a textured clip with additive noise.
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fovvideovdp_amd as pyfvvdp


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    N, H, W, fps = 12, 270, 480, 30
    ref = torch.rand((1, 3, N, H, W), device=dev, generator=g) * 0.6 + 0.2
    test = (ref + 0.03 * torch.randn((1, 3, N, H, W), device=dev, generator=g)).clamp(0, 1)

    metric = pyfvvdp.fvvdp(display_name="standard_fhd", device=dev)
    names = pyfvvdp.fvvdp.DISPLAY_PARAMETER_NAMES
    base = metric.display_parameter_tensor()
    i_peak = names.index("Y_peak")

    def jod_at(log_peak):
        psi = torch.cat([base[:i_peak], torch.exp(log_peak).reshape(1), base[i_peak + 1:]])
        return metric.display_jod_video(test, ref, psi, frames_per_second=fps)

    with torch.no_grad():
        j0 = float(jod_at(torch.log(base[i_peak])))
    target = j0 + 0.05                       # ask for a little more quality than the display gives at its own brightness
    print("JOD %.4f at the display's own %.0f cd/m^2; target %.4f" % (j0, float(base[i_peak]), target))

    lp = torch.log(base[i_peak]).clone()
    for it in range(12):
        lp = lp.detach().requires_grad_(True)
        j = jod_at(lp)
        j.backward()
        slope = float(lp.grad)
        print("step %2d  Y_peak %8.2f cd/m^2  JOD %.4f  dJOD/dln Y_peak %+.4f" % (it, math.exp(float(lp.detach())), float(j.detach()), slope))
        if abs(float(j.detach()) - target) < 1e-3 or slope == 0.0:
            break
        step = (target - float(j.detach())) / slope
        lp = lp.detach() + max(-1.0, min(1.0, step))        # at most a factor e per step
    side = "brightest" if slope < 0 else "dimmest"
    print("%s peak luminance with JOD >= %.4f: %.1f cd/m^2" % (side, target, math.exp(float(lp.detach()))))


if __name__ == "__main__":
    main()
