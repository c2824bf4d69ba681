#!/usr/bin/env python3
"""Generate tests/golden/g2x_display_grad.npz from the REAL reference (build container only: needs the reference checkout).

The reference is imported as tools/gen_golden.py imports it and runs on torch-CPU in float32.  Its fvvdp_display_photo_eotf
takes its attributes as they come, so 0-d tensors that require grad make its own autograd differentiate the JOD for the
display's parameters.  For PQ the reference's `clip(0.005, tensor)` raises a TypeError, so Y_peak stays a float there and only
contrast, E_ambient and k_refl are recorded (the other entries are NaN).  The cases, their inputs and their display parameters
are those of tests/display_grad_ref.py.  Only recorded numbers are written: per case `<name>_jod` [pairs] and `<name>_grad`
[pairs, 5] (dJOD_k/dpsi, laid out as DISPLAY_PARAMETER_NAMES).

usage: tools/gen_golden_display_grad.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gen_golden import import_reference          # noqa: E402
import display_grad_ref as ref                    # noqa: E402


def main():
    pyfvvdp = import_reference()
    from pyfvvdp.fvvdp_display_model import fvvdp_display_geometry, fvvdp_display_photo_eotf
    out = {}
    for name in ref.GOLDEN_CASES:
        display, eotf, _, fov, C, N, fps, padding = ref.CASES[name]
        test, reference, gaze = ref.inputs(name)
        psi = ref.psi0(name)
        jods, grads = [], []
        for k in range(test.shape[0]):
            t = {n: torch.tensor(float(v), dtype=torch.float32, requires_grad=True) for n, v in zip(ref.NAMES, psi)}
            live = [n for n in ref.NAMES if not (eotf == "PQ" and n in ("Y_peak", "gamma"))]
            Yp = t["Y_peak"] if "Y_peak" in live else float(psi[0])
            ph = fvvdp_display_photo_eotf(Yp, contrast=t["contrast"], EOTF=eotf, gamma=t["gamma"], E_ambient=t["E_ambient"],
                                          k_refl=t["k_refl"])
            m = pyfvvdp.fvvdp(display_photometry=ph, display_geometry=fvvdp_display_geometry.load(display), foveated=fov,
                              temp_padding=padding, device=torch.device("cpu"))
            fix = None if gaze is None else torch.as_tensor(gaze)
            jod, _ = m.predict(torch.as_tensor(test[k:k + 1]), torch.as_tensor(reference[k:k + 1]), dim_order="BCFHW",
                               frames_per_second=fps, fixation_point=fix)
            jod.backward()
            g = np.full(len(ref.NAMES), np.nan)
            for i, n in enumerate(ref.NAMES):
                if n in live:
                    g[i] = 0.0 if t[n].grad is None else float(t[n].grad)
            jods.append(float(jod.detach()))
            grads.append(g)
            print(name, k, "JOD %.6f" % jods[-1], g)
        out[name + "_jod"] = np.asarray(jods, dtype=np.float64)
        out[name + "_grad"] = np.asarray(grads, dtype=np.float64)
    path = os.path.join(ROOT, "tests", "golden", "g2x_display_grad.npz")
    np.savez(path, **out)
    print("wrote", path)


if __name__ == "__main__":
    main()
