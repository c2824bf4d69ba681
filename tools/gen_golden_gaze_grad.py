#!/usr/bin/env python3
"""Generate tests/golden/g20_gaze_grad.npz: the JODs of one clip under three gazes and the gradient of their weighted sum
through the REAL reference's torch-CPU autograd (build container only: needs the reference source tree, imported as
tools/gen_golden.py does).

The inputs are rebuilt from their description by tests/gaze_grad_cases.py (a synthetic clip of fovvideovdp_amd.synth), so the
file holds only outputs: jod [3] and grad [C, N, H, W] = d(sum_g w_g JOD_g)/dtest, rounded to 16 significant bits (relative
8e-6, far below any tolerance).

usage: tools/gen_golden_gaze_grad.py
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
from gen_golden import OUT, import_reference, save          # noqa: E402
from gen_golden_grad import round_bits                      # noqa: E402
import gaze_grad_cases as gc                                # noqa: E402


def main():
    pyfvvdp = import_reference()
    test, ref = gc.case_inputs()
    gazes = gc.case_gazes()
    fv = pyfvvdp.fvvdp(display_name=gc.DISPLAY, heatmap=None, device=torch.device("cpu"), foveated=True,
                       temp_padding=gc.PADDING, quiet=True)
    t = torch.tensor(test, requires_grad=True)
    r = torch.tensor(ref)
    t0 = time.time()
    jods, loss = [], 0.0
    for g in range(len(gazes)):
        q, _ = fv.predict(t, r, dim_order="CFHW", frames_per_second=gc.FPS, fixation_point=torch.tensor(gazes[g]))
        jods.append(np.float32(q.item()))
        loss = loss + float(gc.WEIGHTS[g]) * q
    loss.backward()
    grad = t.grad.numpy().astype(np.float32)
    assert np.isfinite(grad).all()
    print("JOD %s  max|g| %.3e  (%.1f s)" % (jods, np.abs(grad).max(), time.time() - t0), flush=True)
    save("g20_gaze_grad", {"jod": np.asarray(jods, np.float32), "grad": round_bits(grad)})
    assert os.path.getsize(os.path.join(OUT, "g20_gaze_grad.npz")) < 1 << 20


if __name__ == "__main__":
    main()
