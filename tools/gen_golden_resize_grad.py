#!/usr/bin/env python3
"""Generate tests/golden/g25_resize_grad_*.npz: the JOD of a test clip shown resized against a reference at the target size, and
dJOD/dtest at the test's own resolution, of the REAL reference's torch-CPU autograd (build container only: needs the reference
source tree, imported as tools/gen_golden_yuv_grad.py does).

The reference side is what a caller writes today: torch.nn.functional.interpolate(test, size, mode).clip(0, 1) into the
reference's predict(..., dim_order="CFHW"), then backward().  The inputs are rebuilt from their seeds by tests/resize_cases.py, so
the files hold only outputs: <case>_jod and <case>_grad [C, N, h, w], the gradient rounded to 16 significant bits.

usage: tools/gen_golden_resize_grad.py [FILE.npz ...]      (the files to write; none: all of them)
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
from resize_cases import CASES, FILES, case_gaze, case_inputs      # noqa: E402


def ref_grad(pyfvvdp, name):
    N, C, source, target, mode, display, fps, padding, opt = CASES[name]
    test, ref = case_inputs(name)
    kw = {}
    if "photometry" in opt:
        kw["display_photometry"] = pyfvvdp.fvvdp_display_photo_eotf(**opt["photometry"])
    fv = pyfvvdp.fvvdp(display_name=display, heatmap=None, device=torch.device("cpu"), foveated=bool(opt.get("foveated")),
                       temp_padding=padding, quiet=True, **kw)
    t = torch.tensor(np.ascontiguousarray(test), requires_grad=True)                   # [C, N, h, w]
    # interpolate takes [batch, channels, h, w]: the frames are the batch
    resized = torch.nn.functional.interpolate(t.permute(1, 0, 2, 3), size=(target[1], target[0]), mode=mode).clip(0, 1)
    gaze = case_gaze(name)
    fp = torch.tensor(gaze, dtype=torch.float32) if gaze is not None else None
    q, _ = fv.predict(resized.permute(1, 0, 2, 3), torch.tensor(np.ascontiguousarray(ref)), dim_order="CFHW", frames_per_second=fps,
                      fixation_point=fp)
    q.backward()
    return np.float32(q.item()), t.grad.numpy().astype(np.float32)


def main():
    pyfvvdp = import_reference()
    only = set(sys.argv[1:])
    assert only <= set(FILES.values()), only - set(FILES.values())
    largest_g24 = max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if f.startswith("g24_"))
    for name in CASES:
        if only and FILES[name] not in only:
            continue
        t0 = time.time()
        jod, g = ref_grad(pyfvvdp, name)
        assert np.isfinite(g).all(), name
        print("%s: JOD %.5f  max|grad| %.3e  zeros %d of %d  (%.1f s)" % (name, jod, np.abs(g).max(), int((g == 0).sum()), g.size,
                                                                         time.time() - t0), flush=True)
        save(FILES[name][:-4], {name + "_jod": jod, name + "_grad": round_bits(g)})
        assert os.path.getsize(os.path.join(OUT, FILES[name])) <= largest_g24, FILES[name]


if __name__ == "__main__":
    main()
