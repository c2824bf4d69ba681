#!/usr/bin/env python3
"""Generate tests/golden/g19_video_grad_*.npz: the video JOD and dJOD/dtest of the REAL reference's torch-CPU autograd (build
container only: needs the reference source tree, imported as tools/gen_golden.py does).

The inputs of every case are rebuilt from their description by tests/video_grad_cases.py (synthetic clips of
fovvideovdp_amd.synth), so the files hold only outputs: <case>_jod and <case>_grad (dJOD/dtest, [C, N, H, W]).  The gradients are
rounded to 16 significant bits (relative 8e-6, far below any tolerance) so that each file stays below 1 MiB.

usage: tools/gen_golden_video_grad.py [FILE.npz ...]      (the files to write; none: all of them)
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
from video_grad_cases import CASES, FILES, case_gaze, case_inputs, golden_frames   # noqa: E402


def ref_grad(pyfvvdp, test, ref, fps, padding, display, opt, gaze):
    """JOD and dJOD/dtest of one [C, N, H, W] clip through the reference's autograd."""
    kw = {}
    if "photometry" in opt:
        kw["display_photometry"] = pyfvvdp.fvvdp_display_photo_eotf(**opt["photometry"])
    fv = pyfvvdp.fvvdp(display_name=display, heatmap=None, device=torch.device("cpu"), foveated=bool(opt.get("foveated")),
                       temp_padding=padding, quiet=True, **kw)
    t = torch.tensor(test, requires_grad=True)
    r = torch.tensor(ref)
    fp = torch.tensor(gaze, dtype=torch.float32) if gaze is not None else None
    q, _ = fv.predict(t, r, dim_order="CFHW", frames_per_second=fps, fixation_point=fp)
    q.backward()
    return np.float32(q.item()), t.grad.numpy().astype(np.float32)


def main():
    pyfvvdp = import_reference()
    only = set(sys.argv[1:])
    assert only <= set(FILES.values()), only - set(FILES.values())
    files = {}
    for name, (C, N, H, W, fps, padding, display, opt) in CASES.items():
        if only and FILES[name] not in only:
            continue
        t0 = time.time()
        test, ref = case_inputs(name)
        jod, g = ref_grad(pyfvvdp, test, ref, fps, padding, display, opt, case_gaze(name))
        assert np.isfinite(g).all(), name
        out = files.setdefault(FILES[name], {})
        out[name + "_jod"] = jod
        frames = golden_frames(name)
        out[name + "_grad"] = round_bits(g if frames is None else np.ascontiguousarray(g[:, frames]))
        zf = [int((g[:, f] == 0).all()) for f in range(N)]
        print("%s: %s JOD %.5f  max|g| %.3e  zeros %d  all-zero frames %s  (%.1f s)" % (
            name, test.shape, jod, np.abs(g).max(), int((g == 0).sum()), zf, time.time() - t0), flush=True)
    for fname, out in files.items():
        save(fname[:-4], out)
        assert os.path.getsize(os.path.join(OUT, fname)) < 1 << 20, fname


if __name__ == "__main__":
    main()
