#!/usr/bin/env python3
"""Generate tests/golden/g18_image_grad.npz and g18_image_grad_g1crop.npz: the still-image JOD and dJOD/dtest of the REAL
reference's torch-CPU autograd (build container only: needs the reference source tree, imported as tools/gen_golden.py does).

The inputs of every case are rebuilt from their description by tests/grad_cases.py (synthetic pairs of fovvideovdp_amd.synth,
the G1 content of goldens g0 / g1), so the files hold only outputs: <case>_jod and <case>_grad (dJOD/dtest, [C, H, W]).  The
gradients are rounded to 16 significant bits (relative 8e-6, far below any tolerance) so that each file stays below 1 MiB.

usage: tools/gen_golden_grad.py
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
from grad_cases import CASES, DEFAULT_FILE, FILES, case_inputs   # noqa: E402


def round_bits(a, bits=16):
    """fp32 rounded to `bits` significant bits (round half away from zero on the integer image; zeros stay exactly 0)."""
    u = a.astype(np.float32).view(np.uint32).astype(np.uint64)
    drop = 24 - bits
    u = ((u + (1 << (drop - 1))) >> drop) << drop
    return u.astype(np.uint32).view(np.float32)


def ref_grad(pyfvvdp, test, ref, display, opt):
    """JOD and dJOD/dtest of one [C, H, W] pair through the reference's autograd."""
    kw = {}
    if "photometry" in opt:
        kw["display_photometry"] = pyfvvdp.fvvdp_display_photo_eotf(**opt["photometry"])
    fv = pyfvvdp.fvvdp(display_name=display, heatmap=None, device=torch.device("cpu"), foveated=bool(opt.get("foveated")),
                       quiet=True, **kw)
    t = torch.tensor(test[:, None], requires_grad=True)          # [C, F=1, H, W]
    r = torch.tensor(ref[:, None])
    fp = torch.tensor(opt["fix"], dtype=torch.float32) if "fix" in opt else None
    q, _ = fv.predict(t, r, dim_order="CFHW", frames_per_second=0, fixation_point=fp)
    q.backward()
    return np.float32(q.item()), t.grad[:, 0].numpy().astype(np.float32)


def main():
    pyfvvdp = import_reference()
    files = {}
    for name, (C, H, W, display, opt) in CASES.items():
        t0 = time.time()
        test, ref = case_inputs(name)
        jod, g = ref_grad(pyfvvdp, test, ref, display, opt)
        out = files.setdefault(FILES.get(name, DEFAULT_FILE), {})
        out[name + "_jod"] = jod
        out[name + "_grad"] = round_bits(g)
        print("%s: %s JOD %.5f  max|g| %.3e  zeros %d  (%.1f s)" % (name, test.shape, jod, np.abs(g).max(), int((g == 0).sum()),
                                                                  time.time() - t0), flush=True)
    for fname, out in files.items():
        save(fname[:-4], out)
        assert os.path.getsize(os.path.join(OUT, fname)) < 1 << 20, fname


if __name__ == "__main__":
    main()
