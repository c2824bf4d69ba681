#!/usr/bin/env python3
"""Generate tests/golden/g26_images_resize_grad_*.npz: the JODs of a stack of test images shown resized against reference images
that may be resized too, and the gradients at each stack's own resolution, of the REAL reference's torch-CPU autograd (build
container only: needs the reference source tree, imported as tools/gen_golden_resize_grad.py does).

The reference side is what a caller writes today: torch.nn.functional.interpolate(x, size, mode).clip(0, 1) on each stack that
is resized, into the reference's predict(..., dim_order="CHW"), one call per pair, sum_k (k + 1) JOD_k, then backward().  The
inputs are rebuilt from their seeds by tests/images_resize_cases.py, so the files hold only outputs: <case>_jod [B] and
<case>_grad_test / <case>_grad_reference, the gradients of the sides the case differentiates, rounded to 16 significant bits.

usage: tools/gen_golden_images_resize_grad.py [FILE.npz ...]      (the files to write; none: all of them)
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
from images_resize_cases import CASES, FILES, WEIGHTS, case_gaze, case_inputs      # noqa: E402


def shown(x, target, mode):
    """A stack [B, C, h, w] as the caller resizes it today; one of the target's size is clipped like the other."""
    if (x.shape[3], x.shape[2]) != tuple(target):
        x = torch.nn.functional.interpolate(x, size=(target[1], target[0]), mode=mode)
    return x.clip(0, 1)


def ref_grad(pyfvvdp, name):
    C, tsize, rsize, target, mode, display, wrt, opt = CASES[name]
    test, ref = case_inputs(name)
    kw = {}
    if "photometry" in opt:
        kw["display_photometry"] = pyfvvdp.fvvdp_display_photo_eotf(**opt["photometry"])
    fv = pyfvvdp.fvvdp(display_name=display, heatmap=None, device=torch.device("cpu"), foveated=bool(opt.get("foveated")),
                       quiet=True, **kw)
    t = torch.tensor(np.ascontiguousarray(test), requires_grad=wrt in ("test", "both"))
    r = torch.tensor(np.ascontiguousarray(ref), requires_grad=wrt in ("reference", "both"))
    ts, rs = shown(t, target, mode), shown(r, target, mode)
    gaze = case_gaze(name)
    jods = []
    for k in range(t.shape[0]):
        fp = torch.tensor(gaze[k], dtype=torch.float32) if gaze is not None else None
        q, _ = fv.predict(ts[k], rs[k], dim_order="CHW", frames_per_second=0, fixation_point=fp)
        jods.append(q.reshape(()))
    jod = torch.stack(jods)
    (jod * torch.from_numpy(WEIGHTS)).sum().backward()
    return jod.detach().numpy().astype(np.float32), {k: x.grad.numpy().astype(np.float32)
                                                     for k, x in (("test", t), ("reference", r)) if x.grad is not None}


def main():
    pyfvvdp = import_reference()
    only = set(sys.argv[1:])
    assert only <= set(FILES.values()), only - set(FILES.values())
    largest_g25 = max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if f.startswith("g25_"))
    for name in CASES:
        if only and FILES[name] not in only:
            continue
        t0 = time.time()
        jod, grads = ref_grad(pyfvvdp, name)
        out = {name + "_jod": jod}
        for k, g in grads.items():
            assert np.isfinite(g).all(), (name, k)
            print("%s: d/d%s max|grad| %.3e  zeros %d of %d" % (name, k, np.abs(g).max(), int((g == 0).sum()), g.size), flush=True)
            out[name + "_grad_" + k] = round_bits(g)
        print("%s: JOD %s  (%.1f s)" % (name, jod, time.time() - t0), flush=True)
        save(FILES[name][:-4], out)
        assert os.path.getsize(os.path.join(OUT, FILES[name])) <= largest_g25, FILES[name]


if __name__ == "__main__":
    main()
