#!/usr/bin/env python3
"""Generate tests/golden/g23_diff_map_grad_*.npz: the difference map of the REAL reference on torch-CPU before its float16
rounding and its detach, and the gradients of sum(W * map) with respect to the test through the reference's autograd (build
container only: needs the reference source tree, imported as tools/gen_golden.py does).

The reference forms the map one line before it detaches it, so the tool wraps fvvdp_lpyr_dec.reconstruct at run time, keeps the
value v it returns for every frame (still attached to the graph) and forms map = v^beta_jod |jod_a| itself; the linear map is v.
The inputs and the cotangent W >= 0 of every case are rebuilt from their description by tests/map_grad_cases.py, so the files
hold only outputs: <case>_map_jod, <case>_map_linear [N, H, W] and <case>_grad_jod, <case>_grad_linear [C, N, H, W], rounded to 16
significant bits (relative 8e-6, far below any tolerance) so that each file stays below 1 MiB.  v > 0 everywhere is asserted
for every case: the reference's gradient of the JOD-unit map is inf * 0 where v == 0.

usage: tools/gen_golden_diff_map.py [CASE ...]      (the cases to write; none: all of them)
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
from map_grad_cases import CASES, case_inputs, case_weights, golden_file   # noqa: E402


def ref_maps(pyfvvdp, test, ref, fps, padding, display, opt):
    """(test tensor with requires_grad, [v of frame 0, v of frame 1, ...] attached to its graph, the metric)."""
    import importlib
    cls = importlib.import_module("pyfvvdp.fvvdp_lpyr_dec").fvvdp_lpyr_dec
    kept = []
    plain = cls.reconstruct

    def keeping(self, bands):
        v = plain(self, bands)
        kept.append(v)
        return v

    fv = pyfvvdp.fvvdp(display_name=display, heatmap="raw", device=torch.device("cpu"), foveated=bool(opt.get("foveated")),
                       temp_padding=padding, quiet=True)
    t = torch.tensor(test, requires_grad=True)
    r = torch.tensor(ref)
    fp = torch.tensor(opt["fix"], dtype=torch.float32) if "fix" in opt else None
    cls.reconstruct = keeping
    try:
        fv.predict(t, r, dim_order="CFHW", frames_per_second=fps, fixation_point=fp)
    finally:
        cls.reconstruct = plain
    return t, kept, fv


def main():
    pyfvvdp = import_reference()
    only = set(sys.argv[1:])
    assert only <= set(CASES), only - set(CASES)
    for name, (C, N, H, W, fps, padding, display, opt) in CASES.items():
        if only and name not in only:
            continue
        t0 = time.time()
        test, ref = case_inputs(name)
        Wt = torch.from_numpy(case_weights(name))
        t, kept, fv = ref_maps(pyfvvdp, test, ref, fps, padding, display, opt)
        assert len(kept) == N, (name, len(kept))
        v = torch.stack([k.reshape(H, W) for k in kept])                      # [N, H, W]
        assert bool((v > 0).all()), "%s: v == 0 somewhere, the reference's gradient is not finite there" % name
        beta_jod = float(np.power(10.0, fv.log_jod_exp))
        maps = {"linear": v, "jod": torch.pow(v, beta_jod) * abs(float(fv.jod_a))}
        out = {}
        for units, m in maps.items():
            (g,) = torch.autograd.grad((Wt * m).sum(), t, retain_graph=True)
            g = g.numpy().astype(np.float32)
            assert np.isfinite(g).all(), (name, units)
            out["%s_map_%s" % (name, units)] = round_bits(m.detach().numpy().astype(np.float32))
            out["%s_grad_%s" % (name, units)] = round_bits(g)
            print("%s %s: map in [%.3e, %.3e]  max|g| %.3e  zeros %d" % (name, units, float(m.min()), float(m.max()),
                                                                       np.abs(g).max(), int((g == 0).sum())), flush=True)
        fname = golden_file(name)
        save(fname[:-4], out)
        size = os.path.getsize(os.path.join(OUT, fname))
        assert size < 1 << 20, (fname, size)
        print("%s: %s -> %s, %d bytes (%.1f s)" % (name, test.shape, fname, size, time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
