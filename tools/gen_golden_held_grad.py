#!/usr/bin/env python3
"""Generate tests/golden/g26_held_grad.npz: the JOD of a test clip shown by sample-and-hold against a reference at the display's
rate, and dJOD/dtest at the test's own frame count, of the REAL reference's torch-CPU autograd (build container only: needs the
reference source tree, imported as tools/gen_golden_resize_grad.py does).

The reference side is what a caller writes today: test.index_select(frames, m_t) and reference.index_select(frames, m_r) into the
reference's predict(..., dim_order="CFHW"), then backward() -- torch adds the gradients of the copies back together.  The inputs
are rebuilt from their seeds by tests/held_cases.py, so the file holds only outputs: <case>_jod and <case>_grad [C, F_t, H, W], the
gradient rounded to 16 significant bits.
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
from held_cases import GOLDEN_CASES, GOLDEN_FILE, case_gaze, case_inputs, case_maps      # noqa: E402


def ref_grad(pyfvvdp, name):
    (W, H), C, fps, padding, dtype, ts, rs, N, opt = GOLDEN_CASES[name]
    test, ref = case_inputs(name)
    m_t, F_t, m_r, F_r = case_maps(name)
    fv = pyfvvdp.fvvdp(display_name=opt.get("display", "standard_fhd"), heatmap=None, device=torch.device("cpu"),
                       foveated=bool(opt.get("foveated")), temp_padding=padding, quiet=True)
    t = torch.tensor(np.ascontiguousarray(test), requires_grad=True)                   # [C, F_t, H, W]
    r = torch.tensor(np.ascontiguousarray(ref))
    gaze = case_gaze(name)
    fp = torch.tensor(gaze, dtype=torch.float32) if gaze is not None else None
    q, _ = fv.predict(t.index_select(1, torch.as_tensor(m_t, dtype=torch.int64)), r.index_select(1, torch.as_tensor(m_r, dtype=torch.int64)),
                      dim_order="CFHW", frames_per_second=fps, fixation_point=fp)
    q.backward()
    return np.float32(q.item()), t.grad.numpy().astype(np.float32)


def main():
    pyfvvdp = import_reference()
    largest_g25 = max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if f.startswith("g25_"))
    out = {}
    for name in GOLDEN_CASES:
        t0 = time.time()
        jod, g = ref_grad(pyfvvdp, name)
        assert np.isfinite(g).all(), name
        print("%s: JOD %.5f  max|grad| %.3e  zeros %d of %d  (%.1f s)" % (name, jod, np.abs(g).max(), int((g == 0).sum()), g.size,
                                                                         time.time() - t0), flush=True)
        out[name + "_jod"] = jod
        out[name + "_grad"] = round_bits(g)
    save(GOLDEN_FILE[:-4], out)
    assert os.path.getsize(os.path.join(OUT, GOLDEN_FILE)) <= largest_g25, GOLDEN_FILE


if __name__ == "__main__":
    main()
