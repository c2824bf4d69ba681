#!/usr/bin/env python3
"""Generate tests/golden/g21_image_ref_grad.npz and g22_video_ref_grad_*.npz: the JOD and dJOD/dreference of the REAL reference's
torch-CPU autograd, run with BOTH inputs requiring grad (build container only: needs the reference source tree, imported as
tools/gen_golden.py does).

The inputs of every case are rebuilt from their description by tests/ref_grad_cases.py, so the files hold only outputs:
<case>_jod and <case>_gref (dJOD/dreference, [C, H, W] or [C, N, H, W]), rounded to 16 significant bits so that each file stays
below 1 MiB.  For every case that shares its inputs with g18 / g19 the generator asserts that the test gradient of the same run
equals the stored g18 / g19 gradient after the same rounding, and the JOD bit for bit: the generator and the old goldens
describe the same run.  Torch's CPU reductions depend on the thread count, so it is pinned to 8, the count the stored goldens
reproduce with.  For the clamp-coverage
cases the band pixels each clamp catches are counted on the CPU oracle's maps and printed; the L_bkg clamp and the test's
contrast clamp must bind in both, the reference's contrast clamp in the clip (in a still image it cannot: see
ref_grad_cases._dark_frame).

usage: tools/gen_golden_ref_grad.py [FILE.npz ...]      (the files to write; none: all of them)
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
import grad_cases as ic                                     # noqa: E402
import video_grad_cases as vc                               # noqa: E402
import ref_grad_cases as rc                                 # noqa: E402


def both_grads(pyfvvdp, test, ref, fps, padding, display, opt, gaze):
    """JOD, dJOD/dtest and dJOD/dreference of one [C, N, H, W] clip (N = 1, fps = 0: an image) through the reference's autograd."""
    kw = {}
    if "photometry" in opt:
        kw["display_photometry"] = pyfvvdp.fvvdp_display_photo_eotf(**opt["photometry"])
    fv = pyfvvdp.fvvdp(display_name=display, heatmap=None, device=torch.device("cpu"), foveated=bool(opt.get("foveated")),
                       temp_padding=padding, quiet=True, **kw)
    t = torch.tensor(test, requires_grad=True)
    r = torch.tensor(ref, requires_grad=True)
    fp = torch.tensor(gaze, dtype=torch.float32) if gaze is not None else None
    q, _ = fv.predict(t, r, dim_order="CFHW", frames_per_second=fps, fixation_point=fp)
    q.backward()
    return np.float32(q.item()), t.grad.numpy().astype(np.float32), r.grad.numpy().astype(np.float32)


THREADS = 8            # torch-CPU reductions split by thread: the count at which the stored g18 / g19 reproduce bit for bit


def same_run(name, jod, gt, stored_jod, stored_g):
    """The test gradient of this run (both inputs requiring grad) is the stored g18 / g19 golden of the same inputs."""
    assert float(jod) == stored_jod, (name, float(jod), stored_jod)
    assert np.array_equal(round_bits(gt), stored_g), name + ": the test gradient of this run is not the stored g18 / g19 one"


def report(name, shape, jod, g, t0, extra=""):
    print("%s: %s JOD %.5f  max|gref| %.3e  zeros %d%s  (%.1f s)" % (name, shape, jod, np.abs(g).max(), int((g == 0).sum()),
                                                                     extra, time.time() - t0), flush=True)


def check_clamps(name, need_r):
    n = rc.clamp_counts(name)
    print("%s: band pixels caught by the L_bkg clamp %d, the contrast clamp of t %d, of r %d" % (name, n["lbkg"], n["t"], n["r"]),
          flush=True)
    assert n["lbkg"] > 0 and n["t"] > 0, (name, n)
    assert (n["r"] > 0) == need_r, (name, n)


def main():
    pyfvvdp = import_reference()
    torch.set_num_threads(THREADS)
    only = set(sys.argv[1:])
    all_files = {rc.IMAGE_FILE} | set(rc.VIDEO_FILES.values())
    assert only <= all_files, only - all_files
    files = {}
    if not only or rc.IMAGE_FILE in only:
        for name, (C, H, W, display, opt) in rc.IMAGE_CASES.items():
            t0 = time.time()
            test, ref = rc.image_inputs(name)
            jod, gt, gr = both_grads(pyfvvdp, test[:, None], ref[:, None], 0, "replicate", display, opt, opt.get("fix"))
            gt, gr = gt[:, 0], gr[:, 0]
            assert np.isfinite(gr).all(), name
            if name in rc.SHARED_IMAGE:
                same_run(name, jod, gt, *ic.load_golden(name))
            if opt.get("dark"):
                check_clamps(name, need_r=False)
            out = files.setdefault(rc.IMAGE_FILE, {})
            out[name + "_jod"] = jod
            out[name + "_gref"] = round_bits(gr)
            report(name, test.shape, jod, gr, t0)
    for name, (C, N, H, W, fps, padding, display, opt) in rc.VIDEO_CASES.items():
        if only and rc.VIDEO_FILES[name] not in only:
            continue
        t0 = time.time()
        test, ref = rc.video_inputs(name)
        jod, gt, gr = both_grads(pyfvvdp, test, ref, fps, padding, display, opt, rc.video_gaze(name))
        assert np.isfinite(gr).all(), name
        if name in rc.SHARED_VIDEO:
            same_run(name, jod, gt, *vc.load_golden(name))
        if opt.get("dark"):
            check_clamps(name, need_r=True)
        out = files.setdefault(rc.VIDEO_FILES[name], {})
        out[name + "_jod"] = jod
        out[name + "_gref"] = round_bits(gr)
        zf = [int((gr[:, f] == 0).all()) for f in range(N)]
        report(name, test.shape, jod, gr, t0, "  all-zero frames %s" % zf)
    for fname, out in files.items():
        save(fname[:-4], out)
        assert os.path.getsize(os.path.join(OUT, fname)) < 1 << 20, fname


if __name__ == "__main__":
    main()
