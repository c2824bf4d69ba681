#!/usr/bin/env python3
"""Generate tests/golden/g24_yuv_grad_*.npz: the JOD of a planar YUV clip and dJOD/d(Y, U, V) of the REAL reference's torch-CPU
autograd (build container only: needs the reference source tree, imported as tools/gen_golden.py does).

The reference's own unpack takes numpy and is not differentiable, so display-encoded RGB is made from the float planes with the
torch ops of fvvdp_video_source_yuv_frames.unpack (pinned against the reference's unpack by tests/test_host_cpu.py); the
reference's predict(..., dim_order="CFHW") runs on the result and backward() goes into the planes.  The inputs are rebuilt from
their seeds by tests/yuv_grad_cases.py, so the files hold only outputs: <case>_jod, <case>_dy, <case>_du, <case>_dv, the gradients
rounded to 16 significant bits.

usage: tools/gen_golden_yuv_grad.py [FILE.npz ...]      (the files to write; none: all of them)
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
from yuv_grad_cases import CASES, FILES, case_gaze, case_inputs, split      # noqa: E402

from fovvideovdp_amd.video_source_yuv import YCBCR2RGB      # noqa: E402


def unpack_rgb(Y, U, V, bit_depth, chroma_ss, color_space):
    """fvvdp_video_source_yuv_frames.unpack on planes of one clip: [N, H, W] + 2 x [N, uvh, uvw] -> RGB [3, N, H, W] in [0, 1]."""
    sc = 2 ** (bit_depth - 8)
    Yf = torch.clip(Y * (1 / (sc * 219)) - 16 / 219, 0, 1)
    uv = torch.clip(torch.stack((U, V), 1) * (1 / (sc * 224)) - 128 / 224, -0.5, 0.5)          # [N, 2, uvh, uvw]
    if chroma_ss == "420":
        uv = torch.nn.functional.interpolate(uv, scale_factor=2, mode='bilinear')
    Yuv = torch.cat((Yf[:, None], uv), 1).permute(0, 2, 3, 1)                                   # [N, H, W, 3]
    M = torch.tensor(YCBCR2RGB["bt2020nc" if color_space == "bt2020nc" else "bt709"], dtype=torch.float32)
    return (Yuv @ M.transpose(1, 0)).clip(0, 1).permute(3, 0, 1, 2)


def ref_grad(pyfvvdp, name):
    N, H, W, bd, css, cs, display, fps, padding, opt = CASES[name]
    test, ref = case_inputs(name)
    kw = {}
    if "photometry" in opt:
        kw["display_photometry"] = pyfvvdp.fvvdp_display_photo_eotf(**opt["photometry"])
    fv = pyfvvdp.fvvdp(display_name=display, heatmap=None, device=torch.device("cpu"), foveated=bool(opt.get("foveated")),
                       temp_padding=padding, quiet=True, color_space="BT.2020" if cs == "bt2020nc" else "sRGB", **kw)
    planes = [torch.tensor(np.ascontiguousarray(p), requires_grad=True) for p in split(test, H, W, css)]
    rplanes = [torch.tensor(np.ascontiguousarray(p.astype(np.float32))) for p in split(ref, H, W, css)]
    gaze = case_gaze(name)
    fp = torch.tensor(gaze, dtype=torch.float32) if gaze is not None else None
    q, _ = fv.predict(unpack_rgb(*planes, bd, css, cs), unpack_rgb(*rplanes, bd, css, cs).detach(), dim_order="CFHW",
                      frames_per_second=fps, fixation_point=fp)
    q.backward()
    grads = [np.zeros(p.shape, np.float32) if p.grad is None else p.grad.numpy().astype(np.float32) for p in planes]
    return np.float32(q.item()), grads


def main():
    pyfvvdp = import_reference()
    only = set(sys.argv[1:])
    assert only <= set(FILES.values()), only - set(FILES.values())
    files = {}
    for name in CASES:
        if only and FILES[name] not in only:
            continue
        t0 = time.time()
        jod, g = ref_grad(pyfvvdp, name)
        assert all(np.isfinite(x).all() for x in g), name
        out = files.setdefault(FILES[name], {})
        out[name + "_jod"] = jod
        for p, x in zip("yuv", g):
            out[name + "_d" + p] = round_bits(x)
        print("%s: JOD %.5f  max|dY| %.3e  max|dU| %.3e  max|dV| %.3e  zeros %d  (%.1f s)" % (
            name, jod, np.abs(g[0]).max(), np.abs(g[1]).max(), np.abs(g[2]).max(), sum(int((x == 0).sum()) for x in g),
            time.time() - t0), flush=True)
    for fname, out in files.items():
        save(fname[:-4], out)
        assert os.path.getsize(os.path.join(OUT, fname)) < 1 << 20, fname


if __name__ == "__main__":
    main()
