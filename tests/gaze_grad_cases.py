"""Inputs of the many-gaze gradient golden (tests/golden/g20_gaze_grad.npz), rebuilt from their description: the golden stores
only the reference's outputs.  Shared by tools/gen_golden_gaze_grad.py (which writes it) and tests/test_gpu_gaze_grad.py
(which reads it).  Also the numpy restatement of the per-gaze CSF query of gaze_layer_kernel (tests/test_gaze_grad_cpu.py)."""
import os

import numpy as np

from fovvideovdp_amd.synth import synth_gaze, synth_video_pair

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_gaze_grad.npz")

# one clip: gray, 6 frames of 68 x 121 at 30 frames per second, `replicate` padding, foveated standard_4k
C, N, H, W, FPS, PADDING, DISPLAY = 1, 6, 68, 121, 30, "replicate", "standard_4k"
SEED = 420
WEIGHTS = np.asarray([1.0, -0.5, 2.0], np.float32)          # the loss is sum_g WEIGHTS[g] * JOD_g


def case_inputs():
    """(test, reference) float32 [C, N, H, W] numpy arrays."""
    t8, r8 = synth_video_pair(N, H, W, C=C, seed_ref=SEED, seed_test=SEED + 50)
    t = t8[0].numpy().astype(np.float32) / np.float32(255.0)
    r = r8[0].numpy().astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(t), np.ascontiguousarray(r)


def case_gazes():
    """[3, N, 2]: the corner (0, 0), the moving gaze of synth_gaze, and a point 500 pixels outside the frame."""
    g = np.empty((3, N, 2), np.float32)
    g[0] = (0, 0)
    g[1] = synth_gaze(N, H, W).numpy()
    g[2] = (W + 499, H + 499)
    return g


def load_golden():
    """(JOD [3], gradient of the weighted sum [C, N, H, W]) the reference computed."""
    z = np.load(GOLDEN_FILE)
    return z["jod"].astype(np.float32), z["grad"].astype(np.float32)


def s_query(lut, rho, lbkg, ecc, dtype=np.float64):
    """S_log of gaze_layer_kernel's CSF query for arrays of (rho, L_bkg, eccentricity): clamp, interval from the uniform grid,
    fraction from the stored knots with the + 1e-6 of the reference, rho blend in slope form, then Y, then ecc.
    lut: {"S_log" [Y, rho, ecc], "Y_log", "rho_log", "ecc_sqrt"} as fvvdp.csf_lut holds them."""
    S = np.asarray(lut["S_log"], dtype)
    ax = [np.asarray(lut[k], dtype).ravel() for k in ("Y_log", "rho_log", "ecc_sqrt")]
    n = len(ax[0])
    q = [np.log2(np.clip(np.asarray(lbkg, dtype), 2.0 ** ax[0][0], 2.0 ** ax[0][-1])),
         np.log2(np.clip(np.asarray(rho, dtype), 2.0 ** ax[1][0], 2.0 ** ax[1][-1])),
         np.sqrt(np.clip(np.asarray(ecc, dtype), ax[2][0] ** 2, ax[2][-1] ** 2))]
    k, f = [], []
    for a, x in zip(ax, q):
        inv_step = dtype(n - 1) / (a[-1] - a[0])
        ki = np.clip(np.floor((x - a[0]) * inv_step).astype(np.int64), 0, n - 2)
        k.append(ki)
        f.append(np.maximum((x - a[ki]) * (1.0 / (a[ki + 1] - a[ki] + dtype(1e-6))), 0.0))
    (kY, kR, kE), (fY, fR, fE) = k, f

    def r(dy, de):
        v, w = S[kY + dy, kR, kE + de], S[kY + dy, kR + 1, kE + de]
        return v + (w - v) * fR
    return (r(0, 0) * (1 - fY) + r(1, 0) * fY) * (1 - fE) + (r(0, 1) * (1 - fY) + r(1, 1) * fY) * fE
