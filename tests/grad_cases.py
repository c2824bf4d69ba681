"""Inputs of the still-image gradient goldens (tests/golden/g18_image_grad*.npz), rebuilt from their description: the goldens
store only the reference's outputs.  Shared by tools/gen_golden_grad.py (which writes them) and the tests (which read them)."""
import os

import numpy as np

from fovvideovdp_amd.synth import synth_frame_pair

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name: (C, H, W, display_name, options)
CASES = {
    "a_gray_fhd": (1, 68, 121, "standard_fhd", {}),                          # odd sizes: both parities of the reduce quirk
    "b_rgb_4k_oob": (3, 135, 240, "standard_4k", {"oob": True}),             # some test samples outside [0, 1]
    "c_rgb_hdr_pq": (3, 90, 160, "standard_hdr_pq", {}),
    "d_gray_hdr_linear": (1, 90, 160, "standard_hdr_linear", {"scale": 400.0}),   # cd/m^2
    "e_rgb_gamma22": (3, 120, 200, "standard_4k",
                      {"photometry": dict(Y_peak=300.0, contrast=800.0, EOTF="gamma", gamma=2.2)}),
    "f_rgb_foveated": (3, 135, 240, "standard_4k", {"foveated": True, "fix": [170.0, 40.0]}),
    "g_identical": (3, 64, 96, "standard_4k", {"identical": True}),
    "h_g1_crop256": (3, 256, 256, "standard_fhd", {"g1": True}),             # 256x256 crop of the G1 content
}
# the file each case's outputs live in (each committed file stays below 1 MiB)
FILES = {"h_g1_crop256": "g18_image_grad_g1crop.npz"}
DEFAULT_FILE = "g18_image_grad.npz"


def case_inputs(name):
    """(test, reference) float32 [C, H, W] numpy arrays of one case."""
    C, H, W, _, opt = CASES[name]
    if opt.get("g1"):
        ref16 = np.load(os.path.join(GOLDEN, "g0_wavy_facade_blur_4k.npz"))["ref_u16"][85:597, 256:768]
        test16 = np.load(os.path.join(GOLDEN, "g1_crop512_blur_fhd.npz"))["test_u16"]
        crop = (slice(128, 384), slice(128, 384))
        t = (test16[crop].astype(np.float32) / np.float32(65535.0)).transpose(2, 0, 1)
        r = (ref16[crop].astype(np.float32) / np.float32(65535.0)).transpose(2, 0, 1)
        return np.ascontiguousarray(t), np.ascontiguousarray(r)
    seed = 100 + sorted(CASES).index(name)
    t8, r8 = synth_frame_pair(1, H, W, C=C, seed_ref=seed, seed_test=seed + 50)
    t = t8.numpy().astype(np.float32) / np.float32(255.0)
    r = r8.numpy().astype(np.float32) / np.float32(255.0)
    if opt.get("identical"):
        t = r.copy()
    if opt.get("oob"):
        t[:, 10:14, 20:60] = np.float32(1.15)
        t[C - 2, 100:104, 200:230] = np.float32(-0.1)
    if "scale" in opt:
        t, r = t * np.float32(opt["scale"]), r * np.float32(opt["scale"])
    return np.ascontiguousarray(t), np.ascontiguousarray(r)


def load_golden(name):
    """(jod, grad [C, H, W]) the reference computed for one case."""
    z = np.load(os.path.join(GOLDEN, FILES.get(name, DEFAULT_FILE)))
    return float(z[name + "_jod"]), z[name + "_grad"].astype(np.float32)
