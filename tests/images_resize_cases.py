"""Shapes and inputs of the mixed-resolution still-image tests (tests/test_images_resize_cpu.py, tests/test_gpu_images_resize.py)
and of the goldens tests/golden/g26_images_resize_grad_*.npz, rebuilt from fixed seeds: the goldens store only the reference's
outputs.  Shared by tools/gen_golden_images_resize_grad.py (which writes them) and the tests (which read them).

The sizes are resize_cases.py's and the stacks are drawn by its draw_clip with the frame axis as B, so they carry samples on both
sides of [0, 1] with the margin that module describes.  Stacks are [B, C, h, w] here."""
import os

import numpy as np

import resize_cases as rc
import resize_ref as rref

GOLDEN = rc.GOLDEN
B = 3
TARGETS = rc.TARGETS
SOURCES = rc.SOURCES
DISPLAYS = rc.DISPLAYS

# (mode, C, source, target, the reference's sample type, its size (None: the target's), display).  Every mode at both channel
# counts; the reference at the target's size, at the test's and at a third; nearest has the x0.5 source, the one mode whose
# downscale skips samples.  The last case has the TEST at the target's size and the reference resized.
_TABLE = [
    ("nearest", 3, (240, 136), (120, 68), "float32", None, "standard_fhd"),
    ("bilinear", 3, (60, 34), (122, 68), "uint8", (60, 34), "standard_hdr_pq"),
    ("bicubic", 3, (80, 46), (120, 68), "float32", (40, 23), "gamma2.4"),
    ("area", 3, (240, 136), (122, 68), "uint8", None, "standard_fhd"),
    ("nearest", 1, (40, 23), (122, 68), "uint8", (121, 67), "standard_hdr_pq"),
    ("bilinear", 1, (121, 67), (120, 68), "float32", None, "gamma2.4"),
    ("bicubic", 1, (7, 5), (122, 68), "uint8", (7, 5), "standard_fhd"),
    ("area", 1, (60, 34), (120, 68), "float32", (240, 136), "standard_hdr_pq"),
    ("bilinear", 3, (120, 68), (120, 68), "float32", (60, 34), "gamma2.4"),
]


def rotation():
    """Entries: dict(mode, source, target, C, ref_dtype, ref_source (None: the reference has the target's size), display)."""
    return [dict(mode=m, C=C, source=s, target=t, ref_dtype=rd, ref_source=rs, display=d) for m, C, s, t, rd, rs, d in _TABLE]


def case_id(c):
    return "%s-%dx%d-to-%dx%d-C%d-%s-ref-%s%s" % (c["mode"], *c["source"], *c["target"], c["C"], c["display"], c["ref_dtype"],
                                                  "" if c["ref_source"] is None else "-%dx%d" % c["ref_source"])


_ROTATION = {}


def rotation_inputs(c):
    """(test float32 [B, C, h, w], reference [B, C, hr, wr] of the case's sample type) of one rotation case; computed once and left
    unchanged."""
    key = case_id(c)
    if key not in _ROTATION:
        seed = [26, rref.MODES.index(c["mode"]), c["C"], *c["source"], *c["target"]]
        test, _ = rc.draw_clip(seed, c["C"], B, c["source"], c["target"], c["mode"])
        ref, _ = rc.draw_clip(seed + [1], c["C"], B, c["ref_source"] or c["target"], c["target"], c["mode"], c["ref_dtype"])
        test, ref = np.ascontiguousarray(test.transpose(1, 0, 2, 3)), np.ascontiguousarray(ref.transpose(1, 0, 2, 3))
        test.setflags(write=False)
        ref.setflags(write=False)
        _ROTATION[key] = (test, ref)
    return _ROTATION[key]


# ---- the goldens ------------------------------------------------------------------------------------------------------------------
# name: (C, test size, reference size, target, mode, display_name, wrt, options)
CASES = {
    "a_bilinear_x2_srgb_test": (3, (60, 34), (120, 68), (120, 68), "bilinear", "standard_fhd", "test", {}),
    "b_bicubic_x1p5_pq_both": (3, (80, 46), (60, 34), (120, 68), "bicubic", "standard_hdr_pq", "both", {}),
    "c_area_down_gamma_reference": (3, (120, 68), (240, 136), (120, 68), "area", "standard_4k", "reference",
                                    {"photometry": dict(Y_peak=300.0, contrast=800.0, EOTF="gamma", gamma=2.2)}),
    "d_nearest_x3_gray_fov": (1, (40, 23), (120, 68), (120, 68), "nearest", "standard_4k", "test",
                              {"foveated": True, "gaze": [[30.0, 20.0], [60.0, 34.0], [100.0, 50.0]]}),
}
FILES = {name: "g26_images_resize_grad_%d.npz" % (i + 1) for i, name in enumerate(CASES)}
# (seeds are kept clear of a band pixel on the d_max clamp: see the finding recorded in yuv_grad_cases.py)
SEEDS = {"a_bilinear_x2_srgb_test": 2600, "b_bicubic_x1p5_pq_both": 2601, "c_area_down_gamma_reference": 2602,
         "d_nearest_x3_gray_fov": 2603}
WEIGHTS = np.arange(1, B + 1, dtype=np.float32)          # the loss is sum_k (k + 1) JOD_k
_INPUTS = {}


def case_inputs(name):
    """(test float32 [B, C, h, w], reference float32 [B, C, h', w']) of one golden case; computed once and left unchanged.  The
    stack that is drawn (draw_clip: out-of-range samples, with the margin) is the one the case resizes and differentiates -- the
    reference in case c, the test in the others.  The other stack is the drawn one resized and clipped plus noise, so the JODs are
    neither 10 nor at the floor; where it has a size of its own (case b) it is that image resized once more (bilinear) and kept
    inside [0.1, 0.9], where no interpolation of it reaches a clip."""
    if name not in _INPUTS:
        C, tsize, rsize, target, mode = CASES[name][:5]
        drawn_is_ref = tsize == target
        drawn, _ = rc.draw_clip([SEEDS[name]], C, B, rsize if drawn_is_ref else tsize, target, mode)
        rng = np.random.default_rng([SEEDS[name], 26])
        other = np.clip(rref.resize(drawn.astype(np.float64), target, mode), 0, 1)
        other = np.clip(other + rng.normal(0, 0.05, other.shape), 0, 1)
        osize = tsize if drawn_is_ref else rsize
        if osize != target:
            other = 0.1 + 0.8 * np.clip(rref.resize(other, osize, "bilinear"), 0, 1)
        drawn, other = (np.ascontiguousarray(x.transpose(1, 0, 2, 3).astype(np.float32)) for x in (drawn, other))
        drawn.setflags(write=False)
        other.setflags(write=False)
        _INPUTS[name] = (other, drawn) if drawn_is_ref else (drawn, other)
    return _INPUTS[name]


def case_gaze(name):
    """One gaze per pair [B, 2] in target pixels of a foveated case (None otherwise: the image centre)."""
    g = CASES[name][7].get("gaze")
    return None if g is None else np.asarray(g, dtype=np.float32)


def load_golden(name):
    """(jod [B], gradient of the test or None, gradient of the reference or None) the reference computed for one case."""
    z = np.load(os.path.join(GOLDEN, FILES[name]))
    g = {k: z[name + "_grad_" + k].astype(np.float32) if name + "_grad_" + k in z.files else None for k in ("test", "reference")}
    return z[name + "_jod"].astype(np.float32), g["test"], g["reference"]
