"""Shapes and inputs of the mixed-resolution tests (tests/test_resize_cpu.py, tests/test_gpu_resize.py) and of the goldens
tests/golden/g25_resize_grad_*.npz, rebuilt from fixed seeds: the goldens store only the reference's outputs.  Shared by
tools/gen_golden_resize_grad.py (which writes them) and the tests (which read them).

A clip is drawn with samples on both sides of [0, 1] (float32: uniform in [-0.25, 1.25]; uint8: every code).  Then every source
sample that reaches a target sample whose float64 pre-clip value lies in the zone where float32 and float64 could clip differently
(resize_ref.margin: within 1e-4 of 0 or 1 without being beyond by more than 1e-2) is drawn again from the middle of the range,
until no such target sample is left.  Values interpolated between middle samples stay in the middle, so this ends; at small
factors most of the out-of-range samples survive it, at factor 17 (where almost every transition across 0 or 1 lands a target
sample in the zone) few do -- that source exercises the long candidate ranges and the border clamps instead."""
import os

import numpy as np

import resize_ref as rref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TARGETS = [(120, 68), (122, 68)]                                      # (width, height); 122: W % 4 != 0
# (width, height): x2; x1.5 (not an integer, another factor per axis); x3 with an odd height; near-identity, both parities; x0.5
# (a downscale skips samples: they must come back as written zeros); factor 17 (long candidate ranges, every tap clamped at a border)
SOURCES = [(60, 34), (80, 46), (40, 23), (121, 67), (240, 136), (7, 5)]
DISPLAYS = ("standard_fhd", "standard_hdr_pq", "gamma2.4")
PADDINGS = ("replicate", "circular", "pingpong")
FPS = (30, 60, 120)                                                   # rings of 8, 16 and 32 slots


def rotation():
    """The twelve mode x ring cases; source, target, channel count, the reference's sample type and size, display and padding rotate
    through them.  Entries: dict(mode, fps, source, target, C, ref_dtype, ref_source (None: the reference has the target's size),
    display, padding)."""
    out = []
    for mi, mode in enumerate(rref.MODES):
        for fi, fps in enumerate(FPS):
            k = 3 * mi + fi
            # (nearest gets the x0.5 source: the one mode whose downscale skips samples)
            out.append(dict(mode=mode, fps=fps, source=SOURCES[(2 * k + mi) % 6], target=TARGETS[(mi + fi) % 2], C=(3, 1)[(k + mi // 2) % 2],
                            ref_dtype=("float32", "uint8")[(k // 2) % 2], ref_source=None if k % 3 == 1 else SOURCES[(2 * k + mi + 2) % 6],
                            display=DISPLAYS[(mi + fi) % 3], padding=PADDINGS[k % 3]))
    return out


# Long axes: (n_in, n_out) of one axis whose products of an index and a size go beyond 2^24, where the floor and ceil of a float32
# quotient leave ATen's integer `area` windows -- 5805 -> 2903: the last float32 window would end one sample past the plane; 4100 ->
# 4099 and 7680 -> 4097: one window bound each.  The other axis is LONG_SHORT, so a frame stays at a few hundred kilobytes.
LONG_AXES = [(5805, 2903), (4100, 4099), (7680, 4097)]
LONG_SHORT = (6, 8)


def long_cases():
    """Cases of the form of rotation() at the long axes, each as the height and as the width: `area` on every pair, the other three
    modes on two pairs each; the 30 fps ring.  Two cases resize both streams (a uint8 reference of the test's size).  The display
    is sRGB throughout, the one model of DISPLAYS whose derivative is well conditioned over all of [0, 1]; the adjoint's bound is
    4 x the error of ONE float32 evaluation, and with some 300 000 target values per case the other two models make that error a
    matter of which value the evaluation order happens to hit:
      PQ     the derivative jumps to 0 at the display's peak; a frame has a value whose float32 and float64 forms lie on either
             side of it, and the float32 restatement is then off by 7.6 times the sum of a sample's absolute terms;
      gamma  the derivative V^1.4 has the relative condition number 1.4 / V, in-range values come as close to 0 as the margin
             lets them (1e-4), and an `area` mean of samples around 0.5 carries a rounding error of about 3e-8: the term moves by
             up to 4e-4 of itself.  On the CPU the float32 derivatives of one frame's targets (7680 -> 4097) are off by 8.8e-6 with
             the windows summed in one order and by 3.0e-5 in the other; on the GPU the adjoint was off by 2.5e-5 where the
             restatement was by 4.4e-6.
    The rotation keeps both models, at sizes that meet neither."""
    plan = [("area", 0, "h"), ("area", 0, "w"), ("area", 1, "h"), ("area", 1, "w"), ("area", 2, "h"), ("area", 2, "w"),
            ("nearest", 0, "h"), ("nearest", 2, "w"), ("bilinear", 1, "w"), ("bilinear", 0, "h"), ("bicubic", 2, "h"), ("bicubic", 1, "w")]
    out = []
    for k, (mode, pair, along) in enumerate(plan):
        n_in, n_out = LONG_AXES[pair]
        source = (LONG_SHORT[0], n_in) if along == "h" else (n_in, LONG_SHORT[0])
        target = (LONG_SHORT[1], n_out) if along == "h" else (n_out, LONG_SHORT[1])
        out.append(dict(mode=mode, fps=30, source=source, target=target, C=(3, 1)[k % 2], ref_dtype=("uint8", "float32")[(k // 2) % 2],
                        ref_source=source if k in (1, 6) else None, display="standard_fhd", padding=PADDINGS[(k + 1) % 3]))
    return out


def case_id(c):
    return "%s-%dfps-%dx%d-to-%dx%d-C%d-%s-%s-ref-%s%s" % (c["mode"], c["fps"], *c["source"], *c["target"], c["C"], c["display"], c["padding"],
                                                           c["ref_dtype"], "" if c["ref_source"] is None else "-%dx%d" % c["ref_source"])


def draw_clip(seed, C, N, source, target, mode, dtype="float32"):
    """(clip [C, N, h, w], samples drawn again) with the margin of the module text; source and target are (width, height)."""
    rng = np.random.default_rng(list(seed) + [25])
    w, h = source
    if dtype == "uint8":
        x = rng.integers(0, 256, (C, N, h, w)).astype(np.uint8)
    else:
        x = rng.uniform(-0.25, 1.25, (C, N, h, w)).astype(np.float32)
    if tuple(source) == tuple(target):
        return x, 0
    redrawn = 0
    frames = x.reshape(C * N, h, w)                      # (a view: the frames that still have such a sample are worked on alone)
    active = np.arange(C * N)
    for _ in range(h * w + 1):
        bad = rref.margin(frames[active], target, mode)
        keep = bad.any(axis=(1, 2))
        active, bad = active[keep], bad[keep]
        if not len(active):
            return x, redrawn
        hit = rref.reaches(bad, source, mode)
        n = int(hit.sum())
        redrawn += n
        sub = frames[active]
        sub[hit] = rng.integers(77, 180, n).astype(np.uint8) if dtype == "uint8" else rng.uniform(0.3, 0.7, n).astype(np.float32)
        frames[active] = sub
    raise AssertionError("no clip with the margin found")


RING = {30: 8, 60: 16, 120: 32}                                       # slots of the register ring at each frame rate
_ROTATION = {}


def rotation_inputs(c, N=None):
    """(test float32 [C, N, h, w], reference [C, N, hr, wr] of the case's sample type, at its own size or at the target's) of one
    rotation case, N = ring + 3 frames unless given; computed once and left unchanged."""
    N = RING[c["fps"]] + 3 if N is None else N
    key = (case_id(c), N)
    if key not in _ROTATION:
        seed = [N, c["fps"], rref.MODES.index(c["mode"]), *c["source"], *c["target"]]
        test, _ = draw_clip(seed, c["C"], N, c["source"], c["target"], c["mode"])
        ref, _ = draw_clip(seed + [1], c["C"], N, c["ref_source"] or c["target"], c["target"], c["mode"], c["ref_dtype"])
        test.setflags(write=False)
        ref.setflags(write=False)
        _ROTATION[key] = (test, ref)
    return _ROTATION[key]


# ---- the goldens ------------------------------------------------------------------------------------------------------------------
# name: (N, C, source, target, mode, display_name, frames per second, temporal padding, options)
CASES = {
    "a_bilinear_x2_srgb_30": (10, 3, (60, 34), (120, 68), "bilinear", "standard_fhd", 30, "replicate", {}),
    "b_bicubic_x1p5_pq_60_circular": (10, 3, (80, 46), (120, 68), "bicubic", "standard_hdr_pq", 60, "circular", {}),
    "c_area_down_gamma_pingpong": (6, 3, (240, 136), (120, 68), "area", "standard_4k", 24, "pingpong",
                                   {"photometry": dict(Y_peak=300.0, contrast=800.0, EOTF="gamma", gamma=2.2)}),
    "d_nearest_x3_gray": (8, 1, (40, 23), (120, 68), "nearest", "standard_4k", 30, "replicate", {}),
    "e_bilinear_fov": (9, 3, (60, 34), (120, 68), "bilinear", "standard_4k", 30, "pingpong", {"foveated": True, "gaze": True}),
}
FILES = {name: "g25_resize_grad_%d.npz" % (i + 1) for i, name in enumerate(CASES)}
# (seeds are kept clear of a band pixel on the d_max clamp: see the finding recorded in yuv_grad_cases.py)
SEEDS = {"a_bilinear_x2_srgb_30": 2500, "b_bicubic_x1p5_pq_60_circular": 2501, "c_area_down_gamma_pingpong": 2502,
         "d_nearest_x3_gray": 2503, "e_bilinear_fov": 2504}
_INPUTS = {}


def case_inputs(name):
    """(test float32 [C, N, h, w], reference float32 [C, N, Ho, Wo] at the target size) of one golden case; computed once and left
    unchanged.  The reference is the test resized and clipped plus noise, so the JOD is neither 10 nor at the floor."""
    if name not in _INPUTS:
        N, C, source, target, mode = CASES[name][:5]
        test, _ = draw_clip([SEEDS[name]], C, N, source, target, mode)
        rng = np.random.default_rng([SEEDS[name], 26])
        ref = np.clip(rref.resize(test.astype(np.float64), target, mode), 0, 1)
        ref = np.clip(ref + rng.normal(0, 0.05, ref.shape), 0, 1).astype(np.float32)
        test.setflags(write=False)
        ref.setflags(write=False)
        _INPUTS[name] = (test, ref)
    return _INPUTS[name]


def case_gaze(name):
    """Per-frame gaze [N, 2] in target pixels of a foveated case with a moving gaze (None otherwise: the frame centre)."""
    from fovvideovdp_amd.synth import synth_gaze
    N, _, _, target = CASES[name][:4]
    return synth_gaze(N, target[1], target[0]).numpy() if CASES[name][8].get("gaze") else None


def load_golden(name):
    """(jod, gradient [C, N, h, w]) the reference computed for one case."""
    z = np.load(os.path.join(GOLDEN, FILES[name]))
    return float(z[name + "_jod"]), z[name + "_grad"].astype(np.float32)
