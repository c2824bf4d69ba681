"""Inputs of the reference-gradient goldens (tests/golden/g21_image_ref_grad.npz, g22_video_ref_grad_*.npz), rebuilt from
their description: the goldens store only the reference implementation's outputs (<case>_jod, <case>_gref = dJOD/dreference).
Shared by tools/gen_golden_ref_grad.py (which writes them) and the tests (which read them).  The cases that exist for the test
gradient (g18 / g19) come from grad_cases.py and video_grad_cases.py unchanged, so a case of the same name has the same test
input; two of them get a different reference here, and one new case per kind drives the clamps of the reference's own paths."""
import os

import numpy as np

import grad_cases as ic
import video_grad_cases as vc

GOLDEN = ic.GOLDEN

# ---- still images: name -> (C, H, W, display_name, options) -----------------------------------------------------------------
IMAGE_CASES = {k: ic.CASES[k] for k in ("a_gray_fhd", "b_rgb_4k_oob", "c_rgb_hdr_pq", "f_rgb_foveated", "g_identical")}
# dark region at the display's black level + peak specks (cd/m^2): the L_bkg clamp and the contrast clamp bind
IMAGE_CASES["i_hdr_linear_dark"] = (1, 90, 160, "standard_hdr_linear", {"scale": 400.0, "dark": True})
IMAGE_FILE = "g21_image_ref_grad.npz"

# ---- clips: name -> (C, N, H, W, frames per second, temporal padding, display_name, options) -------------------------------
# (c_gray_30_circular is the clip in which no temporal window shows frame 0: fl = 8 < N; in b_rgb_60_circular the head wraps)
VIDEO_CASES = {k: vc.CASES[k] for k in ("a_gray_30_replicate", "b_rgb_60_circular", "c_gray_30_circular", "d_rgb_30_pingpong_fov",
                                        "e_rgb_pq_oob", "h_rgb_2f_120", "j_partly_identical", "k_gray_30_odd")}
VIDEO_CASES["s_hdr_linear_dark"] = (1, 4, 68, 121, 30, "replicate", "standard_hdr_linear", {"scale": 400.0, "dark": True})
VIDEO_FILES = {"a_gray_30_replicate": "g22_video_ref_grad_1.npz", "k_gray_30_odd": "g22_video_ref_grad_1.npz",
               "s_hdr_linear_dark": "g22_video_ref_grad_1.npz", "b_rgb_60_circular": "g22_video_ref_grad_2.npz",
               "h_rgb_2f_120": "g22_video_ref_grad_2.npz", "d_rgb_30_pingpong_fov": "g22_video_ref_grad_3.npz",
               "e_rgb_pq_oob": "g22_video_ref_grad_4.npz", "j_partly_identical": "g22_video_ref_grad_5.npz",
               "c_gray_30_circular": "g22_video_ref_grad_5.npz"}
# cases whose (test, reference) are exactly those of g18 / g19: the generator asserts that its test gradient is the stored one
SHARED_IMAGE = ("a_gray_fhd", "c_rgb_hdr_pq", "f_rgb_foveated", "g_identical")
SHARED_VIDEO = ("a_gray_30_replicate", "b_rgb_60_circular", "c_gray_30_circular", "d_rgb_30_pingpong_fov", "h_rgb_2f_120", "j_partly_identical",
                "k_gray_30_odd")

DARK, PEAK = np.float32(0.01), np.float32(1500.0)     # cd/m^2 behind standard_hdr_linear: 0.01 + black level 0.017 < 0.1


def _dark_frame(t, r, f):
    """In place, one [C, H, W] frame pair in cd/m^2: a region at the display's black level in both images, so that the
    expanded coarser level stays below 0.1 (the L_bkg clamp binds, the LUT's low-luminance end is approached), and isolated
    peak-luminance specks inside it.  Specks only the test has sit on a dark reference: t = layer^T / 0.1 passes the contrast
    clamp of 1000.  r = layer^R / L_bkg with L_bkg from the same plane cannot (the expanded level keeps at least 1/16 of a
    speck: r <= 15); the reference's specks move with the frame number f, so in a clip a new speck is in the TRANSIENT plane
    (tap 0 = 0.48) while the sustained plane, which L_bkg comes from, does not see it yet (tap 0 = 1e-36): r passes 1000 there."""
    H, W = t.shape[-2:]
    y0, y1, x0, x1 = H // 5, H - H // 5, W // 5, W - W // 5
    t[:, y0:y1, x0:x1] = DARK
    r[:, y0:y1, x0:x1] = DARK
    for i in range(6):
        y = y0 + 6 + (7 * i + 5 * f) % (y1 - y0 - 12)
        x = x0 + 6 + (17 * i + 11 * f) % (x1 - x0 - 12)
        r[:, y, x] = PEAK                              # reference only, moving
        t[:, y, (x + 9 - x0) % (x1 - x0 - 12) + x0 + 6] = PEAK      # test only
    t[:, y0 + 3, x0 + 3] = PEAK                        # in both, fixed
    r[:, y0 + 3, x0 + 3] = PEAK


def image_inputs(name):
    """(test, reference) float32 [C, H, W] numpy arrays of one image case."""
    C, H, W, _, opt = IMAGE_CASES[name]
    if name == "i_hdr_linear_dark":
        t, r = ic.case_inputs("d_gray_hdr_linear")      # the same synthetic pair and scale, then the dark region
        t, r = t.copy(), r.copy()
        _dark_frame(t, r, 0)
        return np.ascontiguousarray(t), np.ascontiguousarray(r)
    t, r = ic.case_inputs(name)
    if opt.get("oob"):                                  # an out-of-range patch in the REFERENCE too
        r = r.copy()
        r[:, 40:44, 100:140] = np.float32(1.2)
        r[0, 70:74, 30:60] = np.float32(-0.05)
    return t, r


def video_inputs(name):
    """(test, reference) float32 [C, N, H, W] numpy arrays of one clip case."""
    C, N, H, W, _, _, _, opt = VIDEO_CASES[name]
    if name == "s_hdr_linear_dark":
        from fovvideovdp_amd.synth import synth_video_pair
        t8, r8 = synth_video_pair(N, H, W, C=C, seed_ref=390, seed_test=440)
        t = t8[0].numpy().astype(np.float32) / np.float32(255.0) * np.float32(opt["scale"])
        r = r8[0].numpy().astype(np.float32) / np.float32(255.0) * np.float32(opt["scale"])
        for f in range(N):
            _dark_frame(t[:, f], r[:, f], f)
        return np.ascontiguousarray(t), np.ascontiguousarray(r)
    t, r = vc.case_inputs(name)
    if opt.get("oob"):
        r = r.copy()
        r[:, 2:5, 30:34, 40:80] = np.float32(1.2)
        r[0, 0:3, 55:59, 10:50] = np.float32(-0.05)
    return t, r


def video_gaze(name):
    return vc.case_gaze(name) if name in vc.CASES else None


def load_image_golden(name):
    """(jod, dJOD/dreference [C, H, W]) of the reference implementation."""
    z = np.load(os.path.join(GOLDEN, IMAGE_FILE))
    return float(z[name + "_jod"]), z[name + "_gref"].astype(np.float32)


def load_video_golden(name):
    """(jod, dJOD/dreference [C, N, H, W]) of the reference implementation."""
    z = np.load(os.path.join(GOLDEN, VIDEO_FILES[name]))
    return float(z[name + "_jod"]), z[name + "_gref"].astype(np.float32)


def clamp_counts(name):
    """Band pixels of a clamp-coverage case that each clamp catches, from the maps of the float32 CPU oracle:
    {"lbkg": L_bkg == 0.1, "t": test contrast == 1000, "r": reference contrast == 1000}."""
    from oracle import fvvdp_oracle as orc
    o = orc.Oracle("standard_hdr_linear")
    o.capture = {}
    if name in IMAGE_CASES:
        t, r = image_inputs(name)
        o.predict(t[:, None], r[:, None], dim_order="CFHW")
    else:
        t, r = video_inputs(name)
        o.predict(t, r, dim_order="CFHW", frames_per_second=VIDEO_CASES[name][4])
    out = {"lbkg": 0, "t": 0, "r": 0}
    for bands, lbkg in zip(o.capture["bands"], o.capture["L_bkg"]):
        for b, L in enumerate(lbkg):
            out["lbkg"] += int((L == np.float32(0.1)).sum())
            for p in range(bands[b].shape[0]):
                out["t" if p % 2 == 0 else "r"] += int((bands[b][p] >= np.float32(1000.0)).sum())
    return out
