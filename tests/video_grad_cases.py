"""Inputs of the video gradient goldens (tests/golden/g19_video_grad_*.npz), rebuilt from their description: the goldens store
only the reference's outputs.  Shared by tools/gen_golden_video_grad.py (which writes them) and the tests (which read them)."""
import os

import numpy as np

from fovvideovdp_amd.synth import synth_gaze, synth_video_pair

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name: (C, N, H, W, frames per second, temporal padding, display_name, options)
CASES = {
    "a_gray_30_replicate": (1, 12, 68, 121, 30, "replicate", "standard_fhd", {}),    # odd sizes: both parities of the reduce quirk
    "b_rgb_60_circular": (3, 10, 68, 121, 60, "circular", "standard_4k", {}),         # fl = 15 > N: the head wraps round the clip
    "c_gray_30_circular": (1, 12, 68, 121, 30, "circular", "standard_fhd", {}),       # fl = 8 < N: no window shows frame 0
    "d_rgb_30_pingpong_fov": (3, 9, 68, 121, 30, "pingpong", "standard_4k", {"foveated": True, "gaze": True}),
    "e_rgb_pq_oob": (3, 6, 68, 121, 30, "replicate", "standard_hdr_pq", {"oob": True}),   # some test samples outside [0, 1]
    "f_gray_linear": (1, 8, 68, 121, 24, "pingpong", "standard_hdr_linear", {"scale": 400.0}),      # cd/m^2
    "g_rgb_gamma22": (3, 5, 68, 121, 30, "replicate", "standard_4k",
                      {"photometry": dict(Y_peak=300.0, contrast=800.0, EOTF="gamma", gamma=2.2)}),
    "h_rgb_2f_120": (3, 2, 68, 121, 120, "replicate", "standard_4k", {}),            # fl = 30: nearly everything folds into frame 0
    "i_identical": (1, 4, 68, 121, 30, "replicate", "standard_4k", {"identical": (0, 4)}),
    "j_partly_identical": (3, 6, 68, 121, 30, "replicate", "standard_4k", {"identical": (0, 3)}),   # output frames 0..2 see no difference
    # The variants of the temporal transpose (video_input_kernel<FL, PX>: ring slots, pixels per lane) the cases above do not
    # select: an odd H*W takes the per-pixel variant, H*W % 4 == 2 the 2-pixel variant above 16 taps.  New names sort after
    # the ones above, so every case keeps its seed.
    "k_gray_30_odd": (1, 5, 67, 121, 30, "replicate", "standard_fhd", {}),            # fl = 8:  FL 8, PX 1
    "l_gray_60_circular_odd": (1, 6, 67, 121, 60, "circular", "standard_4k", {}),     # fl = 15: FL 16, PX 1
    "m_gray_120_pingpong_mod2": (1, 5, 69, 122, 120, "pingpong", "standard_4k", {}),  # fl = 30: FL 32, PX 2, H*W % 4 == 2
    "n_gray_120_odd": (1, 4, 67, 121, 120, "replicate", "standard_fhd", {}),          # fl = 30: FL 32, PX 1
    "o_gray_240_replicate": (1, 5, 68, 121, 240, "replicate", "standard_4k", {}),     # fl = 60: FL 64, PX 2
    "p_gray_144_circular_odd": (1, 6, 67, 121, 144, "circular", "standard_4k", {}),   # fl = 36: FL 64, PX 1
    "q_rgb_256": (3, 4, 68, 121, 256, "replicate", "standard_4k", {}),                # fl = 64: every slot of the longest ring
    # more than 256 frames: the second stride of video_coef_kernel's clip sum, and many backward batches; the golden holds
    # the gradient of the listed frames only
    "r_gray_long": (1, 300, 18, 32, 30, "replicate", "standard_fhd", {"frames": (0, 255, 256, 299)}),
}
# the file each case's outputs live in (each committed file stays below 1 MiB)
FILES = {"a_gray_30_replicate": "g19_video_grad_1.npz", "c_gray_30_circular": "g19_video_grad_1.npz",
         "f_gray_linear": "g19_video_grad_1.npz", "b_rgb_60_circular": "g19_video_grad_2.npz",
         "h_rgb_2f_120": "g19_video_grad_2.npz", "d_rgb_30_pingpong_fov": "g19_video_grad_3.npz",
         "i_identical": "g19_video_grad_3.npz", "e_rgb_pq_oob": "g19_video_grad_4.npz", "g_rgb_gamma22": "g19_video_grad_4.npz",
         "j_partly_identical": "g19_video_grad_5.npz",
         "k_gray_30_odd": "g19_video_grad_6.npz", "l_gray_60_circular_odd": "g19_video_grad_6.npz",
         "m_gray_120_pingpong_mod2": "g19_video_grad_6.npz", "n_gray_120_odd": "g19_video_grad_6.npz",
         "o_gray_240_replicate": "g19_video_grad_7.npz", "p_gray_144_circular_odd": "g19_video_grad_7.npz",
         "q_rgb_256": "g19_video_grad_8.npz", "r_gray_long": "g19_video_grad_8.npz"}


def case_inputs(name):
    """(test, reference) float32 [C, N, H, W] numpy arrays of one case."""
    C, N, H, W, _, _, _, opt = CASES[name]
    seed = 300 + sorted(CASES).index(name)
    t8, r8 = synth_video_pair(N, H, W, C=C, seed_ref=seed, seed_test=seed + 50)
    t = t8[0].numpy().astype(np.float32) / np.float32(255.0)
    r = r8[0].numpy().astype(np.float32) / np.float32(255.0)
    if "identical" in opt:
        f0, f1 = opt["identical"]
        t[:, f0:f1] = r[:, f0:f1]
    if opt.get("oob"):
        t[:, 1:4, 10:14, 20:60] = np.float32(1.15)
        t[C - 2, 2:5, 50:54, 70:110] = np.float32(-0.1)
    if "scale" in opt:
        t, r = t * np.float32(opt["scale"]), r * np.float32(opt["scale"])
    return np.ascontiguousarray(t), np.ascontiguousarray(r)


def case_gaze(name):
    """Per-frame gaze [N, 2] of a foveated case with a moving gaze (None otherwise: the frame centre)."""
    C, N, H, W, _, _, _, opt = CASES[name]
    return synth_gaze(N, H, W).numpy() if opt.get("gaze") else None


def golden_frames(name):
    """The frames whose gradient the golden of a case holds (None: all of them)."""
    frames = CASES[name][7].get("frames")
    return None if frames is None else list(frames)


def load_golden(name):
    """(jod, grad [C, N, H, W]) the reference computed for one case (of a case with `frames`: [C, len(frames), H, W])."""
    z = np.load(os.path.join(GOLDEN, FILES[name]))
    return float(z[name + "_jod"]), z[name + "_grad"].astype(np.float32)
