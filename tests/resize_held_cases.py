"""Cases of the resized-and-held tests (tests/test_resize_held_cpu.py, tests/test_gpu_resize_held.py): the rotation of
resize_cases.py (four modes x three rings; sources x2, x1.5, x3 with an odd height, x0.5, ...; targets 120x68 and 122x68; C = 1 / 3;
a uint8 reference; the three paddings) paired with the frame maps of held_cases.py.  Inputs are resize_cases' own, drawn at each
stream's frame count, computed once and left unchanged."""
import numpy as np

import held_cases as hc
import resize_cases as rc

# name: (the test's map kind, the reference's) of held_cases.c_abi_map -- k = 2, k = 4, 3:2 pulldown, skipping (frames that are
# never shown, the clip's last among them), the identity on one stream, two different maps with differing source frame counts
MAPS = {"k2": ("hold2", "identity"), "k4": ("hold4", "identity"), "pulldown": ("pulldown", "identity"),
        "skipping": ("skip", "identity"), "ref_k2": ("identity", "hold2"), "both": ("pulldown", "skip")}


def case_maps(name, N):
    """(m_t, F_t, m_r, F_r) for N display frames; a hold's last frame is cut short where N is no multiple of k."""
    kt, kr = MAPS[name]
    (m_t, F_t), (m_r, F_r) = hc.c_abi_map(kt, N), hc.c_abi_map(kr, N)
    return m_t, F_t, m_r, F_r


def rotation():
    """resize_cases.rotation() with a `maps` name per case: every name appears, and every ring meets a held test and a held
    reference (test_resize_held_cpu.test_rotation_covers_the_matrix)."""
    names = list(MAPS)
    return [dict(c, maps=names[(k + k // 3) % len(names)]) for k, c in enumerate(rc.rotation())]


def case_id(c):
    return rc.case_id(c) + "-" + c["maps"]


def inputs(c, N=None):
    """(test float32 [C, F_t, h, w], reference [C, F_r, hr, wr], m_t, m_r) of one case for N display frames (default: ring + 3, so
    every ring wraps once and a reuse crosses the chunk boundary at u = 0)."""
    N = rc.RING[c["fps"]] + 3 if N is None else N
    m_t, F_t, m_r, F_r = case_maps(c["maps"], N)
    test = rc.rotation_inputs(c, F_t)[0]
    ref = rc.rotation_inputs(c, F_r)[1]
    return test, ref, m_t, m_r


def gl_for(c, N):
    """A luminance gradient [N, Ho, Wo] of mixed signs and magnitudes in [0.25, 2], as test_gpu_resize.py draws it."""
    Wo, Ho = c["target"]
    rng = np.random.default_rng([N, Wo, Ho, c["source"][0]])
    return (rng.uniform(0.25, 2.0, (N, Ho, Wo)) * rng.choice([-1.0, 1.0], (N, Ho, Wo))).astype(np.float32)
