"""Frame maps, shapes and inputs of the held-frame tests (tests/test_held_cpu.py, tests/test_gpu_held_input.py,
tests/test_gpu_held.py) and of the golden tests/golden/g26_held_grad.npz, rebuilt from fixed seeds: the golden stores only the
reference's outputs.  Shared by tools/gen_golden_held_grad.py (which writes it) and the tests (which read it)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_FILE = "g26_held_grad.npz"
FL = {30: 8, 60: 15, 120: 30}                       # taps of the temporal filters at each display rate (rings of 8 / 16 / 32 slots)
PADDINGS = ("replicate", "circular", "pingpong")


# ---- frame maps -----------------------------------------------------------------------------------------------------------------
def pulldown(N):
    """3:2 pulldown: source frames shown for 3, 2, 3, 2, ... display frames."""
    m = np.repeat(np.arange(N), np.resize([3, 2], N))[:N]
    return m.astype(np.int32)


def skipping(N):
    """Every third source frame is never shown: 0, 1, 3, 4, 6, 7, ..."""
    v = np.arange(N)
    return (v + v // 2).astype(np.int32)


MAP_KINDS = ("hold2", "hold3", "hold4", "pulldown", "skip", "above0", "constant")


def c_abi_map(kind, N):
    """(map [N], n_source) of the C-ABI test: N is whatever the case asks for, so a hold's last frame is cut short whenever N is
    not a multiple of k."""
    v = np.arange(N)
    if kind.startswith("hold"):
        m = v // int(kind[4:])
        return m.astype(np.int32), int(m[-1]) + 1
    if kind == "pulldown":
        m = pulldown(N)
        return m, int(m[-1]) + 1
    if kind == "skip":
        m = skipping(N)
        return m, int(m[-1]) + 2                    # ... and the clip's last frame is not shown either
    if kind == "above0":
        m = 2 + v // 2
        return m.astype(np.int32), int(m[-1]) + 1   # frames 0 and 1 are never shown
    if kind == "constant":
        return np.full(N, 1, np.int32), 3           # one frame held for the whole clip, between two that are never shown
    if kind == "identity":
        return v.astype(np.int32), N
    raise ValueError(kind)


# ---- end-to-end cases -------------------------------------------------------------------------------------------------------------
# name: (W, H), C, display rate, padding, sample type, test_frames, reference_frames, N, options.  A spec is an int k or the name of
# a map function above.  N >= 2 fl + 3 for circular and pingpong: the head then shows at most half of either stream's frames
# (test_held_cpu.test_head_shown_frames_stay_within_the_cap), which the derived bound of the gradient test does not cover.
CASES = {
    "k2":      ((121, 68), 3, 30, "replicate", "float32", 2, 1, 12, {}),
    "k3":      ((122, 69), 1, 60, "circular", "float16", 3, 1, 36, {}),
    "k4":      ((121, 68), 3, 120, "pingpong", "bfloat16", 4, 1, 64, {}),
    "kr2":     ((122, 69), 3, 30, "circular", "uint8", 1, 2, 20, {"host": True}),
    "seq":     ((121, 67), 1, 60, "replicate", "uint16", "pulldown", "skipping", 30, {"host": True}),
    "fov":     ((121, 68), 3, 30, "pingpong", "float32", 2, 1, 20, {"foveated": True, "batch_frames": 7}),
    "mixed":   ((121, 68), 3, 30, "replicate", ("float16", "uint8"), 2, 1, 12, {}),
    "fchw":    ((122, 69), 3, 60, "replicate", "float32", 4, 2, 32, {"dim_order": "FCHW"}),
    "odd":     ((121, 67), 3, 30, "replicate", "float32", 3, 1, 12, {}),
    "pq":      ((121, 68), 3, 30, "pingpong", "float32", "pulldown", 1, 20, {"display": "standard_hdr_pq"}),
    "skipref": ((121, 68), 1, 30, "replicate", "float32", "pulldown", "skipping", 20, {}),
}
GRAD_CASES = ("k2", "k3", "k4", "fov", "fchw", "odd", "pq")      # float samples: what jod_video_held takes
# the golden: k = 4, sRGB, 60 fps, replicate; pulldown, PQ, 30 fps, pingpong; k = 2, foveated with a moving gaze
GOLDEN_CASES = {
    "g_k4":       ((121, 68), 3, 60, "replicate", "float32", 4, 1, 8, {}),
    "g_pulldown": ((121, 68), 1, 30, "pingpong", "float32", "pulldown", 1, 20, {"display": "standard_hdr_pq"}),
    "g_fov":      ((122, 69), 1, 30, "replicate", "float32", 2, 1, 8, {"foveated": True}),
}
ALL_CASES = dict(CASES, **GOLDEN_CASES)


def spec_map(spec, N):
    """(frame map [N], source frames of the stream) of a case's spec."""
    if isinstance(spec, int):
        assert N % spec == 0
        return (np.arange(N) // spec).astype(np.int32), N // spec
    m = {"pulldown": pulldown, "skipping": skipping}[spec](N)
    return m, int(m[-1]) + 1


def spec_arg(spec, N):
    """What the case passes as test_frames= / reference_frames=: the int, or the sequence."""
    return spec if isinstance(spec, int) else spec_map(spec, N)[0]


def case_maps(name):
    c = ALL_CASES[name]
    (m_t, F_t), (m_r, F_r) = spec_map(c[5], c[7]), spec_map(c[6], c[7])
    return m_t, F_t, m_r, F_r


_INPUTS = {}


def case_inputs(name):
    """(test [C, F_t, H, W], reference [C, F_r, H, W]) as numpy arrays (float32 for every float type), drawn once per process.
    The reference is a random clip at its own rate; the test is the reference at the frames it shows plus noise, so the JOD
    lies well inside (0, 10)."""
    if name not in _INPUTS:
        (W, H), C, fps, padding, dtype, ts, rs, N, opt = ALL_CASES[name]
        dt_t, dt_r = dtype if isinstance(dtype, tuple) else (dtype, dtype)
        m_t, F_t, m_r, F_r = case_maps(name)
        rng = np.random.default_rng([26, sorted(ALL_CASES).index(name)])
        ref = rng.uniform(0.1, 0.9, (C, F_r, H, W))
        # the reference frame on screen when each test frame first appears
        first = np.asarray([int(m_r[int(np.argmax(m_t >= j))]) if (m_t >= j).any() else F_r - 1 for j in range(F_t)])
        test = np.clip(ref[:, first] + rng.normal(0.0, 0.08, (C, F_t, H, W)), 0.02, 0.98)

        def cast(x, dt):
            if dt == "uint8":
                return np.round(x * 255).astype(np.uint8)
            if dt == "uint16":
                return np.round(x * 65535).astype(np.uint16)
            return x.astype(np.float32)
        _INPUTS[name] = (cast(test, dt_t), cast(ref, dt_r))
    return _INPUTS[name]


def case_gaze(name):
    """[N, 2] gaze positions in pixels for a foveated case: a diagonal sweep; None otherwise."""
    (W, H), _, _, _, _, _, _, N, opt = ALL_CASES[name]
    if not opt.get("foveated"):
        return None
    s = np.linspace(0.2, 0.8, N)
    return np.stack([s * W, (1 - s) * H], axis=1).astype(np.float32)


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, GOLDEN_FILE))
    return float(z[name + "_jod"]), z[name + "_grad"]
