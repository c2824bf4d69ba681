"""What every differentiable entry point asks of the native library, call by call: the symbols in order, with one token per
positional argument -- a plain Python int as itself, None as "null", everything else (pointers, byref, arrays) as "ptr".  The
numeric tests pin the results bit for bit; this one pins what they cannot see: an added launch, ingest, workspace query or
context call, a changed batch offset or size, a slope-map bracket that is not closed.

Per case: a fresh metric (batch_frames = 2, grad_batch = 2: every loop runs a full and a partial batch, whatever memory is
free), one warm-up forward + backward (context creation and table uploads), then the second forward + backward is recorded
through a proxy in the place of fovvideovdp_amd._native.lib and compared with tests/golden/grad_call_sequences.json.

The fixture is a record of the library calls, not a property to tune: it is written by this same file, with

    FVVDP_RECORD_CALL_SEQUENCES=tests/golden/grad_call_sequences.json python -m pytest -m gpu tests/test_gpu_grad_call_sequence.py

(the variable names the file to write) run on the commit whose behaviour is to be kept -- the parent of a change to the launch
code -- and only compared otherwise.  Recording asserts what comparing asserts about the slope-map brackets and the context's
parameter calls, so a record that lacks them is never written."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
RECORD = os.environ.get("FVVDP_RECORD_CALL_SEQUENCES")
W, H, C_CH, B, N, FPS, G = 121, 67, 3, 3, 5, 30, 3
GAZE = [40.0, 30.0]


@pytest.fixture(scope="module")
def fv():
    import fovvideovdp_amd
    from fovvideovdp_amd import _native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _native.lib()
    return fovvideovdp_amd


@pytest.fixture(scope="module")
def fixture_file(golden_dir):
    """The recorded sequences by case name; in recording mode the dict the cases fill, written when the module is done."""
    if not RECORD:
        with open(os.path.join(golden_dir, "grad_call_sequences.json")) as f:
            yield json.load(f)
        return
    have = {}
    yield have
    with open(RECORD, "w") as f:
        f.write("{\n" + ",\n".join('%s: [\n%s\n]' % (json.dumps(k), ",\n".join(json.dumps(c) for c in have[k]))
                                   for k in sorted(have)) + "\n}\n")


def _token(a):
    if type(a) is int:
        return a
    return "null" if a is None else "ptr"


class _Recorder:
    """Stands in for the ctypes library: every foreign function looked up on it is called through, after its name and argument
    tokens have been appended to `calls`."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self.calls.append([name] + [_token(a) for a in args])
            return fn(*args)
        return call


def _pair(shape, requires=()):
    g = torch.Generator(device=DEV).manual_seed(20240611)
    r = torch.rand(shape, generator=g, device=DEV, dtype=torch.float32)
    t = (r + 0.05 * (torch.rand(shape, generator=g, device=DEV, dtype=torch.float32) - 0.5)).clamp(0, 1)
    return t.requires_grad_("test" in requires), r.requires_grad_("reference" in requires)


def _stills(wrt_needs=()):
    return _pair((B, C_CH, H, W), wrt_needs)


def _clip(wrt_needs=()):
    return _pair((1, C_CH, N, H, W), wrt_needs)


NEEDS = {"test": ("test",), "both": ("test", "reference")}


def _jod_images(wrt):
    def run(m):
        t, r = _stills(NEEDS[wrt])
        return m.jod_images(t, r, wrt=wrt)
    return {}, run


def _jod_video(wrt, foveated=False):
    def run(m):
        t, r = _clip(NEEDS[wrt])
        return m.jod_video(t, r, frames_per_second=FPS, wrt=wrt, fixation_point=GAZE if foveated else None)
    return dict(foveated=foveated), run


def _jod_gazes():
    def run(m):
        t, r = _clip(("test",))
        gaze = torch.tensor([[30.0, 20.0], [60.0, 33.0], [100.0, 50.0]])
        assert gaze.shape[0] == G
        return m.jod_gazes(t, r, gaze, frames_per_second=FPS)
    return dict(foveated=True), run


def _calibration_images(grad):
    def run(m):
        t, r = _stills()
        return m.calibration_jod_images(t, r, m.parameter_tensor().requires_grad_(grad))
    return {}, run


def _calibration_video(theta_grad, phi_grad=None):
    """phi_grad None: no temporal=."""
    def run(m):
        t, r = _clip()
        phi = None if phi_grad is None else m.temporal_parameter_tensor().requires_grad_(phi_grad)
        return m.calibration_jod_video(t, r, m.parameter_tensor().requires_grad_(theta_grad), frames_per_second=FPS, temporal=phi)
    return {}, run


def _display(video, grad):
    def run(m):
        t, r = _clip() if video else _stills()
        psi = m.display_parameter_tensor().requires_grad_(grad)
        return m.display_jod_video(t, r, psi, frames_per_second=FPS) if video else m.display_jod_images(t, r, psi)
    return {}, run


CASES = {
    "jod_images_test": _jod_images("test"),
    "jod_images_both": _jod_images("both"),
    "jod_video_test": _jod_video("test"),
    "jod_video_both": _jod_video("both"),
    "jod_video_test_foveated": _jod_video("test", foveated=True),
    "jod_gazes": _jod_gazes(),
    "calibration_jod_images_theta": _calibration_images(True),
    "calibration_jod_video_theta": _calibration_video(True),
    "calibration_jod_video_phi": _calibration_video(False, True),
    "calibration_jod_video_theta_phi": _calibration_video(True, True),
    "display_jod_images_psi": _display(False, True),
    "display_jod_video_psi": _display(True, True),
    # nothing requires grad: the forward alone
    "calibration_jod_images_forward": _calibration_images(False),
    "calibration_jod_video_forward": _calibration_video(False),
    "calibration_jod_video_temporal_forward": _calibration_video(False, False),
    "display_jod_images_forward": _display(False, False),
    "display_jod_video_forward": _display(True, False),
}


def _once(run, m):
    jod = run(m)
    if jod.requires_grad:
        jod.sum().backward()
    torch.cuda.synchronize()


def _brackets_closed(calls):
    """Every fvvdp_ctx_set_slope_maps(on) is followed by exactly one forward and then fvvdp_ctx_set_slope_maps(None)."""
    names = [c[0] for c in calls]
    for i, c in enumerate(calls):
        if c[0] == "fvvdp_ctx_set_slope_maps" and c[-1] == "ptr":
            if i + 2 >= len(calls) or not (names[i + 1] in ("fvvdp_bands_forward", "fvvdp_images_forward_pool")
                    and calls[i + 2] == ["fvvdp_ctx_set_slope_maps", "ptr", "null"]):
                return False
        if c[0] == "fvvdp_ctx_set_slope_maps" and c[-1] == "null" and (i < 2 or calls[i - 2][0] != "fvvdp_ctx_set_slope_maps"):
            return False
    return True


@pytest.mark.parametrize("name", sorted(CASES))
def test_native_call_sequence(fv, fixture_file, monkeypatch, name):
    from fovvideovdp_amd import _native
    kwargs, run = CASES[name]
    m = fv.fvvdp(display_name="standard_4k", batch_frames=2, quiet=True, device=DEV, **kwargs)
    m.grad_batch = 2
    _once(run, m)
    rec = _Recorder(_native.lib())
    monkeypatch.setattr(_native, "lib", lambda: rec)
    _once(run, m)
    monkeypatch.undo()
    calls = rec.calls
    names = [c[0] for c in calls]
    # what a recording must show whatever commit it is made on
    assert _brackets_closed(calls)
    uses_slopes = name in ("jod_images_both", "jod_video_both", "calibration_jod_video_phi", "calibration_jod_video_theta_phi",
                           "display_jod_images_psi", "display_jod_video_psi")
    assert (names.count("fvvdp_ctx_set_slope_maps") > 0) == uses_slopes
    assert names.count("fvvdp_ctx_set_params") == (2 if name.startswith("calibration") else 0)
    if RECORD:
        fixture_file[name] = calls
        return
    assert calls == fixture_file[name]
