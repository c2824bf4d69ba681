"""Differentiable many-tests JOD: fvvdp.jod_tests and its autograd function (include/fvvdp_hip_tests_grad.h).

The forward makes the launches of fvvdp.predict_tests (multitest.launch_passes: the same quads, slots, groups, batch schedule
and split into passes), so row k is bit-identical to it, and so to jod_video(tests[k], reference); no flag is read back.  The
backward runs, per backward batch and test, the single-pair ingest and map-writing pyramid pass of jod_video.  The test side is
jod_video's own (fvvdp_video_grad_frames per test, into that test's clip-long level-0 buffer): nothing after the layer gradient
can be shared there.  The reference side is shared: fvvdp_tests_ref_grad_layer sums the reference's layer gradients of up to
four tests per launch, reading what depends on the reference only once per launch, and the coarse-to-fine sweep, level 0, the
temporal transpose and the display model's derivative run once per batch or clip instead of once per test.  The maps that depend
on the reference only (L_bkg, S, the slope planes) are one set of buffers that every pass rewrites with the same values; per
test only D and the contrast planes are kept, for the tests of one layer call.  Setup, buffers and the map-writing pass are
grad_passes.py's, as jod_video's."""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .grad_passes import ClipBuffers, ClipSetup, Maps, _ptr, batches, grad_batch_size, workspace_bytes
from .multitest import _is_source_object, launch_passes
from .video_grad import GRAD_PLANES, clip_arguments

# Largest group of tests one tests_ref_layer_kernel launch takes: 0 = the library's default (FVVDP_TESTS_GRAD_GROUP_MAX = 4), or
# 1, 2, 4.  The gradient does not depend on it, bit for bit; smaller groups only make more launches (tests, A/B runs).
GROUP_MAX = 0
WRT = ("tests", "reference", "both")
# per-test planes of a map set (D 2 + contrast 4), the planes the kernel reads once for all tests (L_bkg 1 + S 2 + slopes 2 +
# the reference's contrast 2: an upper bound, the last two lie inside every set's contrast planes), the reference's workspace
# (GLR + GX + GG of both channels) and the test side's (layer + sweep gradients of both channels)
TEST_PLANES, SHARED_PLANES, REF_WORK_PLANES, TEST_WORK_PLANES = 6, 7, 6, 4


def check_wrt(wrt):
    if wrt not in WRT:
        raise ValueError('wrt must be "tests", "reference" or "both", got %r' % (wrt,))
    return wrt


def map_sets(metric, n_tests):
    """Map sets (D and contrast of one test each) a backward batch holds: the tests of one layer call.  As many as the largest
    launch group takes, or metric.tests_grad_sets (fewer: more layer calls per batch, the same bits)."""
    sets = getattr(metric, "tests_grad_sets", None)
    sets = nat.TESTS_GRAD_GROUP_MAX if sets is None else int(sets)
    return max(1, min(sets, n_tests))


def tests_grad_planes(wrt, sets):
    """fp32 values per pyramid pixel and frame of a backward batch: "tests" holds what jod_video's test side holds (one full
    map set and its workspace, 13); "reference" `sets` map sets of 6, the 7 shared planes and the reference's workspace of 6
    (37 at four sets); "both" the test side's workspace of 4 on top."""
    check_wrt(wrt)
    if wrt == "tests":
        return GRAD_PLANES
    ref = sets * TEST_PLANES + SHARED_PLANES + REF_WORK_PLANES
    return ref if wrt == "reference" else ref + TEST_WORK_PLANES


class _TestMaps:
    """A further map set beside the Maps `first`: D and contrast of its own, L_bkg, S, the slope planes and the pooling scratch
    are `first`'s."""

    def __init__(self, metric, first, W, H, n_bands, gb):
        self.maps_arr = (nat.BandMaps * n_bands)()
        self._keep = []
        for b, (w, h) in enumerate(metric._level_sizes(W, H, n_bands)[:n_bands]):
            D = torch.empty((gb, 2, h, w), dtype=torch.float32, device=metric.device)
            Cn = torch.empty((gb, 4, h, w), dtype=torch.float32, device=metric.device)
            self.maps_arr[b].d_D, self.maps_arr[b].d_contrast = D.data_ptr(), Cn.data_ptr()
            self.maps_arr[b].d_lbkg, self.maps_arr[b].d_S = first.maps_arr[b].d_lbkg, first.maps_arr[b].d_S
            self._keep += [D, Cn]
        self.slopes, self.q_scratch, self.jod_scratch = first.slopes, first.q_scratch, first.jod_scratch


def _forward(metric, tests, r, fps):
    """JOD [T] and Q_per_ch [T, n_bands, 2, N] on the device: the launches of predict_tests, no flag read back."""
    T = len(tests)
    _, _, N, H, W = r.shape
    res, pl = launch_passes(metric, list(tests) + [r], fps, W, H, N, "jod_tests needs a display model with a closed form for "
                            "float input (sRGB, gamma, PQ, linear or absolute); a user photometry class has none")
    nq = pl.n_bands * 2 * N
    return res[T * nq + 1:], res[:T * nq].view(T, pl.n_bands, 2, N)


def _backward(metric, tests, r, fps, Q, gamma, need_t, need_r):
    """([gamma[k] * dJOD_k/dtests[k] or None], sum_k gamma[k] * dJOD_k/dr or None) for the contiguous device clips
    [1, C, N, H, W]; need_t: per test, whether its gradient is wanted."""
    T, lib = len(tests), nat.lib()
    s = ClipSetup(metric, tests[0], fps, r)
    N, HW, dev = s.N, s.H * s.W, metric.device
    wanted = [k for k in range(T) if need_t[k]]
    wrt = "both" if wanted and need_r else ("reference" if need_r else "tests")
    sets = map_sets(metric, T) if need_r else 1
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, tests_grad_planes(wrt, sets))
    vb = workspace_bytes(lib.fvvdp_video_grad_workspace, s.W, s.H, s.n_bands, gb) if wanted else 0
    rb = workspace_bytes(lib.fvvdp_tests_ref_grad_workspace, s.W, s.H, s.n_bands, gb, T) if need_r else 0
    px = sum(w * h for w, h in metric._level_sizes(s.W, s.H, s.n_bands)[:s.n_bands])
    # beside what ClipBuffers counts (one test's clip-long buffer and result, the reference's, one full map set): the other
    # tests' clip-long buffers and results, the other map sets
    extra = max(0, len(wanted) - 1) * (N * HW * 8 + r.numel() * 4) + (sets - 1) * TEST_PLANES * gb * px * 4
    buf = ClipBuffers("jod_tests", metric, s, r, gb, vb, bool(wanted), rb, maps=False, extra_bytes=extra)
    g0 = {k: buf.g0 if i == 0 else torch.empty_like(buf.g0) for i, k in enumerate(wanted)}
    grads = {k: buf.grad if i == 0 else torch.empty_like(buf.grad) for i, k in enumerate(wanted)}
    first = buf.use_maps(Maps(metric, s.W, s.H, s.n_bands, 4, gb))
    msets = [first] + [_TestMaps(metric, first, s.W, s.H, s.n_bands, gb) for _ in range(sets - 1)]
    resident = (nat.BandMaps * (sets * s.n_bands))()             # the records of the sets, in the order a layer call takes them
    for j, m in enumerate(msets):
        for b in range(s.n_bands):
            resident[j * s.n_bands + b] = m.maps_arr[b]
    prm = s.params()
    gamma = gamma.to(device=dev, dtype=torch.float32).reshape(T).contiguous()
    for b0, nb in batches(N, gb):
        filled, added = [], 0
        for k in range(T):
            if not need_r and not need_t[k]:
                continue                                            # a test without a gradient costs no backward work
            m = msets[len(filled)]
            s.write_maps(m, None, b0, nb, buf.oob, (tests[k], r))   # the pass jod_video runs: its maps, bit for bit
            if need_t[k]:
                nat.check(lib.fvvdp_video_grad_frames(s.W, s.H, s.n_bands, nb, C.byref(prm), C.byref(s.pp), _ptr(Q[k]), N, b0,
                                                      _ptr(gamma, 4 * k), m.maps_arr, _ptr(g0[k]), _ptr(buf.work),
                                                      buf.work_bytes, s.stream))
            if need_r:
                filled.append(k)
                if len(filled) == sets or k == T - 1:
                    nat.check(lib.fvvdp_tests_ref_grad_layer(s.W, s.H, s.n_bands, nb, T, filled[0], len(filled), int(GROUP_MAX),
                                                             added, C.byref(prm), C.byref(s.pp), _ptr(Q), N, b0, _ptr(gamma),
                                                             resident, first.slopes, _ptr(buf.work_r), buf.ref_bytes, s.stream))
                    filled, added = [], 1
        if need_r:
            nat.check(lib.fvvdp_tests_ref_grad_finish(s.W, s.H, s.n_bands, nb, T, N, b0, _ptr(buf.g0_r), _ptr(buf.work_r),
                                                      buf.ref_bytes, s.stream))
    out = [None] * T
    for k in wanted:
        out[k] = buf.input_grad(lib, s, tests[k], g0[k], grads[k])
    grad_r = buf.input_grad(lib, s, r, buf.g0_r, buf.grad_r) if need_r else None
    return out, grad_r


class JodTestsFunction(torch.autograd.Function):
    """reference, tests... [1, C, N, H, W] (contiguous, of one dtype -- float32, float16 or bfloat16 -- on the metric's device)
    -> JOD [T] (fp32).  The tensors saved for backward are the clips as they came, and each gradient has its clip's dtype.
    _place() detaches what `wrt` treats as a constant, so needs_input_grad names the gradients to make."""

    @staticmethod
    def forward(ctx, reference, metric, fps, *tests):
        with torch.cuda.device(metric.device):
            jod, Q = _forward(metric, tests, reference, fps)
        ctx.metric, ctx.fps = metric, fps
        ctx.save_for_backward(reference, Q, *tests)
        return jod.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_jod):
        reference, Q = ctx.saved_tensors[:2]
        tests = ctx.saved_tensors[2:]
        need_r, need_t = ctx.needs_input_grad[0], list(ctx.needs_input_grad[3:])
        grads, grad_r = [None] * len(tests), None
        if need_r or any(need_t):
            with torch.cuda.device(ctx.metric.device):
                grads, grad_r = _backward(ctx.metric, tests, reference, ctx.fps, Q, grad_jod, need_t, need_r)
        return (grad_r, None, None) + tuple(grads)


def tests_arguments(metric, tests, reference, dim_order, frames_per_second, wrt):
    """What jod_tests accepts, checked before any device work: what predict_tests refuses, then per clip what jod_video
    refuses (clip_arguments).  Returns the tests and the reference as [1, C, N, H, W] tensors of one dtype, not yet placed."""
    if metric.foveated:
        raise RuntimeError("jod_tests covers the non-foveated metric (no fixation_point): for a foveated metric call jod_video() "
                           "once per test")
    if metric.do_heatmap:
        raise RuntimeError("jod_tests makes no heat maps: build the metric without heatmap=, or call jod_video() per test")
    if _is_source_object(reference) or _is_source_object(tests) or \
            (isinstance(tests, (list, tuple)) and any(_is_source_object(t) for t in tests)):
        raise RuntimeError("jod_tests takes arrays or tensors: a fvvdp_video_source object or a YUV frame source has no gradient "
                           "here (planar YUV: jod_video_yuv(), one test per call)")
    if not isinstance(tests, (list, tuple)) or len(tests) < 1:
        raise RuntimeError("tests must be a list or tuple of at least one clip, each shaped like the reference")
    one = {"tests": "test", "reference": "reference", "both": "both"}[wrt]      # the word jod_video has for it
    pairs = [clip_arguments("jod_tests", metric, t, reference, dim_order, frames_per_second, one) for t in tests]
    ts, r = [p[0] for p in pairs], pairs[0][1]
    # float_pair's rule on the whole list: one dtype passes as it is, a mixed list is upcast inside autograd's view
    if len({t.dtype for t in ts} | {r.dtype} | {p[1].dtype for p in pairs}) > 1:
        ts, r = [t.float() for t in ts], r.float()
    return ts, r


def _place(metric, ts, r, wrt):
    """The clips contiguous on the metric's device, what `wrt` treats as a constant detached (image_grad.place for a list)."""
    metric._check_device()
    if wrt == "tests":
        r = r.detach()
    elif wrt == "reference":
        ts = [t.detach() for t in ts]
    return [t.to(metric.device).contiguous() for t in ts], r.to(metric.device).contiguous()


def jod_tests(metric, tests, reference, dim_order="BCFHW", frames_per_second=0, wrt="tests"):
    """fvvdp.jod_tests (see there)."""
    check_wrt(wrt)
    ts, r = tests_arguments(metric, tests, reference, dim_order, frames_per_second, wrt)
    ts, r = _place(metric, ts, r, wrt)
    return JodTestsFunction.apply(r, metric, float(frames_per_second), *ts)
