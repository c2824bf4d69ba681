"""fvvdp.predict_tests: T test clips scored against one reference in one pass (include/fvvdp_hip_tests.h).

The level planes of a video context are float4 per pixel, two streams each (a "quad").  Streams 0 .. T-1 are the tests, stream T
is the reference; quad q holds streams 2q and 2q+1, so the reference is ingested and its level 0 written once instead of T
times, and the pyramid pass (multitest_kernel.hpp) evaluates per band pixel what depends on the reference only once per group
of quads.  Test k's results are bit-identical to predict(tests[k], reference) on the same metric ("Many
tests per reference")."""
import ctypes as C
import logging
from types import SimpleNamespace

import numpy as np
import torch

from . import _native as nat
from .fvvdp import _PipelinedSourceFeeder, _refuse_grad
from .video_source import fvvdp_video_source, fvvdp_video_source_array, reshuffle_dims


def quad_plan(n_tests, n, group_max=nat.TESTS_GROUP_MAX):
    """The stream -> (quad, component) convention of include/fvvdp_hip_tests.h and the launch groups of the pyramid pass for
    `n_tests` tests in batches of `n` frames, as fvvdp_bands_forward_tests lays them out.  Pure host arithmetic.
      quads   [(stream in (x, z), stream in (y, w))]; stream k < n_tests is test k, stream n_tests the reference
      slot0   first frame slot of every quad (quad q: slots [q n, q n + n))
      groups  one dict per launch of a level: 'quads' (the reference's quad first), 'store' (the quads whose next level this
              launch writes) and 'tests' (the tests it evaluates)"""
    if n_tests < 1 or n < 1:
        raise ValueError("n_tests and n must be >= 1")
    T = int(n_tests)
    n_quads = T // 2 + 1
    quads = [(2 * q, min(2 * q + 1, T)) for q in range(n_quads)]
    ref_quad = n_quads - 1
    group_max = max(1, min(int(group_max), nat.TESTS_GROUP_MAX))
    if n_quads > 1:
        group_max = max(group_max, 2)
    groups, q0, first = [], 0, True
    while True:
        others = list(range(q0, min(q0 + group_max - 1, ref_quad)))
        tests = [T - 1] if (first and T % 2 == 1) else []
        for q in others:
            tests += [2 * q, 2 * q + 1]
        groups.append({'quads': [ref_quad] + others, 'store': ([ref_quad] if first else []) + others, 'tests': tests})
        q0 += len(others)
        first = False
        if q0 >= ref_quad:
            break
    return SimpleNamespace(n_tests=T, n=int(n), n_quads=n_quads, quads=quads, slot0=[q * int(n) for q in range(n_quads)],
                           ref_quad=ref_quad, groups=groups)


def _is_source_object(x):
    return isinstance(x, fvvdp_video_source) or (hasattr(x, "get_test_frame") and hasattr(x, "get_reference_frame"))


def predict_tests(metric, tests, reference, dim_order="BCFHW", frames_per_second=0, fixation_point=None):
    """fvvdp.predict_tests (see there)."""
    if metric.foveated or fixation_point is not None:
        raise RuntimeError("predict_tests covers the non-foveated metric (no fixation_point): for a foveated metric call predict() "
                           "once per test, or predict_tests_foveated()")
    streams, width, height, N = clip_arguments("predict_tests", metric, tests, reference, dim_order, frames_per_second)
    metric._check_device()
    with torch.cuda.device(metric.device):
        return _on_device(metric, streams, dim_order, frames_per_second, width, height, N)


def clip_arguments(name, metric, tests, reference, dim_order, frames_per_second):
    """The checks on the clips of predict_tests and of predict_tests_foveated (`name`, for the sentences), all before any device
    work.  Returns (streams, width, height, N): the T tests and then the reference, as tensors where they came."""
    if metric.do_heatmap:
        raise RuntimeError("%s makes no heat maps: build the metric without heatmap=, or call predict() per test" % name)
    if _is_source_object(reference) or _is_source_object(tests) or \
            (isinstance(tests, (list, tuple)) and any(_is_source_object(t) for t in tests)):
        raise RuntimeError("%s takes arrays or tensors: a fvvdp_video_source object or a YUV frame source goes through "
                           "predict_video_source(), one test per call" % name)
    if not isinstance(tests, (list, tuple)) or len(tests) < 1:
        raise RuntimeError("tests must be a list or tuple of at least one clip, each shaped like the reference")
    as_tensor = fvvdp_video_source_array._as_tensor
    for k, t in enumerate(tests):
        if not hasattr(t, "shape") or not hasattr(t, "dtype") or tuple(t.shape) != tuple(reference.shape) or \
                as_tensor(t).dtype != as_tensor(reference).dtype:
            raise RuntimeError("test %d differs from the reference in shape or dtype (%s %s against %s %s): the tests share one ingest "
                               "with the reference; predict() converts such a pair, call it for this test"
                               % (k, tuple(getattr(t, "shape", ())), getattr(t, "dtype", None), tuple(reference.shape), reference.dtype))
    for t in tests:
        _refuse_grad(t)
    _refuse_grad(reference)
    ref_t = as_tensor(reference)
    streams = [as_tensor(t) for t in tests] + [ref_t]
    # (fvvdp_video_source_array checks dim_order, the channel count and that a clip states its frame rate)
    vs0 = fvvdp_video_source_array(streams[0], ref_t, frames_per_second, dim_order=dim_order,
                                   display_photometry=metric.display_photometry, color_space_name=metric.color_space)
    height, width, N = vs0.get_video_size()
    if N < 2:
        raise RuntimeError("%s needs clips of at least 2 frames: for a single frame use predict_images() with the "
                           "reference repeated" % name)
    if vs0.test_video.shape[0] != 1:
        raise RuntimeError("Only batch size 1 is supported (as in the reference's sliding-window code)")
    return streams, width, height, N


def _on_device(metric, streams, dim_order, fps, width, height, N, gaze=None, name="predict_tests"):
    """The device part of predict_tests and, with the fp32 [N, 2] trace `gaze`, of predict_tests_foveated (`name`, for the
    sentence).  Returns (JOD [T], stats), or None where the pass under a gaze does not cover the context (launch_passes)."""
    dev, T = metric.device, len(streams) - 1
    h2d = sum(s.numel() * s.element_size() for s in streams if s.device != dev)
    # every clip crosses to the device once, the reference included, and lies there as the ingest kernels read it
    streams = [reshuffle_dims(s.to(dev), in_dims=dim_order, out_dims="BCFHW").contiguous() for s in streams]
    res, pl = launch_passes(metric, streams, fps, width, height, N, "%s needs a display model the ingest kernels "
                            "evaluate (float input behind a user photometry class goes through predict(), one test per call)" % name,
                            gaze)
    if res is None:
        return None
    n_bands, nq = pl.n_bands, pl.n_bands * 2 * N
    metric.last_h2d_bytes = h2d
    res_h = metric._to_host(res)                          # the one host synchronisation of the call
    stats = {'Q_per_ch': res_h[:T * nq].view(T, n_bands, 2, N).numpy(), 'rho_band': pl.rho_band,
             'frames_per_second': fps, 'width': width, 'height': height, 'N_frames': N}
    if int(res_h[T * nq:T * nq + 1].view(torch.int32)[0]) != 0:
        logging.warning("Pixel outside the valid range 0-1")
    return res[T * nq + 1:], stats


def launch_passes(metric, streams, fps, width, height, N, refusal, gaze=None):
    """The launches of predict_tests for the T + 1 contiguous [1, C, N, H, W] device clips `streams` (the tests, then the
    reference): the one launch loop of predict_tests, of tests_grad.jod_tests and of tests_fov.predict_tests_foveated.  Returns
    (res, plan): res the device tensor Q_per_ch [T][bands][2][N] | range flag | JOD [T], nothing of it read back; plan the clip
    plan of the call.  `refusal`: the sentence for a source whose display model the ingest kernels do not evaluate.  `gaze`: None,
    or the fp32 [N, 2] gaze trace of a foveated metric with the stock geometry -- the pyramid pass is then that of
    include/fvvdp_hip_tests_fov.h, and res is None (nothing ingested, no pyramid launch) where that pass does not cover the
    context."""
    dev, T = metric.device, len(streams) - 1

    def source(a, b):
        return fvvdp_video_source_array(streams[a], streams[b], fps, dim_order="BCFHW",
                                        display_photometry=metric.display_photometry, color_space_name=metric.color_space)

    pl = metric._clip_plan(source(0, T))                  # the batches predict() takes: same work decomposition, same sums
    if isinstance(pl.feeder, _PipelinedSourceFeeder):
        raise RuntimeError(refusal)
    nq = pl.n_bands * 2 * N
    res = torch.zeros(T * nq + 1 + T, dtype=torch.float32, device=dev)          # Q_per_ch of every test | range flag | JOD of every test
    oob = res[T * nq:T * nq + 1].view(torch.int32)
    # Scratch: a pass over t tests holds (t // 2 + 1) x batch frame slots.  The batch stays predict()'s (the chunk heights, and with
    # them the grouping of the partial sums, follow it), so where the slots of all tests exceed the budget the tests are taken
    # in several passes, each with the reference.
    per_frame = width * height * pl.planes * 4 * 1.34
    budget = getattr(metric, "tests_scratch_bytes", None)          # (an attribute a caller or a test may set; None: the default)
    if budget is None:
        budget = min(96e9, 0.4 * torch.cuda.get_device_properties(dev).total_memory)
    max_quads = max(1, int(budget // (pl.batch * per_frame)))
    per_pass = T if T // 2 + 1 <= max_quads else max(1, 2 * max_quads - 1)
    fov = None
    if gaze is not None:
        fov = (gaze, metric._geom_struct())
        # asked of the context of the first (largest) pass, before anything is ingested
        ctx = metric._context(width, height, pl.n_bands, pl.planes, (min(per_pass, T) // 2 + 1) * pl.batch, pl.rho_band)
        covered = C.c_int(0)
        nat.check(nat.lib().fvvdp_tests_fov_covered(ctx.handle, C.byref(fov[1]), C.byref(covered),
                                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        if not covered.value:
            return None, pl
    for k0 in range(0, T, per_pass):
        ks = list(range(k0, min(k0 + per_pass, T)))
        _one_pass(metric, pl, source, ks, T, res[k0 * nq:(k0 + len(ks)) * nq], oob, res[T * nq + 1 + k0:], width, height, N, fov)
    return res, pl


def _one_pass(metric, pl, source, ks, ref, Q, oob, jod, width, height, N, fov=None):
    """Tests `ks` (indices into the stream list) against stream `ref`: Q [len(ks)][bands][2][N] and jod [len(ks)] are written.
    `fov`: None, or (gaze [N, 2], geometry struct) for the pass under a gaze."""
    dev, lib, t = metric.device, nat.lib(), len(ks)
    qp = quad_plan(t, max(pl.schedule))
    local = ks + [ref]                                    # stream number of the pass -> stream of the call
    feeders = [metric._make_feeder(source(local[a], local[b]), width, height) for a, b in qp.quads]
    ctx = metric._context(width, height, pl.n_bands, pl.planes, qp.n_quads * pl.batch, pl.rho_band)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    nbytes = C.c_size_t()
    nat.check(lib.fvvdp_tests_workspace(width, height, pl.n_bands, t, max(pl.schedule), C.byref(nbytes)))
    work = torch.empty(nbytes.value // 4, dtype=torch.float32, device=dev)
    pp = metric._pool_params()
    fl, b0 = pl.fl, 0
    for nb in pl.schedule:
        idx = np.ascontiguousarray(pl.widx[b0:b0 + fl - 1 + nb])
        for q, feed in enumerate(feeders):
            feed(ctx, idx, pl.taps, fl, nb, oob, stream, slot0=q * nb)
        last = b0 + nb == N                               # the batch that completes the clip also pools
        args = (ctx.handle, nb, t, C.c_void_p(Q.data_ptr()), N, b0)
        if fov is not None:                               # the batch's rows of the gaze trace, then the geometry
            fxa = np.ascontiguousarray(fov[0][b0:b0 + nb], dtype=np.float32)
            args += (nat.fptr(fxa), C.byref(fov[1]))
        args += (C.c_void_p(work.data_ptr()), nbytes.value)
        args += (C.byref(pp), C.c_void_p(jod.data_ptr()), stream) if last else (stream,)
        if fov is None:
            nat.check(lib.fvvdp_bands_forward_tests_pool(*args) if last else lib.fvvdp_bands_forward_tests(*args))
        else:
            nat.check(lib.fvvdp_bands_forward_tests_fov_pool(*args) if last else lib.fvvdp_bands_forward_tests_fov(*args))
        b0 += nb
