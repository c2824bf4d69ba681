"""fvvdp.predict_tests_foveated: T test clips scored against one reference under one gaze trace in one pass
(include/fvvdp_hip_tests_fov.h).

The quads, the ingest and the launch loop are predict_tests' (multitest.py); the pyramid pass is multitest_fov_kernel.hpp, which
evaluates per band pixel what depends on the reference and the gaze only -- L_bkg, the eccentricity, the cell of the CSF table
and its 3-D interpolation -- once per group of quads.  Test k's results are bit-identical to
predict(tests[k], reference, fixation_point=fixation_point) on the same metric ("Many tests per reference
under a gaze")."""
import logging

import numpy as np
import torch

from . import multitest
from .display_model import native_eotf, native_geometry
from .fvvdp import _is_float_type, _sample_type

NAME = "predict_tests_foveated"


def predict_tests_foveated(metric, tests, reference, dim_order="BCFHW", frames_per_second=0, fixation_point=None):
    """fvvdp.predict_tests_foveated (see there)."""
    if not metric.foveated:
        raise RuntimeError("%s needs a foveated metric (fvvdp(foveated=True)): without foveation the gaze does not enter the "
                           "result, use predict_tests()" % NAME)
    if native_geometry(metric.display_geometry) is None:
        raise RuntimeError("%s covers the stock display geometry; a user display_geometry class takes the map path of "
                           "predict(), one test per call" % NAME)
    streams, width, height, N = multitest.clip_arguments(NAME, metric, tests, reference, dim_order, frames_per_second)
    if _is_float_type(_sample_type(streams[-1].dtype)[0]) and native_eotf(metric.display_photometry) is None:
        raise RuntimeError("%s needs a display model the ingest kernels evaluate (float input behind a user photometry class "
                           "goes through predict(), one test per call)" % NAME)
    if fixation_point is not None:
        shape = tuple(fixation_point.shape) if hasattr(fixation_point, "shape") else np.shape(fixation_point)
        if shape not in ((2,), (N, 2)):
            raise RuntimeError("fixation_point must be [x, y] or an [N_frames, 2] array, got shape %s for %d frames" % (shape, N))
    fix = metric._fixation(fixation_point, width, height, N)
    metric._check_device()
    with torch.cuda.device(metric.device):
        out = multitest._on_device(metric, streams, dim_order, frames_per_second, width, height, N, gaze=fix, name=NAME)
        shared = out is not None
        if not shared:
            out = _loop(metric, tests, reference, dim_order, frames_per_second, fix)
    out[1]['shared_pass'] = shared
    return out


def _loop(metric, tests, reference, dim_order, fps, fix):
    """A context with a band that the shared pass does not cover (its slice of the CSF table does not fit the LDS): predict() per
    test, queued without waiting, and one host synchronisation for all."""
    runs = [metric.predict(t, reference, dim_order=dim_order, frames_per_second=fps, fixation_point=fix, sync=False) for t in tests]
    T, st = len(runs), runs[0][1]
    nq = st['Q_per_ch'].numel()
    res_h = metric._to_host(torch.cat([s['result_buffer'] for _, s in runs])).view(T, nq + 2)     # rows of Q_per_ch | range flag | JOD
    stats = {'Q_per_ch': res_h[:, :nq].reshape((T,) + tuple(st['Q_per_ch'].shape)).numpy()}
    stats.update({k: st[k] for k in ('rho_band', 'frames_per_second', 'width', 'height', 'N_frames')})
    if bool((res_h[:, nq].contiguous().view(torch.int32) != 0).any()):
        logging.warning("Pixel outside the valid range 0-1")
    return torch.stack([q for q, _ in runs]), stats
