"""fvvdp.predict_gazes: one (test, reference) clip scored under G gaze traces in one pass (include/fvvdp_hip_gaze.h).

The temporal channels are made once per batch of frames, as predict makes them; the pyramid pass then runs once per group of
gazes and evaluates per band pixel what does not depend on the gaze once (multigaze_kernel.hpp).  Gaze g's results are
bit-identical to predict(test, ref, fixation_point=fixation_points[g]) on the same metric."""
import ctypes as C
import logging

import numpy as np
import torch

from . import _native as nat
from .display_model import native_geometry
from .fvvdp import _refuse_grad
from .video_source import fvvdp_video_source_array


def _gaze_array(metric, fixation_points, width, height, N):
    """fixation_points [G, 2] or [G, N, 2] in frame pixels -> fp32 [G, N, 2]."""
    if isinstance(fixation_points, torch.Tensor):
        fp = fixation_points.detach().cpu().numpy()
    else:
        fp = np.asarray(fixation_points)
    ok = fp.ndim in (2, 3) and fp.shape[0] >= 1 and fp.shape[-1] == 2 and (fp.ndim == 2 or fp.shape[1] == N)
    if not ok:
        raise RuntimeError("fixation_points must be a [G, 2] array (one fixed gaze per row) or a [G, N_frames, 2] array "
                           "(one trace per gaze) with G >= 1, got shape %s for %d frames" % (tuple(fp.shape), N))
    return np.ascontiguousarray(np.stack([metric._fixation(fp[g], width, height, N) for g in range(fp.shape[0])]))


def predict_gazes(metric, test, reference, fixation_points, dim_order="BCFHW", frames_per_second=0):
    """fvvdp.predict_gazes (see there)."""
    if not metric.foveated:
        raise RuntimeError("predict_gazes needs a foveated metric (fvvdp(foveated=True)): without foveation the gaze does not "
                           "enter the result, use predict()")
    if metric.do_heatmap:
        raise RuntimeError("predict_gazes makes no heat maps: build the metric without heatmap=, or call predict() per gaze")
    if native_geometry(metric.display_geometry) is None:
        raise RuntimeError("predict_gazes covers the stock display geometry; a user display_geometry class takes the map "
                           "path of predict(), one gaze per call")
    _refuse_grad(test)
    _refuse_grad(reference)
    vs = fvvdp_video_source_array(test, reference, frames_per_second, dim_order=dim_order,
                                  display_photometry=metric.display_photometry, color_space_name=metric.color_space)
    height, width, N = vs.get_video_size()
    fix = _gaze_array(metric, fixation_points, width, height, N)
    metric._check_device()
    with torch.cuda.device(metric.device):
        return _on_device(metric, vs, fix, width, height, N)


def _on_device(metric, vs, fix, width, height, N):
    dev, lib, G = metric.device, nat.lib(), fix.shape[0]
    pl = metric._clip_plan(vs)                          # the batches predict() takes: same work decomposition, same sums
    n_bands, rho_band, fl, taps, widx, feeder, schedule = pl.n_bands, pl.rho_band, pl.fl, pl.taps, pl.widx, pl.feeder, pl.schedule
    ctx = metric._context(width, height, n_bands, pl.planes, pl.batch, rho_band)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    nq = n_bands * 2 * N
    res = torch.zeros(G * nq + 1 + G, dtype=torch.float32, device=dev)        # Q_per_ch of every gaze | range flag | JOD of every gaze
    Q = res[:G * nq]
    oob = res[G * nq:G * nq + 1].view(torch.int32)
    jod = res[G * nq + 1:]
    gaze = torch.from_numpy(fix).to(dev)                                       # [G, N, 2], uploaded once
    nbytes = C.c_size_t()
    nat.check(lib.fvvdp_gaze_workspace(width, height, n_bands, G, max(schedule), C.byref(nbytes)))
    work = torch.empty(nbytes.value // 4, dtype=torch.float32, device=dev)
    geom, pp = metric._geom_struct(), metric._pool_params()
    b0 = 0
    try:
        for nb in schedule:
            idx = np.ascontiguousarray(widx[b0:b0 + fl - 1 + nb])
            feeder(ctx, idx, taps, fl, nb, oob, stream)
            gp = C.c_void_p(gaze.data_ptr() + 8 * b0)
            if b0 + nb == N:
                nat.check(lib.fvvdp_bands_forward_gazes_pool(ctx.handle, nb, G, gp, 2 * N, C.c_void_p(Q.data_ptr()), N, b0,
                                                             C.byref(geom), C.c_void_p(work.data_ptr()), nbytes.value, C.byref(pp),
                                                             C.c_void_p(jod.data_ptr()), stream))
            else:
                nat.check(lib.fvvdp_bands_forward_gazes(ctx.handle, nb, G, gp, 2 * N, C.c_void_p(Q.data_ptr()), N, b0,
                                                        C.byref(geom), C.c_void_p(work.data_ptr()), nbytes.value, stream))
            b0 += nb
    except BaseException:
        if hasattr(feeder, "release"):
            feeder.release(synced=False)
        raise
    res_h = metric._to_host(res)                         # the one host synchronisation of the call
    stats = {'Q_per_ch': res_h[:G * nq].view(G, n_bands, 2, N).numpy(), 'rho_band': rho_band,
             'frames_per_second': vs.get_frames_per_second(), 'width': width, 'height': height, 'N_frames': N}
    if int(res_h[G * nq:G * nq + 1].view(torch.int32)[0]) != 0:
        logging.warning("Pixel outside the valid range 0-1")
    if hasattr(feeder, "release"):
        feeder.release(synced=True)
    return jod, stats
