"""Still images whose test and reference stacks have image sizes of their own: fvvdp.predict_images_resized,
fvvdp.jod_images_resized, fvvdp.predict_image_pairs_resized and the autograd function of the second
(include/fvvdp_hip_images_resize.h).

Each stack is float32 or uint8 at its own resolution; the target -- the display's resolution unless resize_resolution says
otherwise -- is the size the metric judges at.  The forward resizes inside the still-image ingest (fvvdp_images_channels_resized:
torch's interpolate arithmetic, the clip to [0, 1] and the display model in one kernel) and then makes the launches of
predict_images / jod_images.  The backward is jod_images' per backward batch -- the map-writing pass, once, whatever `wrt` -- and
then, per differentiated side, fvvdp_images_grad_luminance (the still-image sweep down to the luminance of every target pixel) and
the adjoint of the resize (fvvdp_resize_grad of resize_grad, image k as frame k): dJOD/dtest and dJOD/dreference at each stack's
own resolution.  No RGB image at the target size exists at any point.  The launch layer is grad_passes.py's (ResizedImageSetup,
forward_images, Maps)."""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .display_model import native_eotf
from .image_grad import check_wrt, grad_planes, refuse_unsupported
from .grad_passes import (Maps, ResizedImageSetup, _ptr, batches, forward_images, grad_batch_size, image_resize_stream,
                          image_strides, workspace)
from .resize_grad import ADJOINT_FRAMES
from .video_source import fvvdp_video_source_array, reshuffle_dims

HALF = ("float16", "bfloat16")


def _stack(name, what, x, dim_order, half):
    """One stack as a [B, C, h, w] tensor (a view where possible): float32 or uint8 samples; float16 / bfloat16 where `half`
    (jod_images_resized, which upcasts them)."""
    dt = str(getattr(x, "dtype", type(x).__name__)).replace("torch.", "")
    if dt not in ("float32", "uint8") + (HALF if half else ()):
        raise RuntimeError("%s takes float32 or uint8 samples%s; the %s is %s.  %sloat64 and uint16 samples are not supported"
                           % (name, " (float16 and bfloat16 are upcast)" if half else "", what, dt,
                              "F" if half else "Half-precision, f"))
    t = fvvdp_video_source_array._as_tensor(x)
    d = dim_order.upper()
    if len(d) != t.dim():
        raise RuntimeError('Input tensor much have exactly as many dimensions as there are characters in the "dims" parameter')
    if len(set(d)) != len(d) or set(d) - set("BCFHW") or "H" not in d or "W" not in d:
        raise RuntimeError('dim_order must be made of distinct letters of "BCFHW" and contain H and W, got "%s"' % dim_order)
    if "B" not in d:
        raise RuntimeError('%s needs a B axis (the image pairs) in dim_order, got "%s"' % (name, dim_order))
    if "F" in d:
        if t.shape[d.index("F")] != 1:
            raise RuntimeError("%s takes still images: the F axis must have size 1 (clips with frame sizes of their own: "
                               "predict_resized / jod_video_resized)" % name)
        t = t.select(d.index("F"), 0)
        d = d.replace("F", "")
    t = reshuffle_dims(t, d, "BCHW")
    if t.shape[0] < 1:
        raise RuntimeError("no image pairs")
    if t.shape[1] != 1 and t.shape[1] != 3:
        raise RuntimeError('The content must have either 1 or 3 colour channels.')
    return t


def _arguments(name, metric, test, reference, full_screen_resize, resize_resolution, dim_order, half):
    """Everything that is refused before device work (the refusals for inputs that require grad are the caller's).  Returns (test,
    reference) as [B, C, h, w] views, the mode's code and the target (width, height)."""
    if full_screen_resize not in nat.RESIZE_MODES:
        raise RuntimeError("Unknown resize method '%s'" % (full_screen_resize,))
    if native_eotf(metric.display_photometry) is None:
        raise RuntimeError("%s needs a display model with a closed form (sRGB, gamma, PQ, linear or absolute): samples are "
                           "fractional after the resize, so a look-up table or a user photometry class has none" % name)
    t = _stack(name, "test", test, dim_order, half)
    r = _stack(name, "reference", reference, dim_order, half)
    if t.shape[1] != r.shape[1]:
        raise RuntimeError("%s: test and reference differ in their channel counts (%d and %d)" % (name, t.shape[1], r.shape[1]))
    if t.shape[0] != r.shape[0]:
        raise RuntimeError("%s: test and reference differ in their image counts (%d and %d)" % (name, t.shape[0], r.shape[0]))
    if resize_resolution is None:
        resize_resolution = metric.display_geometry.resolution
    Wo, Ho = int(resize_resolution[0]), int(resize_resolution[1])
    for what, w, h in (("resize_resolution", Wo, Ho), ("test", t.shape[3], t.shape[2]), ("reference", r.shape[3], r.shape[2])):
        if not (1 <= w <= nat.RESIZE_MAX_AXIS and 1 <= h <= nat.RESIZE_MAX_AXIS):
            raise RuntimeError("%s: frame size out of range (1..%d per axis): %dx%d (%s)" % (name, nat.RESIZE_MAX_AXIS, w, h, what))
    return t, r, nat.RESIZE_MODES[full_screen_resize], (Wo, Ho)


def _same_size(t, r, size):
    return all((x.shape[3], x.shape[2]) == size for x in (t, r))


def _place(metric, x):
    """The stack [B, C, h, w] on the metric's device with dense planes (h x w contiguous) that do not overlap; what has to be
    copied is copied inside autograd's view."""
    x = x.to(metric.device)
    B, Cn, H, W = x.shape
    fs, ps = image_strides(x)
    # planes of h x w, planes inside an image ([B][C]) or images inside a plane ([C][B]), gaps allowed
    nested = (ps >= H * W and fs >= Cn * ps) or (fs >= H * W and ps >= B * fs)
    return x if x.stride(3) == 1 and x.stride(2) == W and nested else x.contiguous()


def _unit_float(x):
    """What the other entry points take of a stack this one accepts: uint8 codes scaled as the kernels scale them."""
    return x.to(torch.float32) * (1.0 / 255.0) if x.dtype is torch.uint8 else x


def _fix(metric, fixation_point, size, B):
    return metric._fixation(fixation_point, size[0], size[1], B) if metric.foveated else None


def _backward(metric, t, r, mode, size, fix, Q, gamma, need_t, need_r):
    """(gamma[k] * dJOD_k/dt_k, gamma[k] * dJOD_k/dr_k) for the placed stacks t [B, C, h, w] and r [B, C, h', w'], each laid out as
    its stack; None for the one not asked for.  The ingest and the map-writing pyramid pass run once per backward batch."""
    s = ResizedImageSetup(metric, t, r, mode, size)
    B, HW, dev = s.B, s.H * s.W, metric.device
    wrt = "both" if need_t and need_r else ("reference" if need_r else "test")
    gb = grad_batch_size(metric, s.W, s.H, s.n_bands, s.batch, grad_planes(wrt))
    lib = nat.lib()
    maps = Maps(metric, s.W, s.H, s.n_bands, 2, gb)
    if need_r:
        maps.add_slopes()
    sides = []                  # (stack, gradient laid out as the stack, slope planes or None, workspace, its bytes)
    for x, need, reference in ((t, need_t, 0), (r, need_r, 1)):
        if need:
            nbytes, work = workspace(lib.fvvdp_images_grad_luminance_workspace, s.W, s.H, s.n_bands, gb, reference)
            grad = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=dev)
            sides.append((x, grad, maps.slopes if reference else None, work, nbytes))
        else:
            sides.append(None)
    gL = torch.empty((gb, s.H, s.W), dtype=torch.float32, device=dev)
    # the adjoint's workspace: its tables for the larger of the differentiated stacks and ADJOINT_FRAMES first-stage images
    adj_bytes = max(nat.resize_grad_table_bytes(x[0].shape[3], x[0].shape[2]) for x in sides if x is not None) \
        + 4 * min(gb, ADJOINT_FRAMES) * s.C * HW
    adj = torch.empty(adj_bytes, dtype=torch.uint8, device=dev)
    prm = s.params()
    gamma = gamma.to(device=dev, dtype=torch.float32).contiguous()
    for b0, nb in batches(B, gb):
        s.write_maps(maps, fix, b0, nb)
        for side in sides:
            if side is None:
                continue
            x, grad, slopes, work, nbytes = side
            nat.check(lib.fvvdp_images_grad_luminance(s.W, s.H, s.n_bands, nb, C.byref(prm), C.byref(s.pp), _ptr(Q), B, b0,
                                                      _ptr(gamma, 4 * b0), maps.maps_arr, slopes, _ptr(gL), _ptr(work), nbytes,
                                                      s.stream))
            # written with the stack's strides (every sample of the view once; what lies between its planes is not touched)
            xs = image_resize_stream(x, b0)
            nat.check(lib.fvvdp_resize_grad(s.W, s.H, nb, _ptr(gL), C.byref(xs), _ptr(grad, 4 * b0 * image_strides(x)[0]), mode,
                                            C.byref(s.e), nat.fptr(s.w), _ptr(adj), adj_bytes, s.stream))
    return tuple(side[1] if side is not None else None for side in sides)


class JodImagesResizedFunction(torch.autograd.Function):
    """Test and reference stacks [B, C, h, w], [B, C, h', w'] (placed: _place; the side `wrt` treats as a constant detached) -> JOD
    [B] (fp32)."""

    @staticmethod
    def forward(ctx, test, reference, metric, mode, size, fix):
        with torch.cuda.device(metric.device):
            jod, Q = forward_images(ResizedImageSetup(metric, test, reference, mode, size), fix)
        ctx.metric, ctx.mode, ctx.size, ctx.fix = metric, mode, size, fix
        ctx.save_for_backward(test, reference, Q)
        return jod

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_jod):
        test, reference, Q = ctx.saved_tensors
        grad_t = grad_r = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            with torch.cuda.device(ctx.metric.device):
                grad_t, grad_r = _backward(ctx.metric, test, reference, ctx.mode, ctx.size, ctx.fix, Q, grad_jod,
                                           ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return grad_t, grad_r, None, None, None, None


def jod_images_resized(metric, test, reference, full_screen_resize="bilinear", resize_resolution=None, dim_order="BCHW",
                       fixation_point=None, wrt="test"):
    """fvvdp.jod_images_resized (see there)."""
    name = "jod_images_resized"
    check_wrt(wrt)
    t, r, mode, size = _arguments(name, metric, test, reference, full_screen_resize, resize_resolution, dim_order, True)
    refuse_unsupported(name, metric, test, reference, wrt)
    for what, x in (("test", t), ("reference", r)):
        if x.dtype is torch.uint8 and wrt == what:
            raise RuntimeError('%s: wrt="%s" differentiates the %s, which must be float32 (float16 and bfloat16 are upcast); '
                               'it is uint8' % (name, wrt, what))
    if _same_size(t, r, size):
        return metric.jod_images(_unit_float(t), _unit_float(r), dim_order="BCHW", fixation_point=fixation_point, wrt=wrt)
    metric._check_device()
    # (half precision: torch's .float() inside autograd's view, the gradient returns through torch's cast node)
    t, r = (x.float() if x.dtype in (torch.float16, torch.bfloat16) else x for x in (t, r))
    if wrt == "test":
        r = r.detach()
    elif wrt == "reference":
        t = t.detach()
    t, r = _place(metric, t), _place(metric, r)
    return JodImagesResizedFunction.apply(t, r, metric, mode, size, _fix(metric, fixation_point, size, t.shape[0]))


def predict_images_resized(metric, test, reference, full_screen_resize="bilinear", resize_resolution=None, dim_order="BCHW",
                           fixation_point=None):
    """fvvdp.predict_images_resized (see there)."""
    name = "predict_images_resized"
    for a in (test, reference):
        if isinstance(a, torch.Tensor) and a.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("%s is forward-only and this test or reference requires grad; detach it "
                               "(differentiable: fvvdp.jod_images_resized)" % name)
    t, r, mode, size = _arguments(name, metric, test, reference, full_screen_resize, resize_resolution, dim_order, False)
    if _same_size(t, r, size):
        return metric.predict_images(t, r, dim_order="BCHW", fixation_point=fixation_point)
    metric._check_device()
    t, r = _place(metric, t), _place(metric, r)
    with torch.cuda.device(metric.device):
        s = ResizedImageSetup(metric, t, r, mode, size)
        jod, Q = forward_images(s, _fix(metric, fixation_point, size, s.B))
        stats = {"Q_per_ch": Q.permute(2, 0, 1).contiguous().cpu().numpy()[..., None], "rho_band": s.rho_band,
                 "frames_per_second": 0, "width": s.W, "height": s.H}
    return jod, stats


def predict_image_pairs_resized(metric, pairs, full_screen_resize="bilinear", resize_resolution=None, dim_order="HWC",
                                fixation_points=None):
    """fvvdp.predict_image_pairs_resized (see there)."""
    name = "predict_image_pairs_resized"
    d = dim_order.upper()
    items = []
    for test, reference in pairs:
        for a in (test, reference):
            if isinstance(a, torch.Tensor) and a.requires_grad and torch.is_grad_enabled():
                raise RuntimeError("%s is forward-only and this test or reference requires grad; detach it "
                                   "(differentiable: fvvdp.jod_images_resized)" % name)
        if "B" not in d:
            test, reference = test[None], reference[None]
        t, r, mode, size = _arguments(name, metric, test, reference, full_screen_resize, resize_resolution,
                                      d if "B" in d else "B" + d, False)
        if t.shape[0] != 1:
            raise RuntimeError("%s takes one image pair per list entry (B must be 1)" % name)
        items.append((t, r))
    if fixation_points is not None and len(fixation_points) != len(items):
        raise RuntimeError("fixation_points must hold one [x, y] (or None) per image pair")
    metric._check_device()
    groups = {}
    for i, (t, r) in enumerate(items):
        groups.setdefault((tuple(t.shape), tuple(r.shape), t.dtype, r.dtype), []).append(i)
    out = [None] * len(items)
    for idx in groups.values():
        fix = None
        if metric.foveated:
            fix = torch.cat([torch.from_numpy(metric._fixation(None if fixation_points is None else fixation_points[i], size[0],
                                                               size[1], 1)) for i in idx])
        t = torch.cat([items[i][0].to(metric.device) for i in idx])
        r = torch.cat([items[i][1].to(metric.device) for i in idx])
        q, st = predict_images_resized(metric, t, r, full_screen_resize, size, "BCHW", fix)
        for j, i in enumerate(idx):
            s = {k: v for k, v in st.items() if k not in ("Q_per_ch", "range_flags", "heatmap", "result_buffer")}
            s["N_frames"] = 1
            s["Q_per_ch"] = st["Q_per_ch"][j]
            out[i] = (q[j], s)
    return out
