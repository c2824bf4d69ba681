"""CPU oracle for the FovVideoVDP per-frame visible-difference path.

THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  It is a numpy (fp32) restatement of the reference algorithm
(gfxdisp/FovVideoVDP v1.2.3, PyTorch path) written from its behaviour; every function cites the reference
file:line it follows (paths relative to the reference root).  Only `tests/`, `__graft_entry__.smoke()` and the
`cpu_baseline` leg of `bench.py` may import it.  The product (`fovvideovdp_amd`) never does.

Parity status: PINNED.  `tools/gen_golden.py` imports the real reference in the build container and stores its
stage captures under `tests/golden/`; `tests/test_oracle_golden.py` checks this file against them (<=1e-6
relative per stage, 1e-5 on JOD) together with the README known answer 8.693 JOD (README.md:138).

All arithmetic is float32 unless stated.  `Oracle(..., dtype=np.float64)` (and the `dtype=` argument of the functions below)
runs the same expressions in float64 end to end -- display model, CSF tables, pyramid taps and all -- as a high-precision yardstick
for the GPU kernels; the float32 default is unchanged bit for bit.  Quirks of the reference that change numbers are reproduced on purpose:
  * `gausspyr_reduce` picks the right-edge fix-up of the horizontal pass by the parity of the ROW count
    (pyfvvdp/fvvdp_lpyr_dec.py:202),
  * `+1e-6` in the LUT interpolation denominator (pyfvvdp/interp.py:16),
  * `circular` temporal padding never places frame 0 in the first window (pyfvvdp/fvvdp.py:267).
"""
import json
import math
import os

import numpy as np

_F = np.float32
_DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fovvideovdp_amd", "data")


# --------------------------------------------------------------------------------------------------------
# data (calibration constants, display models, CSF LUT)
# --------------------------------------------------------------------------------------------------------
def load_defaults():
    with open(os.path.join(_DATA, "defaults.json"), "r") as f:
        return json.load(f)


def cache_key(omega, sigma, k_cm):
    """pyfvvdp/fvvdp.py:502-503"""
    return ("o%g_s%g_cm%f" % (omega, sigma, k_cm)).replace("-", "n").replace(".", "_")


def load_lut(omega, sigma, k_cm, dtype=_F):
    """pyfvvdp/fvvdp.py:505-518 (the .mat content is shipped as fovvideovdp_amd/data/csf_lut.npz)."""
    F = dtype
    z = np.load(os.path.join(_DATA, "csf_lut.npz"))
    key = cache_key(omega, sigma, k_cm)
    names = [n for n in z.files if n.startswith(key + "/")]
    if not names:
        raise RuntimeError("Error: cache file for %s not found" % key)
    return {n.split("/", 1)[1]: z[n].astype(F) for n in names}


# --------------------------------------------------------------------------------------------------------
# display photometry  (pyfvvdp/fvvdp_display_model.py)
# --------------------------------------------------------------------------------------------------------
class Photometry:
    """fvvdp_display_photo_eotf, pyfvvdp/fvvdp_display_model.py:114-176 (+ loader :52-98)."""

    dtype = _F                 # working precision of forward()

    def __init__(self, Y_peak, contrast=1000, EOTF="sRGB", gamma=2.2, E_ambient=0, k_refl=0.005, dtype=_F):
        self.Y_peak, self.contrast, self.EOTF = Y_peak, contrast, EOTF
        self.dtype = dtype
        self.gamma, self.E_ambient, self.k_refl = gamma, E_ambient, k_refl

    @classmethod
    def load(cls, display_name, models=None, dtype=_F):
        models = models if models is not None else load_defaults()["display_models.json"]
        if display_name not in models:
            raise RuntimeError('Unknown display model: "' + display_name + '"')
        m = models[display_name]
        Y_peak = m["max_luminance"]
        if "min_luminance" in m:
            contrast = Y_peak / m["min_luminance"]
        elif "contrast" in m:
            contrast = m["contrast"]
        else:
            contrast = 500
        return cls(Y_peak, contrast=contrast, EOTF=m.get("EOTF", "sRGB"), gamma=m.get("gamma", 2.2),
                   E_ambient=m.get("E_ambient", 0), k_refl=m.get("k_refl", 0.005), dtype=dtype)

    def get_black_level(self):
        """:172-176"""
        return self.E_ambient / math.pi * self.k_refl + self.Y_peak / self.contrast

    def forward(self, V):
        """:147-165.  Returns (L, out_of_range_flag)."""
        F = self.dtype
        V = np.asarray(V, dtype=F)
        oob = False
        if self.EOTF != "linear" and (np.any(V > 1) or np.any(V < 0)):
            oob = True
            V = np.clip(V, F(0.0), F(1.0))
        Yb = self.get_black_level()
        if self.EOTF == "sRGB":
            L = F(self.Y_peak - Yb) * srgb2lin(V, F) + F(Yb)
        elif self.EOTF == "gamma":
            L = F(self.Y_peak - Yb) * np.power(V, F(self.gamma)) + F(Yb)
        elif self.EOTF == "PQ":
            L = np.clip(pq2lin(V, F), F(0.005), F(self.Y_peak)) + F(Yb)
        elif self.EOTF == "linear":
            L = np.clip(V, F(0.005), F(self.Y_peak)) + F(Yb)
        else:
            raise RuntimeError("Unknown EOTF '%s'" % self.EOTF)
        return L.astype(F), oob


def srgb2lin(p, dtype=_F):
    """pyfvvdp/fvvdp_display_model.py:17-19"""
    F = dtype
    p = np.asarray(p, dtype=F)
    with np.errstate(invalid="ignore"):
        hi = np.power((p + F(0.055)) / F(1.055), F(2.4))
    return np.where(p > F(0.04045), hi, p / F(12.92)).astype(F)


def pq2lin(V, dtype=_F):
    """pyfvvdp/fvvdp_display_model.py:100-112"""
    F = dtype
    V = np.asarray(V, dtype=F)
    n, m = 0.15930175781250000, 78.843750000000000
    c1, c2, c3 = 0.83593750000000000, 18.851562500000000, 18.687500000000000
    im_t = np.power(V, F(1 / m))
    L = F(10000) * np.power(np.maximum(im_t - F(c1), F(0)) / (F(c2) - F(c3) * im_t), F(1 / n))
    return L.astype(F)


# --------------------------------------------------------------------------------------------------------
# display geometry  (pyfvvdp/fvvdp_display_model.py:383-568)
# --------------------------------------------------------------------------------------------------------
class Geometry:
    dtype = _F                 # working precision of pix2view_direction / resolution_magnification

    def __init__(self, resolution, distance_m=None, distance_display_heights=None, fov_horizontal=None,
                 fov_vertical=None, fov_diagonal=None, diagonal_size_inches=None, dtype=_F):
        """:385-436"""
        self.dtype = dtype
        self.resolution = resolution
        ar = resolution[0] / resolution[1]
        self.display_size_m = None
        if diagonal_size_inches is not None:
            height_mm = math.sqrt((diagonal_size_inches * 25.4) ** 2 / (1 + ar ** 2))
            self.display_size_m = (ar * height_mm / 1000, height_mm / 1000)
        if distance_m is not None and distance_display_heights is not None:
            raise RuntimeError("You can pass only one of: distance_m, distance_display_heights.")
        if distance_m is not None:
            self.distance_m = distance_m
        elif distance_display_heights is not None:
            if self.display_size_m is None:
                raise RuntimeError("diagonal_size_inches is needed with distance_display_heights")
            self.distance_m = distance_display_heights * self.display_size_m[1]
        elif fov_horizontal is not None or fov_vertical is not None or fov_diagonal is not None:
            self.distance_m = 3
        else:
            raise RuntimeError("Viewing distance must be specified as distance_m or distance_display_heights.")
        if (fov_horizontal is not None) + (fov_vertical is not None) + (fov_diagonal is not None) > 1:
            raise RuntimeError("You can pass only one of fov_horizontal, fov_vertical, fov_diagonal.")
        if fov_horizontal is not None:
            width_m = 2 * math.tan(math.radians(fov_horizontal / 2)) * self.distance_m
            self.display_size_m = (width_m, width_m / ar)
        elif fov_vertical is not None:
            height_m = 2 * math.tan(math.radians(fov_vertical / 2)) * self.distance_m
            self.display_size_m = (height_m * ar, height_m)
        elif fov_diagonal is not None:
            distance_px = math.sqrt(resolution[0] ** 2 + resolution[1] ** 2) / (2.0 * math.tan(math.radians(fov_diagonal * 0.5)))
            height_deg = math.degrees(math.atan(resolution[1] / 2 / distance_px)) * 2
            height_m = 2 * math.tan(math.radians(height_deg / 2)) * self.distance_m
            self.display_size_m = (height_m * ar, height_m)
        self.ppd_centre = 1 / (2 * math.degrees(math.atan(0.5 * self.display_size_m[0] / resolution[0] / self.distance_m)))

    @classmethod
    def load(cls, display_name, models=None, dtype=_F):
        """:539-568"""
        models = models if models is not None else load_defaults()["display_models.json"]
        if display_name not in models:
            raise RuntimeError("Error: Display model '%s' not found in display_models.json" % display_name)
        m = models[display_name]
        W, H = m["resolution"]
        if "viewing_distance_meters" in m:
            distance_m = m["viewing_distance_meters"]
        elif "viewing_distance_inches" in m:
            distance_m = m["viewing_distance_inches"] * 0.0254
        else:
            distance_m = None
        if "diagonal_size_meters" in m:
            diag = m["diagonal_size_meters"] / 0.0254
        else:
            diag = m.get("diagonal_size_inches")
        return cls((W, H), distance_m=distance_m, fov_diagonal=m.get("fov_diagonal"), diagonal_size_inches=diag, dtype=dtype)

    def get_ppd(self):
        return self.ppd_centre

    def pix2view_direction(self, res, x_pix, y_pix):
        """:498-510  (fp32 like the reference when fed fp32 pixel coordinates)."""
        F = self.dtype
        x_rel = np.asarray(x_pix, dtype=F) + F(-res[0] / 2)
        y_rel = np.asarray(y_pix, dtype=F) + F(-res[1] / 2)
        x_m = x_rel * F(self.display_size_m[0]) / F(res[0])
        y_m = -y_rel * F(self.display_size_m[1]) / F(res[1])
        vx = np.rad2deg(np.arctan(x_m / F(self.distance_m))).astype(F)
        vy = np.rad2deg(np.arctan(y_m / F(self.distance_m))).astype(F)
        return vx, vy

    exact_geometry = False     # checker switch, see resolution_magnification

    def resolution_magnification(self, vx, vy):
        """get_ppd(view_dir)/get_ppd()  :475-488, :512-526

        The reference evaluates [tan(a+d) - tan(a)] / tan(d) in fp32 with d = 0.0066 deg: a difference of nearly equal
        numbers that carries ~2.5e-4 relative rounding noise (ulp(tan a) / (tan(a+d) - tan a)).  `exact_geometry = True`
        (tests only) evaluates the same expression in fp64 -- the value the fp32 expression scatters around -- so that
        an implementation that does not reproduce the reference's rounding noise bit for bit can still be pinned
        tightly."""
        F = self.dtype
        if self.exact_geometry:
            va64 = np.minimum(np.sqrt(vx.astype(np.float64) ** 2 + vy.astype(np.float64) ** 2), 89.9)
            d64 = (1 / self.ppd_centre) / 2
            return ((np.tan(np.deg2rad(va64 + d64)) - np.tan(np.deg2rad(va64))) / math.tan(math.radians(d64))).astype(F)
        va = np.sqrt(vx * vx + vy * vy).astype(F)
        va = np.minimum(va, F(89.9))
        delta = (1 / self.ppd_centre) / 2
        tan_delta = math.tan(math.radians(delta))
        tan_a = np.tan(np.deg2rad(va)).astype(F)
        ppd = F(self.ppd_centre) * (np.tan(np.deg2rad(va + F(delta))).astype(F) - tan_a) / F(tan_delta)
        return (ppd / F(self.ppd_centre)).astype(F)


# --------------------------------------------------------------------------------------------------------
# frame supply  (pyfvvdp/video_source.py)
# --------------------------------------------------------------------------------------------------------
def reshuffle_dims(T, in_dims, out_dims="BCFHW"):
    """pyfvvdp/video_source.py:43-69"""
    in_dims, out_dims = in_dims.upper(), out_dims.upper()
    inter = "".join(d for d in out_dims if d in in_dims)
    perm = [in_dims.find(d) for d in inter]
    Tp = np.transpose(T, perm)
    out_sh = [Tp.shape[inter.find(d)] if d in inter else 1 for d in out_dims]
    return Tp.reshape(out_sh)


def frame_to_unit(arr_bcfhw, f, dtype=_F):
    """Integer/float unpacking of frame f -> fp32 in [0,1]  (pyfvvdp/video_source.py:184-200)."""
    F = dtype
    fr = arr_bcfhw[:, :, f:f + 1]
    if fr.dtype == np.float32:
        return fr.astype(F)
    if fr.dtype == np.uint16:          # the reference carries it as int16 and masks; same value
        return fr.astype(F) / F(65535)
    if fr.dtype == np.int16:
        return (fr.astype(np.int32) & 0xFFFF).astype(F) / F(65535)
    if fr.dtype == np.uint8:
        return fr.astype(F) / F(255)
    raise RuntimeError("Only uint8, uint16 and float32 is currently supported")


def frame_luminance(arr_bcfhw, f, photometry, rgb2y, dtype=_F):
    """_get_frame: unpack -> photometry -> luminance  (pyfvvdp/video_source.py:180-208).  Returns ([H,W], oob)."""
    F = dtype
    V = frame_to_unit(arr_bcfhw, f, F)
    L, oob = photometry.forward(V)
    if L.shape[1] == 3:
        L = L[:, 0:1] * F(rgb2y[0]) + L[:, 1:2] * F(rgb2y[1]) + L[:, 2:3] * F(rgb2y[2])
    return L[0, 0, 0].astype(F), oob


def torch_interpolate(img, out_h, out_w, mode, dtype=_F):
    """torch.nn.functional.interpolate(img[None], size=(out_h, out_w), mode=mode) for img [C,H,W] fp32 with the defaults the reference
    uses (align_corners=False, no antialiasing; pyfvvdp/video_source_file.py:240-242) -- a restatement of ATen's index arithmetic
    (aten/src/ATen/native/UpSample.h: area_pixel_compute_scale / _source_index, nearest_neighbor_compute_source_index,
    guard_index_and_lambda, get_cubic_upsample_coefficients with A = -0.75; adaptive average pooling for 'area')."""
    F = dtype
    img = np.asarray(img, dtype=F)
    C, H, W = img.shape
    sy, sx = F(H) / F(out_h), F(W) / F(out_w)
    oy, ox = np.arange(out_h, dtype=F), np.arange(out_w, dtype=F)
    if mode == "nearest":
        iy = np.minimum(np.floor(oy * sy).astype(np.int64), H - 1)
        ix = np.minimum(np.floor(ox * sx).astype(np.int64), W - 1)
        return img[:, iy][:, :, ix].astype(F)
    if mode == "bilinear":
        def axis(o, s, n):
            src = np.maximum(s * (o + F(0.5)) - F(0.5), F(0)).astype(F)
            i0 = np.minimum(src.astype(np.int64), n - 1)
            i1 = i0 + (i0 < n - 1)
            l1 = np.clip(src - i0.astype(F), 0, 1).astype(F)
            return i0, i1, (F(1) - l1).astype(F), l1
        y0, y1, ly0, ly1 = axis(oy, sy, H)
        x0, x1, lx0, lx1 = axis(ox, sx, W)
        ly0, ly1 = ly0[None, :, None], ly1[None, :, None]
        top = lx0 * img[:, y0][:, :, x0] + lx1 * img[:, y0][:, :, x1]
        bot = lx0 * img[:, y1][:, :, x0] + lx1 * img[:, y1][:, :, x1]
        return (ly0 * top + ly1 * bot).astype(F)
    if mode == "bicubic":
        A = F(-0.75)

        def coeffs(t):
            cc1 = lambda x: ((A + F(2)) * x - (A + F(3))) * x * x + F(1)
            cc2 = lambda x: ((A * x - F(5) * A) * x + F(8) * A) * x - F(4) * A
            return [cc2(t + F(1)), cc1(t), cc1(F(1) - t), cc2(F(2) - t)]

        def axis(o, s, n):
            src = (s * (o + F(0.5)) - F(0.5)).astype(F)             # cubic: the coordinate is NOT clamped, every tap index is
            fl = np.floor(src)
            idx = [np.clip(fl.astype(np.int64) - 1 + k, 0, n - 1) for k in range(4)]
            return idx, [c.astype(F) for c in coeffs((src - fl).astype(F))]
        ys, cy = axis(oy, sy, H)
        xs, cx = axis(ox, sx, W)
        out = None
        for k in range(4):                                              # x along each of the four rows, then y
            rows = img[:, ys[k]]
            row = ((rows[:, :, xs[0]] * cx[0] + rows[:, :, xs[1]] * cx[1]) + rows[:, :, xs[2]] * cx[2]) + rows[:, :, xs[3]] * cx[3]
            term = row * cy[k][None, :, None]
            out = term if out is None else out + term
        return out.astype(F)
    if mode == "area":
        def win(o, n_in, n_out):            # ATen's integers (AdaptiveAveragePooling.cpp: start_index, end_index), not a float quotient
            return (o * n_in) // n_out, 1 + ((o + 1) * n_in - 1) // n_out
        out = np.empty((C, out_h, out_w), dtype=F)
        wy = [win(o, H, out_h) for o in range(out_h)]
        wx = [win(o, W, out_w) for o in range(out_w)]
        for j, (a0, a1) in enumerate(wy):
            for i, (b0, b1) in enumerate(wx):
                out[:, j, i] = img[:, a0:a1, b0:b1].sum(axis=(1, 2), dtype=F) / F((a1 - a0) * (b1 - b0))
        return out
    raise RuntimeError("Unknown resize method '%s'" % mode)


def yuv_unpack(frame, W, H, bit_depth, chroma_ss, color_space, resize_fn=None, resize_hw=None, dtype=_F, clip=True):
    """video_reader_yuv_pytorch.unpack + _fixed2float_upscale, pyfvvdp/video_source_file.py:219-276.
    frame: 1-D uint8/uint16 (Y plane, U plane, V plane) -> RGB [H,W,3] fp32 in [0,1]; with resize_fn / resize_hw = (height, width):
    resized in RGB before the clip (:238-244).  clip=False: the RGB of :237-243 before that last clip (what a resize takes in)."""
    F = dtype
    ypx = W * H
    uvh, uvw = (H // 2, W // 2) if chroma_ss == "420" else (H, W)
    x = frame.astype(F)
    sc = 2 ** (bit_depth - 8)
    Y = np.clip(F(1 / (sc * 219)) * x[:ypx] - F(16 / 219), 0, 1).reshape(H, W).astype(F)                # :246-251
    uv = np.clip(F(1 / (sc * 224)) * x[ypx:] - F(128 / 224), F(-0.5), F(0.5)).reshape(2, uvh, uvw).astype(F)  # :253-258
    if chroma_ss == "420":                                                                             # :260-262
        # torch interpolate(scale_factor=2, mode='bilinear', align_corners=False): src = (dst+0.5)/2-0.5, clamped at 0
        def axis(n_out, n_in):
            src = np.maximum((np.arange(n_out, dtype=F) + F(0.5)) * F(0.5) - F(0.5), F(0))
            i0 = src.astype(np.int64)
            i1 = np.minimum(i0 + 1, n_in - 1)
            f = (src - i0.astype(F)).astype(F)
            return i0, i1, f
        y0, y1, fy = axis(H, uvh)
        x0, x1, fx = axis(W, uvw)
        fy, fx = fy[None, :, None], fx[None, None, :]
        top = (F(1) - fx) * uv[:, y0][:, :, x0] + fx * uv[:, y0][:, :, x1]
        bot = (F(1) - fx) * uv[:, y1][:, :, x0] + fx * uv[:, y1][:, :, x1]
        uv = ((F(1) - fy) * top + fy * bot).astype(F)
    Yuv = np.stack((Y, uv[0], uv[1]), axis=-1)
    if color_space == "bt2020nc":                                                                      # :225-235
        M = np.array([[1, 0, 1.47460], [1, -0.16455, -0.57135], [1, 1.88140, 0]], dtype=F)
    else:
        M = np.array([[1, 0, 1.402], [1, -0.344136, -0.714136], [1, 1.772, 0]], dtype=F)
    RGB = (Yuv @ M.T).astype(F)                                                                       # :237
    if resize_fn is not None and tuple(resize_hw) != (H, W):                                           # :238-243
        RGB = torch_interpolate(RGB.transpose(2, 0, 1), resize_hw[0], resize_hw[1], resize_fn, F).transpose(1, 2, 0)
    if not clip:
        return RGB
    return np.clip(RGB, 0, 1).astype(F)                                                                # :244


# --------------------------------------------------------------------------------------------------------
# temporal filters and sliding window  (pyfvvdp/fvvdp.py:228-230, 258-300, 609-630)
# --------------------------------------------------------------------------------------------------------
def filter_len(fps):
    """pyfvvdp/fvvdp.py:228"""
    return int(np.ceil(250.0 / (1000.0 / fps)))


def temporal_filters(fps, sustained_sigma=0.5, sustained_beta=0.06, fl=None, dtype=_F):
    """pyfvvdp/fvvdp.py:609-630.  Returns F[2, fl] (fp32 by default)."""
    F = dtype
    fl = filter_len(fps) if fl is None else fl
    t = np.linspace(0.0, fl / fps, fl, dtype=np.float64).astype(F)   # torch.linspace(fp32)
    # torch computes start + i*step in fp32; reproduce that rather than numpy's fp64 path
    step = F((F(fl / fps) - F(0.0)) / F(fl - 1)) if fl > 1 else F(0)
    half = fl // 2
    idx = np.arange(fl)
    t_lo = (F(0.0) + step * idx.astype(F)).astype(F)
    t_hi = (F(fl / fps) - step * (fl - 1 - idx).astype(F)).astype(F)
    t = np.where(idx < half, t_lo, t_hi).astype(F)
    taps = np.zeros((2, fl), dtype=F)
    sigma, beta = F(sustained_sigma), F(sustained_beta)
    e = -np.power(np.log(t + F(1e-4)) - np.log(beta), F(2.0)) / (F(2.0) * (sigma ** F(2.0)))
    taps[0] = np.exp(e.astype(F))
    taps[0] = taps[0] / np.sum(taps[0], dtype=F)
    k2 = 0.062170507756932
    Fdiff = taps[0, 1:] - taps[0, :-1]
    taps[1, :-1] = F(k2) * (Fdiff / (t[1] - t[0]))
    taps[1, -1] = 0
    return taps


def window_frame_indices(N, fl, temp_padding):
    """Source-frame index for every slot of the sliding window.

    Returns idx[N, fl]: idx[ff, k] is the source frame in slot k (oldest first) of the window used for output
    frame ff (pyfvvdp/fvvdp.py:258-291).  Slot fl-1 is the newest frame and is weighted by F[cc][0] (:298).
    """
    if temp_padding == "replicate":
        first = [0] * fl                                                    # :259-262
    elif temp_padding == "circular":
        first = [(N - 1 - fl + kk) % N for kk in range(fl)]                # :263-269 (quirk: frame 0 absent)
    elif temp_padding == "pingpong":
        pingpong = list(range(0, N)) + list(range(N - 2, 0, -1))           # :274-278
        indices = []
        while len(indices) < (fl - 1):
            indices = indices + pingpong
        first = (indices[-(fl - 1):] if fl > 1 else []) + [0]
    else:
        raise RuntimeError('Unknown padding method "{}"'.format(temp_padding))
    idx = np.zeros((N, fl), dtype=np.int64)
    win = list(first)
    idx[0] = win
    for ff in range(1, N):
        win = win[1:] + [ff]                                                # :290-291
        idx[ff] = win
    return idx


def temporal_channels(win_T, win_R, taps, dtype=_F):
    """R[2cc+s] = sum_k win[s][k] * taps[cc][fl-1-k]   (pyfvvdp/fvvdp.py:294-300).  win_*: [fl,H,W] oldest first."""
    F = dtype
    H, W = win_T.shape[-2:]
    R = np.zeros((4, H, W), dtype=F)
    for cc in range(2):
        corr = taps[cc][::-1].reshape(-1, 1, 1).astype(F)
        R[2 * cc + 0] = np.sum(win_T * corr, axis=0, dtype=F)
        R[2 * cc + 1] = np.sum(win_R * corr, axis=0, dtype=F)
    return R


# --------------------------------------------------------------------------------------------------------
# pyramid  (pyfvvdp/fvvdp_lpyr_dec.py)
# --------------------------------------------------------------------------------------------------------
def band_frequencies(W, H, ppd):
    """fvvdp_lpyr_dec.__init__  pyfvvdp/fvvdp_lpyr_dec.py:15-49.  Returns (height, band_freqs[height+1])."""
    max_levels = int(np.floor(np.log2(min(H, W)))) - 1
    bands = np.concatenate([[1.0], np.power(2.0, -np.arange(0.0, 14.0)) * 0.3228], 0) * ppd / 2.0
    invalid = np.nonzero(bands <= 0.5)[0]
    max_band = max_levels if invalid.size == 0 else int(invalid[0])
    height = int(np.clip(max_band + 1, 0, max_levels))
    freqs = np.array([1.0] + [0.3228 * 2.0 ** (-f) for f in range(height)]) * ppd / 2.0
    return height, freqs


_K = np.array([0.25 - 0.4 / 2.0, 0.25, 0.4, 0.25, 0.25 - 0.4 / 2.0]).astype(_F)   # :176 built in fp32 by torch.tensor


def _k(dtype=_F):
    # torch.tensor([...python floats...], dtype=float32): each entry rounded from fp64 (kept exact in float64 mode)
    F = dtype
    return np.array([0.25 - 0.4 / 2.0, 0.25, 0.4, 0.25, 0.25 - 0.4 / 2.0], dtype=np.float64).astype(F)


def gausspyr_reduce(x, dtype=_F):
    """pyfvvdp/fvvdp_lpyr_dec.py:183-207.  x: [P,H,W] fp32 -> [P,ceil(H/2),ceil(W/2)]."""
    F = dtype
    K = _k(F)
    P, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    # vertical: zero-padded 5-tap, stride 2  (:188)
    xp = np.zeros((P, H + 4 + 1, W), dtype=F)
    xp[:, 2:2 + H] = x
    ya = np.zeros((P, Ho, W), dtype=F)
    for k in range(5):
        ya += K[k] * xp[:, k:k + 2 * Ho:2]
    ya[:, 0] += x[:, 0] * K[1] + x[:, 1] * K[0]                     # :191
    if H % 2 == 1:                                                    # :192-195
        ya[:, -1] += x[:, -1] * K[3] + x[:, -2] * K[4]
    else:
        ya[:, -1] += x[:, -1] * K[4]
    # horizontal on the result (:198)
    yp = np.zeros((P, Ho, W + 4 + 1), dtype=F)
    yp[:, :, 2:2 + W] = ya
    y = np.zeros((P, Ho, Wo), dtype=F)
    for k in range(5):
        y += K[k] * yp[:, :, k:k + 2 * Wo:2]
    y[:, :, 0] += ya[:, :, 0] * K[1] + ya[:, :, 1] * K[0]           # :201
    if H % 2 == 1:       # QUIRK (:202): parity of the ROW count of x selects the column fix-up
        y[:, :, -1] += ya[:, :, -1] * K[3] + ya[:, :, -2] * K[4]
    else:
        y[:, :, -1] += ya[:, :, -1] * K[4]
    return y


def _expand_axis(x, n_out, axis, dtype=_F):
    """One axis of gausspyr_expand: zero-stuff, edge pad, valid conv with 2K (:126-142, :225-233).

    Closed form: even i -> 2K0*x[c-1] + 2K2*x[c] + 2K4*x[c+1] (c=i/2), odd i -> 2K1*x[(i-1)/2] + 2K3*x[(i+1)/2],
    neighbour indices clamped to the valid range.
    """
    F = dtype
    K2 = (_k(F) * F(2)).astype(F)
    x = np.moveaxis(x, axis, -1)
    n = x.shape[-1]
    i = np.arange(n_out)
    c = i // 2
    cm, cp = np.clip(c - 1, 0, n - 1), np.clip(c + 1, 0, n - 1)
    c0 = np.clip(c, 0, n - 1)
    even = (K2[0] * x[..., cm] + K2[2] * x[..., c0]) + K2[4] * x[..., cp]
    odd = K2[1] * x[..., c0] + K2[3] * x[..., cp]
    out = np.where((i % 2) == 0, even, odd).astype(F)
    return np.moveaxis(out, -1, axis)


def gausspyr_expand(x, sz, dtype=_F):
    """pyfvvdp/fvvdp_lpyr_dec.py:219-235: vertical first, then horizontal."""
    F = dtype
    return _expand_axis(_expand_axis(x, sz[0], -2, F), sz[1], -1, F)


def gaussian_pyramid(image, levels, dtype=_F):
    """pyfvvdp/fvvdp_lpyr_dec.py:144-158"""
    F = dtype
    res = [image]
    for _ in range(1, levels):
        res.append(gausspyr_reduce(res[-1], F))
    return res


def contrast_pyr_decompose(image, height, dtype=_F):
    """fvvdp_contrast_pyr.decompose  pyfvvdp/fvvdp_lpyr_dec.py:248-273.  image: [P,H,W].

    Returns (contrast bands (list of [P,h,w], base band last), L_bkg bands (list of [h,w])).
    """
    F = dtype
    gpyr = gaussian_pyramid(image, height + 1, F)
    lpyr, lbkg = [], []
    for i in range(len(gpyr) - 1):
        ex = gausspyr_expand(gpyr[i + 1], gpyr[i].shape[-2:], F)
        layer = gpyr[i] - ex
        L_bkg = np.maximum(ex[1], F(0.1))                                   # :265 plane 1 = reference(-sustained)
        contrast = np.minimum(layer / L_bkg[None], F(1000.0))               # :266
        lpyr.append(contrast.astype(F))
        lbkg.append(L_bkg.astype(F))
    lpyr.append(gpyr[-1])
    return lpyr, lbkg


# --------------------------------------------------------------------------------------------------------
# CSF LUT interpolation  (pyfvvdp/interp.py, pyfvvdp/fvvdp.py:520-537)
# --------------------------------------------------------------------------------------------------------
def get_interpolants_v1(x_q, x, dtype=_F):
    """pyfvvdp/interp.py:11-20"""
    F = dtype
    imax = np.searchsorted(x, x_q, side="left")          # torch.bucketize(right=False): first x[i] >= q
    imax = np.minimum(imax, x.shape[0] - 1)
    imin = np.clip(imax - 1, 0, x.shape[0] - 1)
    ifrc = (x_q - x[imin]) / (x[imax] - x[imin] + F(0.000001))
    ifrc = np.where(imax == imin, F(0), ifrc)
    ifrc = np.where(ifrc < 0, F(0), ifrc).astype(F)
    return imin, imax, ifrc


def interp3(x, y, z, v, x_q, y_q, z_q, dtype=_F):
    """pyfvvdp/interp.py:43-59  (v indexed [y, x, z])."""
    F = dtype
    shp = x_q.shape
    x_q, y_q, z_q = x_q.ravel(), y_q.ravel(), z_q.ravel()
    imin, imax, ifrc = get_interpolants_v1(x_q, x, F)
    jmin, jmax, jfrc = get_interpolants_v1(y_q, y, F)
    kmin, kmax, kfrc = get_interpolants_v1(z_q, z, F)
    one = F(1.0)
    filtered = (
        ((v[jmin, imin, kmin] * (one - ifrc) + v[jmin, imax, kmin] * ifrc) * (one - jfrc) +
         (v[jmax, imin, kmin] * (one - ifrc) + v[jmax, imax, kmin] * ifrc) * jfrc) * (one - kfrc) +
        ((v[jmin, imin, kmax] * (one - ifrc) + v[jmin, imax, kmax] * ifrc) * (one - jfrc) +
         (v[jmax, imin, kmax] * (one - ifrc) + v[jmax, imax, kmax] * ifrc) * jfrc) * kfrc)
    return filtered.reshape(shp).astype(F)


def cached_sensitivity(lut, rho, L_bkg, ecc, dtype=_F):
    """pyfvvdp/fvvdp.py:520-537.  rho, L_bkg, ecc broadcastable fp32 arrays -> S."""
    F = dtype
    rho, L_bkg, ecc = np.broadcast_arrays(np.asarray(rho, F), np.asarray(L_bkg, F), np.asarray(ecc, F))
    rho_q = np.log2(np.clip(rho, lut["rho"][0], lut["rho"][-1])).astype(F)
    Y_q = np.log2(np.clip(L_bkg, lut["Y"][0], lut["Y"][-1])).astype(F)
    ecc_q = np.sqrt(np.clip(ecc, lut["ecc"][0], lut["ecc"][-1])).astype(F)
    interpolated = interp3(lut["rho_log"], lut["Y_log"], lut["ecc_sqrt"], lut["S_log"], rho_q, Y_q, ecc_q, F)
    return np.power(F(2.0), interpolated).astype(F)


# --------------------------------------------------------------------------------------------------------
# masking, pooling, JOD  (pyfvvdp/fvvdp.py:337-357, 574-607)
# --------------------------------------------------------------------------------------------------------
def apply_masking_model(T, R, N, cc, prm, dtype=_F):
    """pyfvvdp/fvvdp.py:574-596 with phase_uncertainty :550-556 (pu_dilate=0) and mask_func_perc_norm2 :569-572."""
    F = dtype
    p = F(prm["mask_p"])
    q = F(prm["mask_q_sust"] if cc == 0 else prm["mask_q_trans"])
    T = T / N
    R = R / N
    k = np.power(F(10.0), F(prm["mask_c"]))
    M = np.minimum(np.abs(T), np.abs(R)) * k
    D = np.power(np.abs(T - R), p) / (F(1.0) + np.power(M, q))
    return np.minimum(D, F(1e4)).astype(F)


def lp_norm(x, p, axis=0, normalize=True, dtype=_F):
    """pyfvvdp/fvvdp.py:598-607 (torch.norm accumulates wider than fp32 on CPU; fp64 here)."""
    F = dtype
    N = x.shape[axis] if normalize else 1.0
    s = np.sum(np.power(np.abs(x.astype(np.float64)), p), axis=axis, keepdims=True)
    return (np.power(s, 1.0 / p) / (float(N) ** (1.0 / p))).astype(F)


def do_pooling_and_jods(Q_per_ch, prm, dtype=_F):
    """pyfvvdp/fvvdp.py:337-357.  Q_per_ch: [height, 2, N]."""
    F = dtype
    if Q_per_ch.shape[1] == 2:
        w = np.array([1.0, prm["w_transient"]], dtype=F).reshape(1, 2, 1)
    else:
        w = F(1)
    Q_sc = lp_norm(Q_per_ch * w, prm["beta_sch"], 0, False, F)
    Q_tc = lp_norm(Q_sc, prm["beta_tch"], 1, False, F)
    Q = float(lp_norm(Q_tc, prm["beta_t"], 2, True, F).squeeze())
    beta_jod = 10.0 ** prm["log_jod_exp"]
    a = prm["jod_a"]
    sign = -1 if a < 0 else 1
    return F(sign * ((abs(a) ** (1.0 / beta_jod)) * F(Q)) ** beta_jod + 10.0)


# --------------------------------------------------------------------------------------------------------
# per-frame core and the frame loop  (pyfvvdp/fvvdp.py:190-334, 359-478)
# --------------------------------------------------------------------------------------------------------
# --------------------------------------------------------------------------------------------------------
# PU21-PSNR side metric  (pyfvvdp/pupsnr.py:52-79, pyfvvdp/utils.py:157-202)
# --------------------------------------------------------------------------------------------------------
PU21_BANDING_GLARE = (234.0235618, 216.9339286, 0.0001091864237, 0.893206924, 0.06733984121, 1.444718567, 567.6315065)
PU21_L_MIN, PU21_L_MAX = 0.005, 10000.0


def pu21_peak(p=PU21_BANDING_GLARE, L_max=PU21_L_MAX):
    """utils.py:181 (python floats = fp64, like the reference)"""
    return p[6] * (((p[0] + p[1] * L_max ** p[3]) / (1 + p[2] * L_max ** p[3])) ** p[4] - p[5])


def pu21_encode(Y, p=PU21_BANDING_GLARE):
    """PU.encode, utils.py:183-193: clip to [0.005, 10000], rational power function; fp32 like torch."""
    Y = np.clip(Y.astype(_F), _F(PU21_L_MIN), _F(PU21_L_MAX))
    Yp = np.power(Y, _F(p[3]))
    return (_F(p[6]) * (np.power((_F(p[0]) + _F(p[1]) * Yp) / (_F(1) + _F(p[2]) * Yp), _F(p[4])) - _F(p[5]))).astype(_F)


def pu_psnr(test, ref, dim_order="BCFHW", display_name="standard_4k", photometry=None, color_space="sRGB"):
    """pu_psnr.predict_video_source, pupsnr.py:52-79: per frame 20*log10(peak / sqrt(mean((PU(T)-PU(R))^2))),
    averaged over the frames (fp32 per frame like torch, accumulated in python float)."""
    test = reshuffle_dims(np.asarray(test), dim_order)
    ref = reshuffle_dims(np.asarray(ref), dim_order)
    phot = photometry if photometry is not None else Photometry.load(display_name)
    rgb2y = load_defaults()["color_spaces.json"][color_space]["RGB2Y"]
    N = test.shape[2]
    peak = pu21_peak()
    acc = 0.0
    for f in range(N):
        T, _ = frame_luminance(test, f, phot, rgb2y)
        R, _ = frame_luminance(ref, f, phot, rgb2y)
        d = pu21_encode(T) - pu21_encode(R)
        mse = np.mean((d * d).astype(_F), dtype=_F)
        acc = acc + float(_F(20.0) * np.log10(_F(peak) / np.sqrt(mse))) / N
    return acc


class Oracle:
    """Mirror of `class fvvdp` restricted to the live branch (local_adapt=gpyr, contrast=weber, pu_dilate=0)."""

    def __init__(self, display_name="standard_4k", photometry=None, geometry=None, color_space="sRGB",
                 foveated=False, temp_padding="replicate", heatmap=None, dtype=_F):
        if heatmap not in (None, "raw"):
            raise RuntimeError("the oracle restates the 'raw' difference map only (the colouring is a function of it and the context frame)")
        self.heatmap = heatmap
        self.dtype = dtype             # working precision: np.float32 (the reference's) or np.float64 (a high-precision yardstick)
        d = load_defaults()
        self.prm = d["fvvdp_parameters.json"]
        self.photometry = photometry if photometry is not None else Photometry.load(display_name, d["display_models.json"], dtype)
        self.geometry = geometry if geometry is not None else Geometry.load(display_name, d["display_models.json"], dtype)
        if color_space not in d["color_spaces.json"]:
            raise RuntimeError('Unknown color space: "' + color_space + '"')
        self.rgb2y = d["color_spaces.json"][color_space]["RGB2Y"]
        self.foveated = foveated
        self.temp_padding = temp_padding
        self.ppd = self.geometry.get_ppd()
        self.lut = [load_lut(om, self.prm["csf_sigma"], self.prm["k_cm"], dtype) for om in (0, 5)]
        self.capture = None            # optional dict of lists filled with stage outputs

    # -- foveated maps, pyfvvdp/fvvdp.py:416-437 ----------------------------------------------------------
    def _fov_maps(self, w_band, h_band, w_frame, h_frame, fix):
        F = self.dtype
        xv = np.linspace(0.5, w_band - 0.5, w_band).astype(F)
        yv = np.linspace(0.5, h_band - 0.5, h_band).astype(F)
        xx, yy = np.meshgrid(xv, yv, indexing="xy")
        vx, vy = self.geometry.pix2view_direction((w_band, h_band), xx, yy)
        gx, gy = self.geometry.pix2view_direction((w_frame, h_frame), F(fix[0]) + F(0.5), F(fix[1]) + F(0.5))
        ecc = np.sqrt((vx - gx) ** 2 + (vy - gy) ** 2).astype(F)
        res_mag = self.geometry.resolution_magnification(vx, vy)
        return ecc, res_mag

    def process_frame(self, ff, R, height, rho_band, temp_ch, fixation, frame_size):
        """process_block_of_frames, pyfvvdp/fvvdp.py:359-478.  R: [P,H,W].  Returns Q[height,2]."""
        prm, F = self.prm, self.dtype
        bands, lbkg = contrast_pyr_decompose(R, height, F)
        Q = np.zeros((height, 2), dtype=F)
        dmap_bands = [None] * height
        sens = F(10.0 ** (prm["sensitivity_correction"] / 20.0))
        for cc in range(temp_ch):
            for bb in range(height):
                m = F(1.0 if bb == 0 else 2.0)                       # get_band, fvvdp_lpyr_dec.py:57-63
                T_f = bands[bb][2 * cc + 0] * m
                R_f = bands[bb][2 * cc + 1] * m
                L_bkg = lbkg[bb]
                h, w = T_f.shape
                if self.foveated:
                    fix = fixation[ff] if np.ndim(fixation) == 2 else fixation
                    ecc, res_mag = self._fov_maps(w, h, frame_size[1], frame_size[0], fix)
                else:
                    res_mag = np.ones((h, w), dtype=F)
                    ecc = np.zeros((h, w), dtype=F)
                rho = (F(rho_band[bb]) * res_mag).astype(F)         # fvvdp.py:442 (numpy fp64 scalar * fp32 tensor -> fp32)
                S_raw = cached_sensitivity(self.lut[cc], rho, L_bkg, ecc, F)
                S = S_raw * sens                                      # fvvdp.py:447
                N_nCSF = (F(1.0) / S).astype(F)                     # fvvdp.py:451
                D = apply_masking_model(T_f, R_f, N_nCSF, cc, prm, F)
                if self.capture is not None:
                    self.capture.setdefault("S", []).append(S_raw)
                    self.capture.setdefault("D", []).append(D)
                Q[bb, cc] = lp_norm(D.ravel(), prm["beta"], 0, True, F)[0]
                if self.heatmap is not None:                          # fvvdp.py:458-462 with set_band / get_band, fvvdp_lpyr_dec.py:57-71
                    if cc == 0:
                        dmap_bands[bb] = (D / m).astype(F)
                    else:
                        dmap_bands[bb] = ((dmap_bands[bb] * m + F([1.0, prm["w_transient"]][cc]) * D) / m).astype(F)
        if self.heatmap is not None:
            # heatmap_pyr.reconstruct (fvvdp_lpyr_dec.py:96-103) from the base band of a decomposed zero image, then fvvdp.py:468-470
            img = np.zeros_like(bands[height][0])
            for i in reversed(range(height)):
                img = (gausspyr_expand(img, dmap_bands[i].shape, F) + dmap_bands[i]).astype(F)
            beta_jod = np.float64(10.0) ** prm["log_jod_exp"]
            self.last_dmap = (np.power(img, F(beta_jod)) * F(abs(prm["jod_a"]))).astype(F).astype(np.float16)
        if self.capture is not None:
            self.capture.setdefault("bands", []).append(bands)
            self.capture.setdefault("L_bkg", []).append(lbkg)
            self.capture.setdefault("R", []).append(R)
        return Q

    def predict_yuv(self, test_yuv, ref_yuv, frames_per_second, W, H, bit_depth=8, chroma_ss="420", color_space="bt709",
                    fixation_point=None, frames=None, full_screen_resize=None, resize_resolution=None):
        """Raw planar YUV frames [N, frame_elems] through unpack -> photometry -> luminance
        (fvvdp_video_source_video_file._prepare_frame, pyfvvdp/video_source_file.py:355-363), then the usual path.
        full_screen_resize / resize_resolution = (width, height): the CLI's --full-screen-resize (run_fvvdp.py:84, :209-210)."""
        rhw = None if full_screen_resize is None else (int(resize_resolution[1]), int(resize_resolution[0]))

        def to_rgb(arr):
            vid = np.stack([yuv_unpack(arr[f], W, H, bit_depth, chroma_ss, color_space, full_screen_resize, rhw, self.dtype)
                            for f in range(arr.shape[0])], 0)
            return np.ascontiguousarray(vid.transpose(3, 0, 1, 2)[None])           # [1,3,N,H,W] fp32
        return self.predict(to_rgb(np.asarray(test_yuv)), to_rgb(np.asarray(ref_yuv)), "BCFHW", frames_per_second,
                            fixation_point, frames)

    def predict(self, test, ref, dim_order="BCFHW", frames_per_second=0, fixation_point=None, frames=None):
        """fvvdp.predict / predict_video_source, pyfvvdp/fvvdp.py:181-334.

        `frames` (optional iterable) restricts the OUTPUT frames that are evaluated (used for bounded CPU
        timing); pooling then runs over those frames only.
        """
        F = self.dtype
        test = reshuffle_dims(np.asarray(test), dim_order)
        ref = reshuffle_dims(np.asarray(ref), dim_order)
        if test.shape != ref.shape:
            raise RuntimeError("Test and reference image/video tensors must be exactly the same shape")
        B, C, N, H, W = test.shape
        if frames_per_second == 0 and N > 1:
            raise RuntimeError("When passing video sequences, you must set frames_per_second parameter")
        if C not in (1, 3):
            raise RuntimeError("The content must have either 1 or 3 colour channels.")
        height, rho_band = band_frequencies(W, H, self.ppd)
        if fixation_point is None:
            fixation_point = np.array([W // 2, H // 2])
        fixation_point = np.asarray(fixation_point)
        is_image = N == 1
        oob = False
        lum_cache = {}

        def lum(arr, tag, f):
            nonlocal oob
            if (tag, f) not in lum_cache:
                L, o = frame_luminance(arr, f, self.photometry, self.rgb2y, F)
                oob = oob or o
                lum_cache[(tag, f)] = L
            return lum_cache[(tag, f)]

        out_frames = list(range(N)) if frames is None else list(frames)
        Q_per_ch = np.zeros((height, 2, len(out_frames)), dtype=F)
        heat = np.zeros((1, 1, len(out_frames), H, W), dtype=np.float16) if self.heatmap is not None else None
        if is_image:
            temp_ch = 1
        else:
            temp_ch = 2
            fl = filter_len(frames_per_second)
            taps = temporal_filters(frames_per_second, self.prm["sustained_sigma"], self.prm["sustained_beta"], fl, F)
            widx = window_frame_indices(N, fl, self.temp_padding)
            self.F = taps
        for oi, ff in enumerate(out_frames):
            if is_image:
                R = np.stack([lum(test, "t", 0), lum(ref, "r", 0)], 0)
            else:
                win_T = np.stack([lum(test, "t", int(j)) for j in widx[ff]], 0)
                win_R = np.stack([lum(ref, "r", int(j)) for j in widx[ff]], 0)
                R = temporal_channels(win_T, win_R, taps, F)
                keep = set(int(j) for j in widx[min(ff + 1, N - 1)])
                for key in [k for k in lum_cache if k[1] not in keep]:
                    del lum_cache[key]
            Q_per_ch[:, :, oi] = self.process_frame(ff, R, height, rho_band, temp_ch, fixation_point, (H, W))
            if heat is not None:
                heat[0, 0, oi] = self.last_dmap
        jod = do_pooling_and_jods(Q_per_ch, self.prm, F)
        stats = {"Q_per_ch": Q_per_ch, "rho_band": rho_band, "frames_per_second": frames_per_second,
                 "width": W, "height": H, "N_frames": N, "oob": oob}
        if heat is not None:
            stats["heatmap"] = heat                                  # fp16 [1,1,frames,H,W] like the reference's 'raw' mode (fvvdp.py:216-221, 471-472)
        return jod, stats
