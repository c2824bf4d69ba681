"""ctypes binding of libfvvdp_hip.so (include/fvvdp_hip.h).  No fallback: if the library is missing or does not
load, every entry point raises -- the product never computes the hot path on the CPU."""
import ctypes as C
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("FVVDP_LIB", os.path.join(_HERE, "libfvvdp_hip.so"))   # override: A/B builds
BUILD_FLAGS_NOTE = "hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -mllvm -pragma-unroll-threshold=1000000"
SRC_PATH = os.path.join(_HERE, "csrc", "fvvdp_hip.hip")
INCLUDE_DIR = os.path.join(ROOT, "include")

FVVDP_U8, FVVDP_U16, FVVDP_F32, FVVDP_F16, FVVDP_BF16 = 0, 1, 2, 3, 4
FVVDP_EUNSUPPORTED = -5
EOTF_LUT, EOTF_SRGB, EOTF_GAMMA, EOTF_PQ, EOTF_LINEAR, EOTF_ABSOLUTE, EOTF_NONE = range(7)
PSNR_SLICES = 256            # FVVDP_PSNR_SLICES
MAX_BANDS = 16
MAX_TAPS = 256
LUT_N = 32
RESIZE_MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2, "area": 3}      # FVVDP_RESIZE_*


class Params(C.Structure):
    _fields_ = [("mask_p", C.c_float), ("mask_q", C.c_float * 2), ("mask_k", C.c_float), ("beta", C.c_float),
                ("sens_gain", C.c_float), ("lbkg_min", C.c_float), ("contrast_max", C.c_float), ("d_max", C.c_float)]


class Eotf(C.Structure):
    _fields_ = [("kind", C.c_int32), ("Y_peak", C.c_float), ("Y_black", C.c_float), ("gamma", C.c_float),
                ("L_min", C.c_float), ("L_max", C.c_float), ("d_lut", C.c_void_p)]


class YuvFormat(C.Structure):
    _fields_ = [("bit_depth", C.c_int32), ("chroma_420", C.c_int32), ("ycbcr2rgb", C.c_float * 9)]


class YuvPlanes(C.Structure):
    """fvvdp_yuv_planes (include/fvvdp_hip_yuv_grad.h): one stream of float32 planes, strides in elements."""
    _fields_ = [("d_y", C.c_void_p), ("d_u", C.c_void_p), ("d_v", C.c_void_p), ("luma_stride", C.c_size_t),
                ("chroma_stride", C.c_size_t)]


class ResizeStream(C.Structure):
    """fvvdp_resize_stream (include/fvvdp_hip_resize.h): one stream at its own frame size, strides in elements."""
    _fields_ = [("d_data", C.c_void_p), ("dtype", C.c_int32), ("channels", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("frame_stride", C.c_size_t), ("plane_stride", C.c_size_t)]


class Geom(C.Structure):
    _fields_ = [("display_size_m", C.c_float * 2), ("distance_m", C.c_float), ("ppd_centre", C.c_float)]


class PoolParams(C.Structure):
    _fields_ = [("beta_sch", C.c_float), ("beta_tch", C.c_float), ("beta_t", C.c_float), ("w_transient", C.c_float),
                ("jod_a", C.c_float), ("beta_jod", C.c_float)]


class Pu21(C.Structure):
    _fields_ = [("p", C.c_float * 7), ("L_min", C.c_float), ("L_max", C.c_float)]


class BandMaps(C.Structure):
    _fields_ = [("d_D", C.c_void_p), ("d_contrast", C.c_void_p), ("d_lbkg", C.c_void_p), ("d_S", C.c_void_p)]


# every symbol declared in include/fvvdp_hip.h: name -> (restype, argtypes)
SYMBOLS = {
    "fvvdp_ctx_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.POINTER(C.c_double), C.POINTER(Params)]),
    "fvvdp_ctx_destroy": (None, [C.c_void_p]),
    "fvvdp_last_error": (C.c_char_p, []),
    "fvvdp_ctx_level_size": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fvvdp_ctx_scratch_bytes": (C.c_size_t, [C.c_void_p]),
    "fvvdp_ctx_set_csf_1d": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "fvvdp_ctx_set_csf_3d": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                       C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "fvvdp_ctx_set_view_maps": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float]),
    "fvvdp_temporal_channels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t,
                                          C.POINTER(Eotf), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fvvdp_temporal_channels_frames": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int,
                                                 C.c_size_t, C.POINTER(Eotf), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                                 C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fvvdp_temporal_channels_yuv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(YuvFormat), C.c_size_t,
                                              C.POINTER(Eotf), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                              C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fvvdp_load_channels_planar": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "fvvdp_bands_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float),
                                      C.POINTER(Geom), C.POINTER(BandMaps), C.c_void_p]),
    "fvvdp_bands_forward_pool": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float),
                                           C.POINTER(Geom), C.POINTER(BandMaps), C.POINTER(PoolParams), C.c_void_p, C.c_void_p]),
    "fvvdp_heatmap_reconstruct": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_float, C.c_float, C.c_float,
                                            C.c_void_p, C.c_void_p]),
    "fvvdp_export_level": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fvvdp_pool_jod": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PoolParams), C.c_void_p, C.c_void_p]),
    "fvvdp_heatmap_colorize": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int,
                                         C.POINTER(C.c_float), C.c_void_p, C.c_size_t, C.c_void_p]),
    "fvvdp_pu21_sse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t,
                                 C.POINTER(Eotf), C.POINTER(C.c_float), C.POINTER(Pu21), C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "fvvdp_yuv_frame_resized": (C.c_int, [C.c_void_p, C.POINTER(YuvFormat), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(Eotf), C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]),
    "fvvdp_ctx_timing_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "fvvdp_ctx_timing_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int, C.c_int]),
    "fvvdp_ctx_alloc_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int,
                                      C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fvvdp_ctx_call_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
}

# include/fvvdp_hip_images.h: batched still images (bound by lib() as well; SYMBOLS stays the ABI of fvvdp_hip.h)
IMAGE_SYMBOLS = {
    "fvvdp_images_channels": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int,
                                        C.c_size_t, C.POINTER(Eotf), C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p]),
    "fvvdp_images_forward_pool": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float),
                                            C.POINTER(Geom), C.POINTER(BandMaps), C.POINTER(PoolParams), C.c_void_p, C.c_void_p]),
    "fvvdp_pool_jod_columns": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PoolParams), C.c_void_p,
                                         C.c_void_p]),
}
IMAGES_MAX_PAIRS_PER_LAUNCH = 128        # FVVDP_IMAGES_MAX_PAIRS_PER_LAUNCH

# include/fvvdp_hip_grad.h: gradients of the still-image JOD with respect to the test images (bound by lib() as well)
GRAD_SYMBOLS = {
    "fvvdp_images_grad_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "fvvdp_images_grad": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(PoolParams), C.c_void_p,
                                    C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_size_t,
                                    C.POINTER(Eotf), C.POINTER(C.c_float), C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t,
                                    C.c_void_p]),
}

# include/fvvdp_hip_video_grad.h: gradients of the video JOD with respect to the test clip (bound by lib() as well)
VIDEO_GRAD_SYMBOLS = {
    "fvvdp_video_grad_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "fvvdp_video_grad_frames": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(PoolParams), C.c_void_p,
                                          C.c_int, C.c_int, C.c_void_p, C.POINTER(BandMaps), C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_void_p]),
    "fvvdp_video_grad_input": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t,
                                         C.POINTER(Eotf), C.POINTER(C.c_float), C.c_void_p, C.c_size_t, C.c_void_p]),
}
VIDEO_GRAD_MAX_TAPS = 64                 # FVVDP_VIDEO_GRAD_MAX_TAPS

# include/fvvdp_hip_gaze.h: one clip under many gaze traces (bound by lib() as well)
GAZE_SYMBOLS = {
    "fvvdp_gaze_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "fvvdp_bands_forward_gazes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int,
                                            C.POINTER(Geom), C.c_void_p, C.c_size_t, C.c_void_p]),
    "fvvdp_bands_forward_gazes_pool": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int,
                                                 C.c_int, C.POINTER(Geom), C.c_void_p, C.c_size_t, C.POINTER(PoolParams),
                                                 C.c_void_p, C.c_void_p]),
}
GAZE_GROUP_MAX = 8                       # FVVDP_GAZE_GROUP_MAX

# include/fvvdp_hip_tests.h: many test clips against one reference (bound by lib() as well)
MULTITEST_SYMBOLS = {
    "fvvdp_tests_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "fvvdp_bands_forward_tests": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                            C.c_void_p]),
    "fvvdp_bands_forward_tests_pool": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                 C.c_size_t, C.POINTER(PoolParams), C.c_void_p, C.c_void_p]),
}
TESTS_GROUP_MAX = 3                      # FVVDP_TESTS_GROUP_MAX

# include/fvvdp_hip_tests_fov.h: many test clips against one reference under a gaze (bound by lib() as well)
TESTS_FOV_SYMBOLS = {
    "fvvdp_tests_fov_covered": (C.c_int, [C.c_void_p, C.POINTER(Geom), C.POINTER(C.c_int), C.c_void_p]),
    "fvvdp_bands_forward_tests_fov": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float),
                                                C.POINTER(Geom), C.c_void_p, C.c_size_t, C.c_void_p]),
    "fvvdp_bands_forward_tests_fov_pool": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float),
                                                     C.POINTER(Geom), C.c_void_p, C.c_size_t, C.POINTER(PoolParams), C.c_void_p,
                                                     C.c_void_p]),
}

# include/fvvdp_hip_gaze_grad.h: gradients of the video JOD under many gaze traces (bound by lib() as well)
GAZE_GRAD_SYMBOLS = {
    "fvvdp_gaze_grad_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "fvvdp_gaze_grad_frames": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(PoolParams),
                                         C.POINTER(Geom), C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_float), C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                         C.POINTER(BandMaps), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}

# include/fvvdp_hip_ref_grad.h: gradients of the image and video JOD with respect to the reference (bound by lib() as well)
REF_GRAD_SYMBOLS = {
    "fvvdp_ctx_set_slope_maps": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "fvvdp_ref_grad_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "fvvdp_images_ref_grad": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(PoolParams), C.c_void_p,
                                        C.c_int, C.c_int, C.c_void_p, C.POINTER(BandMaps), C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p), C.c_int, C.c_size_t, C.POINTER(Eotf), C.POINTER(C.c_float),
                                        C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p]),
    "fvvdp_video_ref_grad_frames": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(PoolParams),
                                              C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(BandMaps), C.POINTER(C.c_void_p),
                                              C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}

# include/fvvdp_hip_params.h: the model parameters of a live context and the sums their gradients need (bound by lib() as well)
PARAM_SYMBOLS = {
    "fvvdp_ctx_set_params": (C.c_int, [C.c_void_p, C.POINTER(Params)]),
    "fvvdp_param_sums_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "fvvdp_param_sums": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(BandMaps), C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
}
PARAM_SUMS = 5                           # FVVDP_PARAM_SUMS

# include/fvvdp_hip_taps.h: the gradient with respect to the taps of the temporal filters (bound by lib() as well)
TAP_SYMBOLS = {
    "fvvdp_luminance_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t,
                                         C.POINTER(Eotf), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "fvvdp_tap_grad_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "fvvdp_tap_grad": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}
TAPS_MAX_POSITIONS = 320                 # FVVDP_TAPS_MAX_POSITIONS
TAP_GROUP = 8                            # FVVDP_TAP_GROUP

# include/fvvdp_hip_display.h: the sums behind the gradient with respect to the display's photometry (bound by lib() as well)
DISPLAY_SYMBOLS = {
    "fvvdp_video_display_sums_workspace": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "fvvdp_video_display_sums": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t,
                                           C.POINTER(Eotf), C.POINTER(C.c_float), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                           C.c_size_t, C.c_void_p]),
    "fvvdp_images_display_sums_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "fvvdp_images_display_sums": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(PoolParams), C.c_void_p,
                                            C.c_int, C.c_int, C.c_void_p, C.POINTER(BandMaps), C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_void_p), C.c_int, C.c_size_t, C.POINTER(Eotf), C.POINTER(C.c_float),
                                            C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}
DISPLAY_SUMS = 3                         # FVVDP_DISPLAY_SUMS

# include/fvvdp_hip_half.h: fvvdp_images_grad, fvvdp_images_ref_grad and fvvdp_video_grad_input with an `int dtype` (FVVDP_F32 /
# F16 / BF16) for the samples and the gradient, after the sample pointers (bound by lib() as well)
def _with_dtype(args, at):
    return args[:at] + [C.c_int] + args[at:]


HALF_SYMBOLS = {
    "fvvdp_images_grad_st": (C.c_int, _with_dtype(GRAD_SYMBOLS["fvvdp_images_grad"][1], 12)),
    "fvvdp_images_ref_grad_st": (C.c_int, _with_dtype(REF_GRAD_SYMBOLS["fvvdp_images_ref_grad"][1], 13)),
    "fvvdp_video_grad_input_st": (C.c_int, _with_dtype(VIDEO_GRAD_SYMBOLS["fvvdp_video_grad_input"][1], 10)),
}

# include/fvvdp_hip_diffmap.h: the difference map before its power and the gradient of a per-pixel cotangent of the map (bound by
# lib() as well)
DIFFMAP_SYMBOLS = {
    "fvvdp_heatmap_reconstruct_linear": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_float, C.c_void_p, C.c_void_p]),
    "fvvdp_diffmap_grad_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t),
                                               C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "fvvdp_diffmap_grad_levels": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(PoolParams),
                                            C.c_int, C.c_void_p, C.c_void_p, C.POINTER(BandMaps), C.c_void_p, C.c_size_t, C.c_void_p]),
    "fvvdp_diffmap_images_grad": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(PoolParams), C.c_int,
                                            C.c_void_p, C.c_void_p, C.POINTER(BandMaps), C.POINTER(C.c_void_p), C.c_int, C.c_int,
                                            C.c_size_t, C.POINTER(Eotf), C.POINTER(C.c_float), C.POINTER(C.c_void_p), C.c_void_p,
                                            C.c_size_t, C.c_void_p]),
    "fvvdp_diffmap_video_grad_frames": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(PoolParams),
                                                  C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(BandMaps), C.c_void_p,
                                                  C.c_void_p, C.c_size_t, C.c_void_p]),
}
DIFFMAP_JOD, DIFFMAP_LINEAR = 0, 1       # FVVDP_DIFFMAP_JOD, FVVDP_DIFFMAP_LINEAR

# include/fvvdp_hip_yuv_grad.h: planar YUV clips of float32 code values -- their ingest, the temporal transpose down to the
# luminance frames and the adjoint of the unpack (bound by lib() as well)
YUV_GRAD_SYMBOLS = {
    "fvvdp_temporal_channels_yuv_planes": (C.c_int, [C.c_void_p, C.POINTER(YuvPlanes), C.POINTER(YuvPlanes), C.POINTER(YuvFormat),
                                                     C.POINTER(Eotf), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                                     C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fvvdp_video_grad_luminance": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                             C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "fvvdp_yuv_grad_planes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(YuvPlanes), C.POINTER(YuvPlanes),
                                        C.POINTER(YuvFormat), C.POINTER(Eotf), C.POINTER(C.c_float), C.c_void_p]),
}
YUV_GRAD_MAX_TAPS = 32                   # FVVDP_YUV_GRAD_MAX_TAPS

# include/fvvdp_hip_resize.h: clips whose streams have frame sizes of their own -- the resize fused into the ingest, and its adjoint
# (bound by lib() as well)
RESIZE_SYMBOLS = {
    "fvvdp_temporal_channels_resized": (C.c_int, [C.c_void_p, C.POINTER(ResizeStream), C.POINTER(ResizeStream), C.c_int,
                                                  C.POINTER(Eotf), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                                  C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "fvvdp_resize_grad": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(ResizeStream), C.c_void_p, C.c_int,
                                    C.POINTER(Eotf), C.POINTER(C.c_float), C.c_void_p, C.c_size_t, C.c_void_p]),
}
RESIZE_MAX_TAPS = 32                     # FVVDP_RESIZE_MAX_TAPS


def resize_grad_table_bytes(width, height):
    """FVVDP_RESIZE_GRAD_TABLE_BYTES"""
    return (2 * (width + height) * 4 + 255) // 256 * 256


# include/fvvdp_hip_tests_grad.h: gradients of many tests' video JODs with respect to their one reference (bound by lib() as well)
TESTS_GRAD_SYMBOLS = {
    "fvvdp_tests_ref_grad_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "fvvdp_tests_ref_grad_layer": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.POINTER(Params), C.POINTER(PoolParams), C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                             C.POINTER(BandMaps), C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p]),
    "fvvdp_tests_ref_grad_finish": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_size_t, C.c_void_p]),
}
TESTS_GRAD_GROUP_MAX = 4                 # FVVDP_TESTS_GRAD_GROUP_MAX

# include/fvvdp_hip_held.h: clips whose streams have frame counts of their own -- held frames in the ingest, and the transpose of the
# hold in the last kernel of the backward (bound by lib() as well)
class HeldStream(C.Structure):
    """fvvdp_held_stream (include/fvvdp_hip_held.h): one stream with its own strides (in elements) and frame count."""
    _fields_ = [("d_data", C.c_void_p), ("chan_stride", C.c_size_t), ("frame_stride", C.c_size_t), ("n_frames", C.c_int32)]


HELD_SYMBOLS = {
    "fvvdp_temporal_channels_held": (C.c_int, [C.c_void_p, C.POINTER(HeldStream), C.POINTER(HeldStream), C.c_int, C.c_int,
                                               C.POINTER(Eotf), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                               C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fvvdp_video_grad_input_held": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int32),
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(Eotf),
                                              C.POINTER(C.c_float), C.c_void_p, C.c_size_t, C.c_void_p]),
}
HELD_MAX_TAPS = 32                       # FVVDP_HELD_MAX_TAPS


def held_map_bytes(n_display):
    """FVVDP_HELD_MAP_BYTES"""
    return (n_display * 4 + 255) // 256 * 256


# include/fvvdp_hip_images_resize.h: still images whose stacks have image sizes of their own -- the resize fused into the still-image
# ingest, and the level-0 step of the still-image backward that ends in luminance (bound by lib() as well)
IMAGES_RESIZE_SYMBOLS = {
    "fvvdp_images_channels_resized": (C.c_int, [C.c_void_p, C.POINTER(ResizeStream), C.POINTER(ResizeStream), C.c_int, C.c_int,
                                                C.POINTER(Eotf), C.POINTER(C.c_float), C.c_int, C.c_void_p]),
    "fvvdp_images_grad_luminance_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "fvvdp_images_grad_luminance": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(PoolParams), C.c_void_p,
                                              C.c_int, C.c_int, C.c_void_p, C.POINTER(BandMaps), C.POINTER(C.c_void_p), C.c_void_p,
                                              C.c_void_p, C.c_size_t, C.c_void_p]),
}
RESIZE_MAX_AXIS = 32768                  # FVVDP_RESIZE_MAX_AXIS

# include/fvvdp_hip_resize_held.h: clips whose streams have frame sizes and frame counts of their own -- the resizing ingest with a
# window list per stream, and the resize's adjoint behind the transpose of the hold (bound by lib() as well)
RESIZE_HELD_SYMBOLS = {
    "fvvdp_temporal_channels_resized_held": (C.c_int, [C.c_void_p, C.POINTER(ResizeStream), C.POINTER(ResizeStream), C.c_int, C.c_int,
                                                       C.c_int, C.POINTER(Eotf), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                                       C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int,
                                                       C.c_void_p]),
    "fvvdp_resize_grad_held": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(ResizeStream),
                                         C.c_void_p, C.c_int, C.POINTER(Eotf), C.POINTER(C.c_float), C.c_void_p, C.c_size_t,
                                         C.c_void_p]),
}


def resize_grad_held_table_bytes(width, height, n_source):
    """FVVDP_RESIZE_GRAD_HELD_TABLE_BYTES"""
    return ((2 * (width + height) + n_source + 1) * 4 + 255) // 256 * 256


_lib = None


def build(force=False, verbose=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU).  Twenty-seven translation units -- the band /
    pooling / side-metric kernels with the C ABI (the many-gazes pass of fvvdp_hip_gaze.h and the many-tests passes of fvvdp_hip_tests.h and fvvdp_hip_tests_fov.h among them;
    their launch plans and bounds are the host-only header pyramid_host.hpp, the strip constants pyramid_constants.hpp), the temporal kernels once
    per sample type (temporal_launch.hip with -DK1_PART=0..5: uint8, uint16, float32, planar YUV with the dispatcher, float16, bfloat16), the batched still-image ingest (still_launch.hip), the still-image gradients (grad_launch.hip), the
    video gradients (video_grad_launch.hip), the video gradients under many gazes (gaze_grad_launch.hip), the gradients with
    respect to the reference (ref_grad_launch.hip), the sums for the gradients with respect to the model parameters
    (param_launch.hip), the gradient with respect to the temporal taps (tap_grad_launch.hip), the sums for the gradient with
    respect to the display's photometry (display_grad_launch.hip), the gradients of the difference map (map_grad_launch.hip), the
    float YUV planes with their gradients (yuv_grad_launch.hip), the gradients of many tests with respect to their one reference
    (tests_grad_launch.hip), the clips resized inside the ingest with the resize's adjoint (resize_launch.hip), the still images
    resized inside their ingest (images_resize_launch.hip), the resized clips shown through frame maps (resize_held_launch.hip) and the clips with held frames (held_launch.hip with -DHELD_PART=0..5: the ingest per sample type, then the C ABI with the backward's kernel) -- are
    compiled concurrently and linked into one shared library."""
    csrc = os.path.dirname(SRC_PATH)
    deps = [os.path.join(csrc, f) for f in os.listdir(csrc) if not f.startswith("_")] + [os.path.join(INCLUDE_DIR, h) for h in ("fvvdp_hip.h", "fvvdp_hip_images.h", "fvvdp_hip_grad.h",
                                                                                                                              "fvvdp_hip_video_grad.h", "fvvdp_hip_gaze.h", "fvvdp_hip_gaze_grad.h",
                                                                                                                              "fvvdp_hip_ref_grad.h", "fvvdp_hip_params.h", "fvvdp_hip_taps.h",
                                                                                                                              "fvvdp_hip_display.h", "fvvdp_hip_half.h", "fvvdp_hip_diffmap.h",
                                                                                                                              "fvvdp_hip_yuv_grad.h", "fvvdp_hip_tests.h", "fvvdp_hip_tests_grad.h",
                                                                                                                              "fvvdp_hip_resize.h", "fvvdp_hip_held.h", "fvvdp_hip_images_resize.h",
                                                                                                                              "fvvdp_hip_resize_held.h", "fvvdp_hip_tests_fov.h")]
    if not force and os.path.isfile(LIB_PATH) and os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(f) for f in deps):
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # -pragma-unroll-threshold: the temporal kernels keep their filter window in registers and rely on FULL unrolling
    # of the tap loops (static ring slots); the default size cap silently falls back to scratch-memory indexing
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-pragma-unroll-threshold=1000000",
             "-I" + INCLUDE_DIR, "-I" + csrc] + os.environ.get("FVVDP_HIPCC_FLAGS", "").split()
    objdir = os.path.join(csrc, "_build")
    os.makedirs(objdir, exist_ok=True)
    units = [(SRC_PATH, [], os.path.join(objdir, "fvvdp_hip.o"))]
    units += [(os.path.join(csrc, "temporal_launch.hip"), ["-DK1_PART=%d" % k], os.path.join(objdir, "temporal_part%d.o" % k))
              for k in range(6)]
    # the batched still-image ingest: per-pixel arithmetic identical to the single-image kernel (see still_launch.hip)
    units += [(os.path.join(csrc, "still_launch.hip"), ["-fno-slp-vectorize"], os.path.join(objdir, "still_launch.o"))]
    # gradients of the still-image JOD (include/fvvdp_hip_grad.h)
    units += [(os.path.join(csrc, "grad_launch.hip"), [], os.path.join(objdir, "grad_launch.o"))]
    # gradients of the video JOD (include/fvvdp_hip_video_grad.h)
    units += [(os.path.join(csrc, "video_grad_launch.hip"), [], os.path.join(objdir, "video_grad_launch.o"))]
    # gradients of the video JOD under many gazes (include/fvvdp_hip_gaze_grad.h)
    units += [(os.path.join(csrc, "gaze_grad_launch.hip"), [], os.path.join(objdir, "gaze_grad_launch.o"))]
    # gradients with respect to the reference (include/fvvdp_hip_ref_grad.h)
    units += [(os.path.join(csrc, "ref_grad_launch.hip"), [], os.path.join(objdir, "ref_grad_launch.o"))]
    # the sums for the gradients with respect to the model parameters (include/fvvdp_hip_params.h)
    units += [(os.path.join(csrc, "param_launch.hip"), [], os.path.join(objdir, "param_launch.o"))]
    # the gradient with respect to the taps of the temporal filters (include/fvvdp_hip_taps.h).  -fno-slp-vectorize: packed
    # multiply-adds want the rotating ring slots in aligned register pairs; the moves that arrange them cost more than the packing
    # saves and push the kernel past the registers of two waves per SIMD
    units += [(os.path.join(csrc, "tap_grad_launch.hip"), ["-fno-slp-vectorize"], os.path.join(objdir, "tap_grad_launch.o"))]
    # the sums behind the gradient with respect to the display's photometry (include/fvvdp_hip_display.h)
    units += [(os.path.join(csrc, "display_grad_launch.hip"), [], os.path.join(objdir, "display_grad_launch.o"))]
    # the gradients of the difference map (include/fvvdp_hip_diffmap.h)
    units += [(os.path.join(csrc, "map_grad_launch.hip"), [], os.path.join(objdir, "map_grad_launch.o"))]
    # planar YUV clips of float32 code values: ingest and gradients (include/fvvdp_hip_yuv_grad.h).  -ffp-contract=off: the ingest
    # evaluates the unpack of the test and of the reference stream as two copies of scalar code, and left to itself the compiler
    # fuses a multiply-add in one copy and not in the other -- an identical pair then has a level 0 that differs in the last bit
    # and a gradient of 1e-8 where the reference has an exact zero.  Every fused multiply-add of this unit is written as one
    units += [(os.path.join(csrc, "yuv_grad_launch.hip"), ["-ffp-contract=off"], os.path.join(objdir, "yuv_grad_launch.o"))]
    # gradients of many tests with respect to their one reference (include/fvvdp_hip_tests_grad.h).  Default flags, as
    # ref_grad_launch.hip: ref_layer_one must compile to the arithmetic it has there
    units += [(os.path.join(csrc, "tests_grad_launch.hip"), [], os.path.join(objdir, "tests_grad_launch.o"))]
    # clips resized inside the ingest, and the resize's adjoint (include/fvvdp_hip_resize.h).  -ffp-contract=off for the reason
    # given for yuv_grad_launch.hip: the interpolation of the test and of the reference stream are two copies of scalar code, and the
    # adjoint recomputes the test's values to decide the clip as the forward decided it -- all three must round alike
    units += [(os.path.join(csrc, "resize_launch.hip"), ["-ffp-contract=off"], os.path.join(objdir, "resize_launch.o"))]
    # clips whose streams have frame counts of their own (include/fvvdp_hip_held.h): the held ingest once per sample type
    # (-DHELD_PART=0..4, new instantiations of the ring bodies of temporal_launch.hip), and the C ABI with the backward's kernel (5)
    units += [(os.path.join(csrc, "held_launch.hip"), ["-DHELD_PART=%d" % k], os.path.join(objdir, "held_part%d.o" % k))
              for k in range(6)]
    # still images resized inside their ingest, and the level-0 step that ends in luminance (include/fvvdp_hip_images_resize.h).
    # -ffp-contract=off as resize_launch.hip: the ingest evaluates the functions that unit's adjoint recomputes, and the two stacks
    # are two copies of scalar code -- all must round alike
    units += [(os.path.join(csrc, "images_resize_launch.hip"), ["-ffp-contract=off"], os.path.join(objdir, "images_resize_launch.o"))]
    # clips resized inside the ingest AND shown through frame maps (include/fvvdp_hip_resize_held.h): the hold variants of
    # resize_launch.hip's kernels.  -ffp-contract=off as that unit: a reused luminance must be the value the unit beside it computes
    units += [(os.path.join(csrc, "resize_held_launch.hip"), ["-ffp-contract=off"], os.path.join(objdir, "resize_held_launch.o"))]
    procs = []
    for src, extra, obj in units:
        cmd = [hipcc] + flags + extra + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(csrc, "exports.map")] + \
          [u[2] for u in units] + ["-o", LIB_PATH]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError("libfvvdp_hip.so is not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'`. "
                               "There is no CPU fallback for the hot path." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SYMBOLS.items()) + list(IMAGE_SYMBOLS.items()) + list(GRAD_SYMBOLS.items()) + \
                list(VIDEO_GRAD_SYMBOLS.items()) + list(GAZE_SYMBOLS.items()) + list(GAZE_GRAD_SYMBOLS.items()) + \
                list(REF_GRAD_SYMBOLS.items()) + list(PARAM_SYMBOLS.items()) + list(TAP_SYMBOLS.items()) + \
                list(DISPLAY_SYMBOLS.items()) + list(HALF_SYMBOLS.items()) + list(DIFFMAP_SYMBOLS.items()) + \
                list(YUV_GRAD_SYMBOLS.items()) + list(MULTITEST_SYMBOLS.items()) + list(TESTS_GRAD_SYMBOLS.items()) + \
                list(RESIZE_SYMBOLS.items()) + list(HELD_SYMBOLS.items()) + list(IMAGES_RESIZE_SYMBOLS.items()) + \
                list(RESIZE_HELD_SYMBOLS.items()) + list(TESTS_FOV_SYMBOLS.items()):
            fn = getattr(L, name)        # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError(lib().fvvdp_last_error().decode("utf-8", "replace"))


def fptr(arr):
    """numpy fp32 array -> float*"""
    return arr.ctypes.data_as(C.POINTER(C.c_float))
