// The gradient of the JOD with respect to the taps of the temporal filters (include/fvvdp_hip_taps.h): argument checks, workspace
// layout and launches of tap_grad_kernel / tap_finalize_kernel (tap_grad_kernels.hpp), and fvvdp_luminance_frames, an entry point
// around the luminance pass of the temporal kernels (k1_launch_luminance, temporal_launch.hip).  A translation unit of its own: it
// reads only what the caller passes, never a context.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "fvvdp_hip.h"
#include "fvvdp_hip_video_grad.h"
#include "fvvdp_hip_taps.h"
#include "device_common.hpp"
#include "temporal_launch.hpp"
#include "transpose_kernels.hpp"   // LaneVec
#include "tap_grad_kernels.hpp"

int fvvdp_fail_from(int code, const char* msg);      // fvvdp_hip.hip: sets the message of fvvdp_last_error
EotfDev fvvdp_eotf_dev(const fvvdp_eotf* e);         // fvvdp_hip.hip: the display model as the temporal kernels take it

static_assert(FVVDP_TAPS_MAX_POSITIONS <= T_MAX_IDX, "LumArgs::fr holds one entry per frame of a call");

static int tap_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static int tap_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return fvvdp_fail_from(code, buf);
}

static int tap_check_frame(int width, int height) {
    if (width < 1 || height < 1 || (size_t)width * height > (size_t)1 << 30)
        return tap_fail(FVVDP_EINVAL, "bad frame size %dx%d", width, height);
    return FVVDP_OK;
}

extern "C" int fvvdp_luminance_frames(const void* d_test, const void* d_ref, int dtype, int C, int width, int height,
                                      size_t chan_stride, size_t frame_stride, const fvvdp_eotf* eotf, const float* h_rgb2y,
                                      const int32_t* h_frames, int n, float* d_out, int32_t* d_oob_flag, void* stream) {
    if (!d_test || !d_ref || !eotf || !h_frames || !d_out) return tap_fail(FVVDP_EINVAL, "null argument");
    // (FVVDP_F16 / FVVDP_BF16 are the ingest's and the *_st gradients'; this pass takes such a clip upcast: the caller's side is exact)
    if (dtype < FVVDP_U8 || dtype > FVVDP_F32) return tap_fail(FVVDP_EINVAL, "Only uint8, uint16 and float32 is currently supported");
    if (C != 1 && C != 3) return tap_fail(FVVDP_EINVAL, "The content must have either 1 or 3 colour channels.");
    if (C == 3 && !h_rgb2y) return tap_fail(FVVDP_EINVAL, "rgb2y weights required for C == 3");
    const int rc = tap_check_frame(width, height);
    if (rc != FVVDP_OK) return rc;
    if (n < 1 || n > FVVDP_TAPS_MAX_POSITIONS)
        return tap_fail(FVVDP_EINVAL, "%d frames in one call: 1 to %d are possible", n, FVVDP_TAPS_MAX_POSITIONS);
    if (eotf->kind < FVVDP_EOTF_LUT || eotf->kind > FVVDP_EOTF_NONE) return tap_fail(FVVDP_EINVAL, "unknown display model %d", eotf->kind);
    if (eotf->kind == FVVDP_EOTF_LUT && (dtype == FVVDP_F32 || !eotf->d_lut))
        return tap_fail(FVVDP_EINVAL, "FVVDP_EOTF_LUT needs an integer source and a table");
    if (eotf->kind != FVVDP_EOTF_LUT && dtype == FVVDP_U8)
        return tap_fail(FVVDP_EINVAL, "uint8 sources need FVVDP_EOTF_LUT (uint16: table or closed form)");
    const size_t es = dtype == FVVDP_U8 ? 1 : (dtype == FVVDP_U16 ? 2 : 4);
    if (reinterpret_cast<uintptr_t>(d_test) % es || reinterpret_cast<uintptr_t>(d_ref) % es)
        return tap_fail(FVVDP_EINVAL, "source pointers must be aligned to their element size");
    if (reinterpret_cast<uintptr_t>(d_out) % 4) return tap_fail(FVVDP_EINVAL, "d_out must be aligned to 4 bytes");
    LumArgs la;
    memset(&la, 0, sizeof(la));
    for (int k = 0; k < n; ++k) {
        if (h_frames[k] < 0) return tap_fail(FVVDP_EINVAL, "frame number %d is negative", h_frames[k]);
        la.fr[k] = h_frames[k];
    }
    la.src[0] = d_test;
    la.src[1] = d_ref;
    la.chan_stride = chan_stride;
    la.frame_stride = frame_stride;
    la.C = C;
    la.HW = width * height;
    la.e = fvvdp_eotf_dev(eotf);
    if (C == 3) { la.w[0] = h_rgb2y[0]; la.w[1] = h_rgb2y[1]; la.w[2] = h_rgb2y[2]; } else { la.w[0] = 1.0f; }
    la.n_frames = n;
    la.out = d_out;
    la.oob = d_oob_flag;
    k1_launch_luminance(dtype, la, reinterpret_cast<hipStream_t>(stream));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fvvdp_fail_from(FVVDP_EHIP, hipGetErrorString(e));
    return FVVDP_OK;
}

// workgroups of the correlation per tap group whatever the variant (one pixel per lane is the most), and tap groups
static int tap_layout(int width, int height, int fl, int& blocks, int& groups) {
    const int rc = tap_check_frame(width, height);
    if (rc != FVVDP_OK) return rc;
    if (fl < 1) return tap_fail(FVVDP_EINVAL, "filter length %d out of range", fl);
    if (fl > FVVDP_VIDEO_GRAD_MAX_TAPS)
        return tap_fail(FVVDP_EUNSUPPORTED, "the temporal filter has %d taps, the tap gradient covers %d (256 frames per second)", fl,
                        FVVDP_VIDEO_GRAD_MAX_TAPS);
    blocks = (int)(((size_t)width * height + 255) / 256);
    groups = (fl + TG_R - 1) / TG_R;
    return FVVDP_OK;
}

extern "C" int fvvdp_tap_grad_workspace(int width, int height, int fl, size_t* bytes) {
    if (!bytes) return tap_fail(FVVDP_EINVAL, "null argument");
    int blocks = 0, groups = 0;
    const int rc = tap_layout(width, height, fl, blocks, groups);
    if (rc != FVVDP_OK) return rc;
    *bytes = (size_t)groups * blocks * 2 * TG_R * sizeof(double);
    return FVVDP_OK;
}

extern "C" int fvvdp_tap_grad(int width, int height, int n, int fl, const float* d_g0, const float* d_g0_r, const float* d_lum_t,
                              const float* d_lum_r, const int32_t* h_pos, int n_lum, double* d_out, void* d_work, size_t work_bytes,
                              void* stream) {
    if (!d_g0 || !d_g0_r || !d_lum_t || !d_lum_r || !h_pos || !d_out || !d_work) return tap_fail(FVVDP_EINVAL, "null argument");
    int max_blocks = 0, groups = 0;
    const int rc = tap_layout(width, height, fl, max_blocks, groups);
    if (rc != FVVDP_OK) return rc;
    if (n < 1 || fl - 1 + n > FVVDP_TAPS_MAX_POSITIONS)
        return tap_fail(FVVDP_EINVAL, "%d frames under a filter of %d taps: the window list of one call holds 1 to %d entries", n, fl,
                        FVVDP_TAPS_MAX_POSITIONS);
    if (n_lum < 1) return tap_fail(FVVDP_EINVAL, "n_lum must be positive, got %d", n_lum);
    uintptr_t bits = 0;
    for (const void* p : {(const void*)d_g0, (const void*)d_g0_r, (const void*)d_lum_t, (const void*)d_lum_r})
        bits |= reinterpret_cast<uintptr_t>(p);
    if (bits % 4 != 0) return tap_fail(FVVDP_EINVAL, "the gradient and luminance planes must be aligned to 4 bytes");
    if (reinterpret_cast<uintptr_t>(d_out) % 8 != 0) return tap_fail(FVVDP_EINVAL, "d_out must be aligned to 8 bytes");
    if (reinterpret_cast<uintptr_t>(d_work) % 256 != 0) return tap_fail(FVVDP_EINVAL, "workspace must be 256-byte aligned");
    const size_t need = (size_t)groups * max_blocks * 2 * TG_R * sizeof(double);
    if (work_bytes < need) return tap_fail(FVVDP_EINVAL, "workspace of %zu bytes is below the %zu needed", work_bytes, need);
    TapGradArgs a;
    memset(&a, 0, sizeof(a));
    for (int q = 0; q < fl - 1 + n; ++q) {
        if (h_pos[q] < 0 || h_pos[q] >= n_lum)
            return tap_fail(FVVDP_EINVAL, "window list entry %d names luminance frame %d of %d", q, h_pos[q], n_lum);
        a.pos[q] = h_pos[q];
    }
    a.g0 = d_g0;
    a.g0r = d_g0_r;
    a.yt = d_lum_t;
    a.yr = d_lum_r;
    a.partial = static_cast<double*>(d_work);
    a.HW = width * height;
    a.n = n;
    a.fl = fl;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t HW = (size_t)a.HW;
    const bool vec = HW % 4 == 0 && bits % 16 == 0;
    const int blocks = vec ? (int)((HW / 4 + 255) / 256) : max_blocks;
    if (vec) hipLaunchKernelGGL((tap_grad_kernel<TG_R, 4>), dim3(blocks, groups), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((tap_grad_kernel<TG_R, 1>), dim3(blocks, groups), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fvvdp_fail_from(FVVDP_EHIP, hipGetErrorString(e));
    TapFinalizeArgs f;
    f.partial = a.partial;
    f.out = d_out;
    f.blocks = blocks;
    f.fl = fl;
    hipLaunchKernelGGL(tap_finalize_kernel, dim3(groups), dim3(256), 0, st, f);
    e = hipGetLastError();
    if (e != hipSuccess) return fvvdp_fail_from(FVVDP_EHIP, hipGetErrorString(e));
    return FVVDP_OK;
}
