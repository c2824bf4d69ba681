// Planar YUV clips of float32 code values (include/fvvdp_hip_yuv_grad.h): argument checks and launches of the kernels of
// yuv_grad_kernels.hpp.  A translation unit of its own: it instantiates no kernel template of the other units, and the one
// function that needs a context asks fvvdp_hip.hip for the context's side of the call (fvvdp_ctx_ingest_begin).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "fvvdp_hip.h"
#include "fvvdp_hip_video_grad.h"
#include "fvvdp_hip_yuv_grad.h"
#include "device_common.hpp"
#include "temporal_launch.hpp"     // fvvdp_ctx_ingest_begin
#include "grad_common.hpp"
#include "transpose_kernels.hpp"
#include "yuv_grad_kernels.hpp"
#include "grad_host.hpp"

static_assert(FVVDP_VIDEO_GRAD_MAX_TAPS == TRANSPOSE_MAX_FL, "fvvdp_video_grad_luminance has the reach of fvvdp_video_grad_input");
static_assert(FVVDP_YUV_GRAD_MAX_TAPS == 32, "YuvPlanesArgs::taps2");

static int check_format(const fvvdp_yuv_format* fmt, int width, int height) {
    if (fmt->bit_depth < 8 || fmt->bit_depth > 16) return grad_fail(FVVDP_EINVAL, "bit depth %d not supported", fmt->bit_depth);
    if (fmt->chroma_420 && ((width | height) & 1)) return grad_fail(FVVDP_EINVAL, "4:2:0 needs even frame dimensions");
    return FVVDP_OK;
}

// pointers set and 4-byte aligned, strides that hold a plane
static int check_planes(const fvvdp_yuv_planes* p, const char* what, size_t HW, size_t uv) {
    if (!p->d_y || !p->d_u || !p->d_v) return grad_fail(FVVDP_EINVAL, "null plane pointer (%s)", what);
    const uintptr_t ptrs = reinterpret_cast<uintptr_t>(p->d_y) | reinterpret_cast<uintptr_t>(p->d_u) | reinterpret_cast<uintptr_t>(p->d_v);
    if (ptrs % 4 != 0) return grad_fail(FVVDP_EINVAL, "plane pointers must be aligned to 4 bytes (%s)", what);
    if (p->luma_stride < HW) return grad_fail(FVVDP_EINVAL, "luma_stride %zu is below the plane size %zu (%s)", p->luma_stride, HW, what);
    if (p->chroma_stride < uv) return grad_fail(FVVDP_EINVAL, "chroma_stride %zu is below the plane size %zu (%s)", p->chroma_stride, uv, what);
    return FVVDP_OK;
}

static void fill_unpack(YuvUnpack& k, int width, int height, const fvvdp_yuv_format* fmt, const fvvdp_eotf* eotf, const float* h_rgb2y) {
    ingest_fill_unpack(k, width, height, fmt);
    grad_fill_eotf(k.e, k.w, eotf, 3, h_rgb2y);
}

static YuvPlaneSet plane_set(const fvvdp_yuv_planes* p) {
    return YuvPlaneSet{p->d_y, p->d_u, p->d_v, p->luma_stride, p->chroma_stride};
}

// the 16-byte luma (and 4:4:4 chroma) loads and the 8-byte chroma loads of the fast path
static bool planes_vector_ok(const fvvdp_yuv_planes* p, bool c420) {
    const size_t ca = c420 ? 8 : 16;
    return reinterpret_cast<uintptr_t>(p->d_y) % 16 == 0 && reinterpret_cast<uintptr_t>(p->d_u) % ca == 0 &&
           reinterpret_cast<uintptr_t>(p->d_v) % ca == 0 && p->luma_stride % 4 == 0 && p->chroma_stride % (ca / 4) == 0;
}

template <int FL>
static void launch_vec(bool c420, const YuvPlanesArgs& a, hipStream_t st) {
    const size_t quads = (size_t)a.k.W * a.k.H / YP_PX;
    const dim3 grid((unsigned int)((quads + 255) / 256)), block(256);
    if (c420) hipLaunchKernelGGL((yuvplanes_vec_kernel<FL, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((yuvplanes_vec_kernel<FL, false>), grid, block, 0, st, a);
}
template <int FL, int PX>
static void launch_ring(const YuvPlanesArgs& a, hipStream_t st) {
    const size_t HW = (size_t)a.k.W * a.k.H;
    hipLaunchKernelGGL((yuvplanes_ring_kernel<FL, PX>), dim3((unsigned int)((HW + 256 * PX - 1) / (256 * PX))), dim3(256), 0, st, a);
}

extern "C" int fvvdp_temporal_channels_yuv_planes(fvvdp_ctx* ctx, const fvvdp_yuv_planes* test, const fvvdp_yuv_planes* ref,
                                                  const fvvdp_yuv_format* fmt, const fvvdp_eotf* eotf, const float* h_rgb2y,
                                                  const int32_t* h_frame_idx, const float* h_taps, int fl, int n_out, int slot0,
                                                  int32_t* d_oob_flag, void* stream) {
    if (!ctx || !test || !ref || !fmt || !eotf || !h_rgb2y || !h_frame_idx || !h_taps) return grad_fail(FVVDP_EINVAL, "null argument");
    if (fmt->bit_depth < 8 || fmt->bit_depth > 16) return grad_fail(FVVDP_EINVAL, "bit depth %d not supported", fmt->bit_depth);
    if (fl < 1 || fl > FVVDP_MAX_TAPS) return grad_fail(FVVDP_EINVAL, "filter length %d outside [1, %d]", fl, FVVDP_MAX_TAPS);
    if (fl > FVVDP_YUV_GRAD_MAX_TAPS)
        return grad_fail(FVVDP_EUNSUPPORTED, "the ingest of float YUV planes covers temporal filters of up to %d taps (120 frames per "
                                             "second); this one has %d", FVVDP_YUV_GRAD_MAX_TAPS, fl);
    if (eotf->kind < FVVDP_EOTF_SRGB || eotf->kind > FVVDP_EOTF_ABSOLUTE)
        return grad_fail(FVVDP_EINVAL, "YUV sources need a closed-form display model (RGB is fractional after the matrix)");
    if (reinterpret_cast<uintptr_t>(d_oob_flag) % 4 != 0) return grad_fail(FVVDP_EINVAL, "d_oob_flag must be aligned to 4 bytes");
    // the plane pointers before the context is touched: its frame size is not known yet, so the strides follow below
    GRAD_CHECK(check_planes(test, "test", 0, 0));
    GRAD_CHECK(check_planes(ref, "reference", 0, 0));
    IngestBegin b;
    GRAD_CHECK(fvvdp_ctx_ingest_begin(ctx, "YUV ingest", fmt->chroma_420 != 0, 3, eotf, h_rgb2y, h_taps, fl, n_out, slot0, &b));
    const int W = b.W, H = b.H;
    const size_t HW = (size_t)W * H;
    const bool c420 = fmt->chroma_420 != 0;
    const size_t uv = c420 ? (size_t)(W / 2) * (H / 2) : HW;
    GRAD_CHECK(check_planes(test, "test", HW, uv));
    GRAD_CHECK(check_planes(ref, "reference", HW, uv));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    const int FL = ingest_ring_length(fl);
    const bool vec = FL <= 16 && W % 4 == 0 && planes_vector_ok(test, c420) && planes_vector_ok(ref, c420);
    for (const IngestWindow wnd : IngestWindows(fl, n_out)) {
        YuvPlanesArgs a;
        memset(&a, 0, sizeof(a));
        a.src[0] = plane_set(test);
        a.src[1] = plane_set(ref);
        fill_unpack(a.k, W, H, fmt, eotf, h_rgb2y);
        a.out = b.out;
        a.oob = d_oob_flag;
        if (const int32_t* f = ingest_fill_window(a, wnd, slot0, h_taps, fl, h_frame_idx))
            return grad_fail(FVVDP_EINVAL, "frame index %d out of range", *f);
        if (vec) {
            if (FL == 8) launch_vec<8>(c420, a, st);
            else launch_vec<16>(c420, a, st);
        } else if (FL == 8) {
            launch_ring<8, 2>(a, st);
        } else if (FL == 16) {
            launch_ring<16, 2>(a, st);
        } else {
            launch_ring<32, 1>(a, st);
        }
        GRAD_HIP_TRY(hipGetLastError());
    }
    return FVVDP_OK;
}

template <int FL>
static void launch_lum_input(const LumInputArgs& ia, bool vec, hipStream_t st) {
    constexpr int PXV = transpose_px(FL);
    const size_t HW = (size_t)ia.t.HW;
    if (vec) hipLaunchKernelGGL((video_lum_input_kernel<FL, PXV>), dim3((unsigned int)((HW / PXV + 255) / 256)), dim3(256), 0, st, ia);
    else hipLaunchKernelGGL((video_lum_input_kernel<FL, 1>), dim3((unsigned int)((HW + 255) / 256)), dim3(256), 0, st, ia);
}

extern "C" int fvvdp_video_grad_luminance(int width, int height, int n_frames, const float* d_g0, const int32_t* h_fold_frame,
                                          const int32_t* h_fold_pos, const float* h_taps, int fl, float* d_gL, float* d_head,
                                          size_t head_bytes, void* stream) {
    if (!d_g0 || !h_fold_frame || !h_fold_pos || !h_taps || !d_gL || !d_head) return grad_fail(FVVDP_EINVAL, "null argument");
    if (width < 1 || height < 1 || n_frames < 1) return grad_fail(FVVDP_EINVAL, "bad shape %dx%d, %d frames", width, height, n_frames);
    const size_t HW = (size_t)width * height;
    if (HW > 0x7FFFFFFFu) return grad_fail(FVVDP_EINVAL, "frame of %zu pixels is too large", HW);
    if (fl < 1 || fl > FVVDP_MAX_TAPS) return grad_fail(FVVDP_EINVAL, "filter length %d outside [1, %d]", fl, FVVDP_MAX_TAPS);
    if (fl > FVVDP_VIDEO_GRAD_MAX_TAPS)
        return grad_fail(FVVDP_EUNSUPPORTED, "the video backward covers temporal filters of up to %d taps (256 frames per second); "
                                             "this one has %d", FVVDP_VIDEO_GRAD_MAX_TAPS, fl);
    GRAD_CHECK(grad_verdict(transpose_check_fold(h_fold_frame, h_fold_pos, fl, n_frames, "frame")));
    GRAD_CHECK(grad_verdict(transpose_check_head_bytes(head_bytes, fl, HW)));
    const uintptr_t ptrs = reinterpret_cast<uintptr_t>(d_g0) | reinterpret_cast<uintptr_t>(d_head) | reinterpret_cast<uintptr_t>(d_gL);
    if (ptrs % 4 != 0) return grad_fail(FVVDP_EINVAL, "device pointers must be aligned to 4 bytes");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    LumInputArgs ia;
    memset(&ia, 0, sizeof(ia));
    transpose_fill(ia.t, d_g0, d_head, HW, n_frames, fl, h_taps, h_fold_frame, h_fold_pos);
    ia.gL = d_gL;
    const int FL = transpose_ring_length(fl, TRANSPOSE_MAX_FL);
    const bool vec = transpose_vector_ok(FL, HW, 0, ptrs);
    transpose_dispatch<TRANSPOSE_MAX_FL>(FL, [&](auto c) { launch_lum_input<c.value>(ia, vec, st); });
    GRAD_HIP_TRY(hipGetLastError());
    return FVVDP_OK;
}

extern "C" int fvvdp_yuv_grad_planes(int width, int height, int n_frames, const float* d_gL, const fvvdp_yuv_planes* test,
                                     const fvvdp_yuv_planes* grad, const fvvdp_yuv_format* fmt, const fvvdp_eotf* eotf,
                                     const float* h_rgb2y, void* stream) {
    if (!d_gL || !test || !grad || !fmt || !eotf || !h_rgb2y) return grad_fail(FVVDP_EINVAL, "null argument");
    // 65535 frames and 65535 * 32 rows: grid dimensions of the two kernels
    if (width < 1 || height < 1 || n_frames < 1 || n_frames > 65535 || height > 65535 * YA_TH)
        return grad_fail(FVVDP_EINVAL, "bad shape %dx%d, %d frames", width, height, n_frames);
    const size_t HW = (size_t)width * height;
    if (HW > 0x7FFFFFFFu) return grad_fail(FVVDP_EINVAL, "frame of %zu pixels is too large", HW);
    GRAD_CHECK(check_format(fmt, width, height));
    GRAD_CHECK(grad_check_closed_form(eotf));
    const bool c420 = fmt->chroma_420 != 0;
    const size_t uv = c420 ? (size_t)(width / 2) * (height / 2) : HW;
    GRAD_CHECK(check_planes(test, "test", HW, uv));
    GRAD_CHECK(check_planes(grad, "gradient", HW, uv));
    if (reinterpret_cast<uintptr_t>(d_gL) % 4 != 0) return grad_fail(FVVDP_EINVAL, "d_gL must be aligned to 4 bytes");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    YuvAdjArgs a;
    memset(&a, 0, sizeof(a));
    a.gL = d_gL;
    a.t = plane_set(test);
    a.gy = const_cast<float*>(grad->d_y);
    a.gu = const_cast<float*>(grad->d_u);
    a.gv = const_cast<float*>(grad->d_v);
    a.gys = grad->luma_stride;
    a.gcs = grad->chroma_stride;
    fill_unpack(a.k, width, height, fmt, eotf, h_rgb2y);
    if (c420) {
        const dim3 grid((width + YA_TW - 1) / YA_TW, (height + YA_TH - 1) / YA_TH, n_frames);
        hipLaunchKernelGGL(yuv_adjoint_420_kernel, grid, dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL(yuv_adjoint_444_kernel, dim3((unsigned int)((HW + 255) / 256), n_frames), dim3(256), 0, st, a);
    }
    GRAD_HIP_TRY(hipGetLastError());
    return FVVDP_OK;
}
