// The sums behind the gradient of the JOD with respect to the display's photometry (include/fvvdp_hip_display.h): argument
// checks, workspace layout and launches of the kernels of display_grad_kernels.hpp and, through grad_launch.hip and
// ref_grad_launch.hip, of the still-image backward's kernels before its last.  A translation unit of its own: it reads only what
// the caller passes, never a context, and changes nothing the forward path or the other gradients compile.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "fvvdp_hip.h"
#include "fvvdp_hip_video_grad.h"
#include "fvvdp_hip_display.h"
#include "device_common.hpp"
#include "temporal_kernels.hpp"
#include "grad_common.hpp"
#include "transpose_kernels.hpp"
#include "display_grad_kernels.hpp"
#include "grad_host.hpp"

static_assert(FVVDP_VIDEO_GRAD_MAX_TAPS == TRANSPOSE_MAX_FL, "the ring reaches as far as the video backward's");

// the five parameters exist for fvvdp_display_photo_eotf's four models only
static int check_display_model(const fvvdp_eotf* eotf) {
    if (eotf->kind < FVVDP_EOTF_LUT || eotf->kind > FVVDP_EOTF_NONE) return grad_fail(FVVDP_EINVAL, "unknown display model %d", eotf->kind);
    if (eotf->kind < FVVDP_EOTF_SRGB || eotf->kind > FVVDP_EOTF_LINEAR)
        return grad_fail(FVVDP_EUNSUPPORTED, "the display's gradient needs a display model with Y_peak, contrast, E_ambient, k_refl "
                                             "and gamma (SRGB, GAMMA, PQ or LINEAR); ABSOLUTE, LUT and NONE have none");
    return FVVDP_OK;
}

static int check_frame(int width, int height, size_t& HW) {
    if (width < 1 || height < 1) return grad_fail(FVVDP_EINVAL, "bad frame size %dx%d", width, height);
    HW = (size_t)width * height;
    if (HW > 0x7FFFFFFFu) return grad_fail(FVVDP_EINVAL, "frame of %zu pixels is too large", HW);
    return FVVDP_OK;
}

static int check_out_and_work(const double* d_out, const void* d_work, size_t work_bytes, size_t need) {
    if (reinterpret_cast<uintptr_t>(d_out) % 8 != 0) return grad_fail(FVVDP_EINVAL, "d_out must be aligned to 8 bytes");
    if (reinterpret_cast<uintptr_t>(d_work) % 256 != 0) return grad_fail(FVVDP_EINVAL, "workspace must be 256-byte aligned");
    if (work_bytes < need) return grad_fail(FVVDP_EINVAL, "workspace of %zu bytes is below the %zu needed", work_bytes, need);
    return FVVDP_OK;
}

static hipError_t finalize_launch(const double* partial, double* d_out, int outputs, int blocks, hipStream_t st) {
    DisplayFinalizeArgs f;
    f.partial = partial;
    f.out = d_out;
    f.blocks = blocks;
    hipLaunchKernelGGL(display_finalize_kernel, dim3(outputs), dim3(256), 0, st, f);
    return hipGetLastError();
}

// ---- video -------------------------------------------------------------------------------------------------------------------
extern "C" int fvvdp_video_display_sums_workspace(int width, int height, size_t* bytes) {
    if (!bytes) return grad_fail(FVVDP_EINVAL, "null argument");
    size_t HW = 0;
    GRAD_CHECK(check_frame(width, height, HW));
    *bytes = ((HW + 255) / 256) * DS_SUMS * sizeof(double);      // one pixel per lane is the most workgroups
    return FVVDP_OK;
}

template <int FL>
static int launch_video_sums(const DisplayVideoSumsArgs& a, bool vec, hipStream_t st) {
    constexpr int PXV = transpose_px(FL);
    const size_t HW = (size_t)a.t.HW;
    const int blocks = (int)(((vec ? HW / PXV : HW) + 255) / 256);
    if (vec) hipLaunchKernelGGL((display_video_sums_kernel<FL, PXV>), dim3(blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((display_video_sums_kernel<FL, 1>), dim3(blocks), dim3(256), 0, st, a);
    return blocks;
}

extern "C" int fvvdp_video_display_sums(int width, int height, int n_frames, const float* d_g0, const int32_t* h_fold_frame,
                                        const int32_t* h_fold_pos, const float* h_taps, int fl, const float* d_src, int C,
                                        size_t chan_stride, size_t frame_stride, const fvvdp_eotf* eotf, const float* h_rgb2y,
                                        float* d_head, size_t head_bytes, double* d_out, void* d_work, size_t work_bytes,
                                        void* stream) {
    if (!d_g0 || !h_fold_frame || !h_fold_pos || !h_taps || !d_src || !eotf || !d_head || !d_out || !d_work)
        return grad_fail(FVVDP_EINVAL, "null argument");
    size_t HW = 0;
    GRAD_CHECK(check_frame(width, height, HW));
    if (n_frames < 1) return grad_fail(FVVDP_EINVAL, "bad clip length %d", n_frames);
    if (fl < 1 || fl > FVVDP_MAX_TAPS) return grad_fail(FVVDP_EINVAL, "filter length %d outside [1, %d]", fl, FVVDP_MAX_TAPS);
    if (fl > FVVDP_VIDEO_GRAD_MAX_TAPS)
        return grad_fail(FVVDP_EUNSUPPORTED, "the display's gradient covers temporal filters of up to %d taps (256 frames per "
                                             "second); this one has %d", FVVDP_VIDEO_GRAD_MAX_TAPS, fl);
    GRAD_CHECK(grad_check_channels(C, h_rgb2y));
    if (frame_stride < HW) return grad_fail(FVVDP_EINVAL, "frame_stride %zu is below the frame size %zu", frame_stride, HW);
    if (C == 3 && chan_stride < HW) return grad_fail(FVVDP_EINVAL, "chan_stride %zu is below the frame size %zu", chan_stride, HW);
    GRAD_CHECK(check_display_model(eotf));
    GRAD_CHECK(grad_verdict(transpose_check_fold(h_fold_frame, h_fold_pos, fl, n_frames, "frame")));
    GRAD_CHECK(grad_verdict(transpose_check_head_bytes(head_bytes, fl, HW)));
    const uintptr_t ptrs = reinterpret_cast<uintptr_t>(d_g0) | reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_head);
    if (ptrs % 4 != 0) return grad_fail(FVVDP_EINVAL, "device pointers must be aligned to 4 bytes");
    GRAD_CHECK(check_out_and_work(d_out, d_work, work_bytes, ((HW + 255) / 256) * DS_SUMS * sizeof(double)));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    DisplayVideoSumsArgs a;
    memset(&a, 0, sizeof(a));
    transpose_fill(a.t, d_g0, d_head, HW, n_frames, fl, h_taps, h_fold_frame, h_fold_pos);
    a.src = d_src;
    a.partial = static_cast<double*>(d_work);
    a.chan_stride = C == 3 ? chan_stride : 0;
    a.frame_stride = frame_stride;
    a.C = C;
    grad_fill_eotf(a.e, a.wgt, eotf, C, h_rgb2y);
    const int FL = transpose_ring_length(fl, TRANSPOSE_MAX_FL);
    const bool vec = transpose_vector_ok(FL, HW, frame_stride | a.chan_stride, ptrs);
    int blocks = 0;
    transpose_dispatch<TRANSPOSE_MAX_FL>(FL, [&](auto c) { blocks = launch_video_sums<c.value>(a, vec, st); });
    GRAD_HIP_TRY(hipGetLastError());
    GRAD_HIP_TRY(finalize_launch(a.partial, d_out, 1, blocks, st));
    return FVVDP_OK;
}

// ---- still images --------------------------------------------------------------------------------------------------------------
static size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// bytes of the gradient's part of the workspace (rounded up to 256) for either side
static size_t sweep_bytes(int width, int height, int n_bands, int n, bool reference) {
    if (reference) return align256(ref_images_workspace_floats(width, height, n_bands, n) * sizeof(float));
    GradLayout L;
    grad_layout(width, height, n_bands, n, 1, L);
    return align256(L.total * sizeof(float));
}

extern "C" int fvvdp_images_display_sums_workspace(int width, int height, int n_bands, int n, int reference, size_t* bytes) {
    if (!bytes) return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(grad_check_dims(width, height, n_bands, n, INT_MAX, INT_MAX, "pairs"));
    size_t HW = 0;
    GRAD_CHECK(check_frame(width, height, HW));
    *bytes = sweep_bytes(width, height, n_bands, n, reference != 0) + (size_t)n * ((HW + 255) / 256) * DS_SUMS * sizeof(double);
    return FVVDP_OK;
}

extern "C" int fvvdp_images_display_sums(int width, int height, int n_bands, int n, const fvvdp_params* prm,
                                         const fvvdp_pool_params* pool, const float* d_Q, int q_stride, int q_col0,
                                         const float* d_gamma, const fvvdp_band_maps* maps, const float* const* h_slope_ptrs,
                                         const void* const* h_img_ptrs, int C, size_t chan_stride, const fvvdp_eotf* eotf,
                                         const float* h_rgb2y, double* d_out, void* d_work, size_t work_bytes, void* stream) {
    if (!prm || !pool || !d_Q || !d_gamma || !maps || !h_img_ptrs || !eotf || !d_out || !d_work)
        return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(grad_check_dims(width, height, n_bands, n, INT_MAX, INT_MAX, "pairs"));
    size_t HW = 0;
    GRAD_CHECK(check_frame(width, height, HW));
    if (q_col0 < 0 || q_stride < 1 || q_col0 + n > q_stride) return grad_fail(FVVDP_EINVAL, "Q columns out of range");
    GRAD_CHECK(grad_check_channels(C, h_rgb2y));
    if (C == 3 && chan_stride < HW) return grad_fail(FVVDP_EINVAL, "chan_stride %zu is below the image size %zu", chan_stride, HW);
    GRAD_CHECK(check_display_model(eotf));
    GRAD_CHECK(grad_check_exponents({pool->beta_sch, pool->beta_tch, pool->beta_jod, prm->beta}));
    GRAD_CHECK(grad_check_maps(maps, n_bands));
    for (int k = 0; k < n; ++k) {
        if (!h_img_ptrs[k]) return grad_fail(FVVDP_EINVAL, "null image pointer at pair %d", k);
        if (reinterpret_cast<uintptr_t>(h_img_ptrs[k]) % 4 != 0)
            return grad_fail(FVVDP_EINVAL, "image pointers must be aligned to 4 bytes (pair %d)", k);
    }
    const bool reference = h_slope_ptrs != nullptr;
    const int blocks = (int)((HW + 255) / 256);
    const size_t sweep = sweep_bytes(width, height, n_bands, n, reference);
    GRAD_CHECK(check_out_and_work(d_out, d_work, work_bytes, sweep + (size_t)n * blocks * DS_SUMS * sizeof(double)));
    float* ws = static_cast<float*>(d_work);
    double* partial = reinterpret_cast<double*>(static_cast<char*>(d_work) + sweep);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    // coefficients, layer kernel, sweep: the gradient entry point's launches before its last
    GradLayout L;
    if (reference) {
        GRAD_CHECK(ref_images_sweep(width, height, n_bands, n, prm, pool, d_Q, q_stride, q_col0, d_gamma, maps, h_slope_ptrs, ws, &L, st));
    } else {
        grad_layout(width, height, n_bands, n, 1, L);
        GRAD_CHECK(grad_images_sweep(n_bands, n, prm, pool, d_Q, q_stride, q_col0, d_gamma, maps, ws, L, st));
    }

    // level 0 and the three products, 128 pairs per launch (pointer table in the kernel arguments)
    DisplayImageSumsArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.chan_stride = C == 3 ? chan_stride : HW;
    ia.C = C;
    ia.w = L.w[0];
    ia.h = L.h[0];
    ia.wc = L.w[1];
    ia.hc = L.h[1];
    grad_fill_eotf(ia.e, ia.wgt, eotf, C, h_rgb2y);
    for (int k0 = 0; k0 < n; k0 += DS_MAX_PAIRS) {
        const int nk = (n - k0) < DS_MAX_PAIRS ? (n - k0) : DS_MAX_PAIRS;
        for (int k = 0; k < DS_MAX_PAIRS; ++k) ia.img[k] = k < nk ? static_cast<const float*>(h_img_ptrs[k0 + k]) : nullptr;
        ia.GL0 = ws + L.gl[0] + (size_t)k0 * HW;
        ia.GG1 = ws + L.gg[1] + (size_t)k0 * L.w[1] * L.h[1];
        ia.partial = partial + (size_t)k0 * blocks * DS_SUMS;
        hipLaunchKernelGGL(display_image_sums_kernel, dim3(blocks, nk), dim3(256), 0, st, ia);
        GRAD_HIP_TRY(hipGetLastError());
    }
    GRAD_HIP_TRY(finalize_launch(partial, d_out, n, blocks, st));
    return FVVDP_OK;
}
