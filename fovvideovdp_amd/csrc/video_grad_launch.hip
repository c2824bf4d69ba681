// Gradients of the video JOD (include/fvvdp_hip_video_grad.h): argument checks, workspace layout and launches of the kernels
// of video_grad_kernels.hpp (and, through grad_launch.hip, of adj_sweep_kernel).  A translation unit of its own: it reads only
// what the caller passes, never a context, and changes nothing the forward path or the still-image backward compiles.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "fvvdp_hip.h"
#include "fvvdp_hip_video_grad.h"
#include "fvvdp_hip_half.h"
#include "device_common.hpp"
#include "temporal_kernels.hpp"
#include "grad_common.hpp"
#include "transpose_kernels.hpp"
#include "video_grad_kernels.hpp"
#include "grad_host.hpp"

static_assert(FVVDP_VIDEO_GRAD_MAX_TAPS == TRANSPOSE_MAX_FL, "the header states the ring's reach");

// n <= 16384: the 2n planes of a batch are one grid dimension (65535 at most); a context holds 128 frames anyway.
// height <= 65535: the rows of level 0 are another (video_level0_kernel)
static int check_dims(int width, int height, int n_bands, int n) {
    return grad_check_dims(width, height, n_bands, n, 16384, 65535, "frames");
}

hipError_t video_coef_launch(const float* d_Q, const float* d_gamma, float* d_coef, int n, int n_bands, int n_frames, int f0,
                             const fvvdp_params* prm, const fvvdp_pool_params* pool, const GradLayout& L, hipStream_t st) {
    VideoCoefArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.Q = d_Q;
    ca.gamma = d_gamma;
    ca.coef = d_coef;
    ca.n = n;
    ca.n_bands = n_bands;
    ca.N = n_frames;
    ca.f0 = f0;
    ca.beta = prm->beta;
    ca.beta_sch = pool->beta_sch;
    ca.beta_tch = pool->beta_tch;
    ca.beta_t = pool->beta_t;
    ca.w_transient = pool->w_transient;
    ca.jod_a = pool->jod_a;
    ca.beta_jod = pool->beta_jod;
    for (int b = 0; b < n_bands; ++b) ca.inv_npx[b] = (float)(1.0 / ((double)L.w[b] * L.h[b]));
    hipLaunchKernelGGL(video_coef_kernel, dim3(1), dim3(256), 0, st, ca);
    return hipGetLastError();
}

hipError_t video_level0_launch(const float* ws, const GradLayout& L, float* d_g0_batch, int n, hipStream_t st) {
    VideoLevel0Args za;
    za.GL0 = ws + L.gl[0];
    za.GG1 = ws + L.gg[1];
    za.g0 = d_g0_batch;
    za.w = L.w[0];
    za.h = L.h[0];
    za.wc = L.w[1];
    za.hc = L.h[1];
    hipLaunchKernelGGL(video_level0_kernel, dim3((L.w[0] + 255) / 256, L.h[0], 2 * n), dim3(256), 0, st, za);
    return hipGetLastError();
}

extern "C" int fvvdp_video_grad_workspace(int width, int height, int n_bands, int n, size_t* bytes) {
    if (!bytes) return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(check_dims(width, height, n_bands, n));
    GradLayout L;
    grad_layout(width, height, n_bands, n, 2, L);
    *bytes = L.total * sizeof(float);
    return FVVDP_OK;
}

extern "C" int fvvdp_video_grad_frames(int width, int height, int n_bands, int n, const fvvdp_params* prm,
                                       const fvvdp_pool_params* pool, const float* d_Q, int n_frames, int f0,
                                       const float* d_gamma, const fvvdp_band_maps* maps, float* d_g0, void* d_work,
                                       size_t work_bytes, void* stream) {
    if (!prm || !pool || !d_Q || !d_gamma || !maps || !d_g0 || !d_work) return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(check_dims(width, height, n_bands, n));
    if (n_frames < 1 || f0 < 0 || f0 + n > n_frames)
        return grad_fail(FVVDP_EINVAL, "frames [%d, %d) lie outside the clip of %d frames", f0, f0 + n, n_frames);
    GRAD_CHECK(grad_check_exponents({pool->beta_sch, pool->beta_tch, pool->beta_t, pool->beta_jod, prm->beta}));
    GRAD_CHECK(grad_check_maps(maps, n_bands));
    if (reinterpret_cast<uintptr_t>(d_g0) % 4 != 0) return grad_fail(FVVDP_EINVAL, "d_g0 must be aligned to 4 bytes");
    GradLayout L;
    grad_layout(width, height, n_bands, n, 2, L);
    GRAD_CHECK(grad_check_workspace(d_work, work_bytes, L));
    float* ws = static_cast<float*>(d_work);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t HW = (size_t)width * height;

    // 1. coefficients of the batch's frames (the clip-level factor needs every column of Q)
    GRAD_HIP_TRY(video_coef_launch(d_Q, d_gamma, ws + L.coef, n, n_bands, n_frames, f0, prm, pool, L, st));

    // 2. layer gradients of every band, both temporal channels
    VideoLayerArgs la;
    memset(&la, 0, sizeof(la));
    const int blocks = grad_fill_layer(la, maps, ws, L, n_bands, prm);
    la.q[0] = prm->mask_q[0];
    la.q[1] = prm->mask_q[1];
    hipLaunchKernelGGL(video_layer_kernel, dim3(blocks, n), dim3(256), 0, st, la);
    GRAD_HIP_TRY(hipGetLastError());

    // 3. coarse to fine on the 2n planes: G_{n_bands} (base band) ... G_1
    GRAD_HIP_TRY(grad_sweep_levels(ws, L, n_bands, 2 * n, st));

    // 4. level 0 into the clip-long buffer
    GRAD_HIP_TRY(video_level0_launch(ws, L, d_g0 + (size_t)f0 * 2 * HW, n, st));
    return FVVDP_OK;
}

// ST == SRC_F32: video_input_kernel; float16 / bfloat16 samples and gradient: video_input_half_kernel, the same grids and the
// same pixels per lane
template <int FL, int ST>
static void launch_input(const VideoInputArgs& ia, bool vec, hipStream_t st) {
    constexpr int PXV = transpose_px(FL);
    const size_t HW = (size_t)ia.t.HW;
    const dim3 grid((unsigned int)(((vec ? HW / PXV : HW) + 255) / 256)), block(256);
    if constexpr (ST == SRC_F32) {
        if (vec) hipLaunchKernelGGL((video_input_kernel<FL, PXV>), grid, block, 0, st, ia);
        else hipLaunchKernelGGL((video_input_kernel<FL, 1>), grid, block, 0, st, ia);
    } else {
        if (vec) hipLaunchKernelGGL((video_input_half_kernel<FL, PXV, ST>), grid, block, 0, st, ia);
        else hipLaunchKernelGGL((video_input_half_kernel<FL, 1, ST>), grid, block, 0, st, ia);
    }
}

extern "C" int fvvdp_video_grad_input(int width, int height, int n_frames, const float* d_g0, const int32_t* h_fold_frame,
                                      const int32_t* h_fold_pos, const float* h_taps, int fl, const float* d_test, float* d_grad,
                                      int C, size_t chan_stride, size_t frame_stride, const fvvdp_eotf* eotf,
                                      const float* h_rgb2y, float* d_head, size_t head_bytes, void* stream) {
    return fvvdp_video_grad_input_st(width, height, n_frames, d_g0, h_fold_frame, h_fold_pos, h_taps, fl, d_test, d_grad, FVVDP_F32,
                                     C, chan_stride, frame_stride, eotf, h_rgb2y, d_head, head_bytes, stream);
}

extern "C" int fvvdp_video_grad_input_st(int width, int height, int n_frames, const float* d_g0, const int32_t* h_fold_frame,
                                         const int32_t* h_fold_pos, const float* h_taps, int fl, const void* d_test, void* d_grad,
                                         int dtype, int C, size_t chan_stride, size_t frame_stride, const fvvdp_eotf* eotf,
                                         const float* h_rgb2y, float* d_head, size_t head_bytes, void* stream) {
    if (!d_g0 || !h_fold_frame || !h_fold_pos || !h_taps || !d_test || !d_grad || !eotf || !d_head)
        return grad_fail(FVVDP_EINVAL, "null argument");
    if (width < 1 || height < 1 || n_frames < 1) return grad_fail(FVVDP_EINVAL, "bad shape %dx%d, %d frames", width, height, n_frames);
    size_t es = 4;
    GRAD_CHECK(grad_check_sample_type(dtype, &es));
    const size_t HW = (size_t)width * height;
    if (HW > 0x7FFFFFFFu) return grad_fail(FVVDP_EINVAL, "frame of %zu pixels is too large", HW);
    if (fl < 1 || fl > FVVDP_MAX_TAPS) return grad_fail(FVVDP_EINVAL, "filter length %d outside [1, %d]", fl, FVVDP_MAX_TAPS);
    if (fl > FVVDP_VIDEO_GRAD_MAX_TAPS)
        return grad_fail(FVVDP_EUNSUPPORTED, "the video backward covers temporal filters of up to %d taps (256 frames per second); "
                                         "this one has %d", FVVDP_VIDEO_GRAD_MAX_TAPS, fl);
    GRAD_CHECK(grad_check_channels(C, h_rgb2y));
    if (frame_stride < HW) return grad_fail(FVVDP_EINVAL, "frame_stride %zu is below the frame size %zu", frame_stride, HW);
    if (C == 3 && chan_stride < HW) return grad_fail(FVVDP_EINVAL, "chan_stride %zu is below the frame size %zu", chan_stride, HW);
    GRAD_CHECK(grad_check_closed_form(eotf));
    GRAD_CHECK(grad_verdict(transpose_check_fold(h_fold_frame, h_fold_pos, fl, n_frames, "frame")));
    GRAD_CHECK(grad_verdict(transpose_check_head_bytes(head_bytes, fl, HW)));
    // fp32 buffers of the backward, and the caller's samples and gradient (es bytes per sample)
    const uintptr_t ptrs = reinterpret_cast<uintptr_t>(d_g0) | reinterpret_cast<uintptr_t>(d_head);
    const uintptr_t sptrs = reinterpret_cast<uintptr_t>(d_test) | reinterpret_cast<uintptr_t>(d_grad);
    if (ptrs % 4 != 0 || sptrs % es != 0)
        return grad_fail(FVVDP_EINVAL, es == 4 ? "device pointers must be aligned to 4 bytes"
                                               : "device pointers must be aligned to 4 bytes (16-bit samples and gradient: 2 bytes)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    VideoInputArgs ia;
    memset(&ia, 0, sizeof(ia));
    transpose_fill(ia.t, d_g0, d_head, HW, n_frames, fl, h_taps, h_fold_frame, h_fold_pos);
    ia.test = static_cast<const float*>(d_test);       // (16-bit samples: the kernel reads and writes them as such)
    ia.grad = static_cast<float*>(d_grad);
    ia.chan_stride = C == 3 ? chan_stride : 0;
    ia.frame_stride = frame_stride;
    ia.C = C;
    grad_fill_eotf(ia.e, ia.wgt, eotf, C, h_rgb2y);
    const int FL = transpose_ring_length(fl, TRANSPOSE_MAX_FL);
    const bool vec = transpose_vector_ok(FL, HW, frame_stride | ia.chan_stride, ptrs, sptrs, es);
    transpose_dispatch<TRANSPOSE_MAX_FL>(FL, [&](auto c) {
        if (dtype == FVVDP_F16) launch_input<c.value, SRC_F16>(ia, vec, st);
        else if (dtype == FVVDP_BF16) launch_input<c.value, SRC_BF16>(ia, vec, st);
        else launch_input<c.value, SRC_F32>(ia, vec, st);
    });
    GRAD_HIP_TRY(hipGetLastError());
    return FVVDP_OK;
}
