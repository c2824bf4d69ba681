// Gradients of the JOD with respect to the reference (include/fvvdp_hip_ref_grad.h): argument checks, workspace layout and
// launches of ref_layer_kernel (ref_grad_kernels.hpp) and, through grad_launch.hip and video_grad_launch.hip, of the kernels
// the test side's backward already has.  A translation unit of its own: it reads only what the caller passes, never a context
// (fvvdp_ctx_set_slope_maps lives with the context, in fvvdp_hip.hip).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "fvvdp_hip.h"
#include "fvvdp_hip_ref_grad.h"
#include "fvvdp_hip_half.h"
#include "device_common.hpp"
#include "temporal_kernels.hpp"
#include "grad_common.hpp"
#include "ref_grad_kernels.hpp"
#include "grad_host.hpp"

// (RefGradLayout, ref_grad_layout and check_slopes: grad_host.hpp, shared with tests_grad_launch.hip)

// the reference layer gradients of every band (CH channels per thread) and the sweep on the n CH planes
template <int CH>
static int ref_layers_and_sweep(const fvvdp_band_maps* maps, const float* const* h_slope_ptrs, float* ws, const RefGradLayout& R,
                                int n_bands, int n, const fvvdp_params* prm, hipStream_t st) {
    RefLayerArgs la;
    memset(&la, 0, sizeof(la));
    const int blocks = grad_fill_layer(la, maps, ws, R.L, n_bands, prm);
    for (int b = 0; b < n_bands; ++b) {
        la.band[b].K = h_slope_ptrs[b];
        la.band[b].GX = ws + R.gx[b];
    }
    la.q[0] = prm->mask_q[0];
    la.q[1] = prm->mask_q[1];
    la.lbkg_min = prm->lbkg_min;
    hipLaunchKernelGGL((ref_layer_kernel<CH>), dim3(blocks, n), dim3(256), 0, st, la);
    GRAD_HIP_TRY(hipGetLastError());
    GRAD_HIP_TRY(grad_sweep_levels(ws, R.L, n_bands, CH * n, st, R.gx));
    return FVVDP_OK;
}

// The reference side of the still-image sums for the display's gradient (display_grad_launch.hip): the layout of
// fvvdp_images_ref_grad's workspace and its launches down to G_1.  ref_layer_kernel is instantiated here only
size_t ref_images_workspace_floats(int width, int height, int n_bands, int n) {
    RefGradLayout R;
    ref_grad_layout(width, height, n_bands, n, 1, R);
    return R.L.total;
}

int ref_images_sweep(int width, int height, int n_bands, int n, const fvvdp_params* prm, const fvvdp_pool_params* pool,
                     const float* d_Q, int q_stride, int q_col0, const float* d_gamma, const fvvdp_band_maps* maps,
                     const float* const* h_slope_ptrs, float* ws, GradLayout* layout, hipStream_t st) {
    GRAD_CHECK(check_slopes(h_slope_ptrs, n_bands));
    RefGradLayout R;
    ref_grad_layout(width, height, n_bands, n, 1, R);
    GRAD_HIP_TRY(grad_coef_launch(d_Q, q_stride, q_col0, d_gamma, ws + R.L.coef, n, n_bands, prm, pool, R.L, st));
    GRAD_CHECK(ref_layers_and_sweep<1>(maps, h_slope_ptrs, ws, R, n_bands, n, prm, st));
    *layout = R.L;
    return FVVDP_OK;
}

extern "C" int fvvdp_ref_grad_workspace(int width, int height, int n_bands, int n, int planes, size_t* bytes) {
    if (!bytes) return grad_fail(FVVDP_EINVAL, "null argument");
    if (planes != 1 && planes != 2) return grad_fail(FVVDP_EINVAL, "planes must be 1 (image pairs) or 2 (video frames), got %d", planes);
    GRAD_CHECK(grad_check_dims(width, height, n_bands, n, planes == 2 ? 16384 : INT_MAX, planes == 2 ? 65535 : INT_MAX,
                               planes == 2 ? "frames" : "pairs"));
    RefGradLayout R;
    ref_grad_layout(width, height, n_bands, n, planes, R);
    *bytes = R.L.total * sizeof(float);
    return FVVDP_OK;
}

extern "C" int fvvdp_images_ref_grad(int width, int height, int n_bands, int n, const fvvdp_params* prm,
                                     const fvvdp_pool_params* pool, const float* d_Q, int q_stride, int q_col0,
                                     const float* d_gamma, const fvvdp_band_maps* maps, const float* const* h_slope_ptrs,
                                     const void* const* h_ref_ptrs, int C, size_t chan_stride, const fvvdp_eotf* eotf,
                                     const float* h_rgb2y, void* const* h_grad_ptrs, void* d_work, size_t work_bytes,
                                     void* stream) {
    return fvvdp_images_ref_grad_st(width, height, n_bands, n, prm, pool, d_Q, q_stride, q_col0, d_gamma, maps, h_slope_ptrs,
                                    h_ref_ptrs, FVVDP_F32, C, chan_stride, eotf, h_rgb2y, h_grad_ptrs, d_work, work_bytes, stream);
}

extern "C" int fvvdp_images_ref_grad_st(int width, int height, int n_bands, int n, const fvvdp_params* prm,
                                        const fvvdp_pool_params* pool, const float* d_Q, int q_stride, int q_col0,
                                        const float* d_gamma, const fvvdp_band_maps* maps, const float* const* h_slope_ptrs,
                                        const void* const* h_ref_ptrs, int dtype, int C, size_t chan_stride,
                                        const fvvdp_eotf* eotf, const float* h_rgb2y, void* const* h_grad_ptrs, void* d_work,
                                        size_t work_bytes, void* stream) {
    if (!prm || !pool || !d_Q || !d_gamma || !maps || !h_ref_ptrs || !eotf || !h_grad_ptrs || !d_work)
        return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(grad_check_dims(width, height, n_bands, n, INT_MAX, INT_MAX, "pairs"));
    size_t es = 4;
    GRAD_CHECK(grad_check_sample_type(dtype, &es));
    if (q_col0 < 0 || q_stride < 1 || q_col0 + n > q_stride) return grad_fail(FVVDP_EINVAL, "Q columns out of range");
    GRAD_CHECK(grad_check_channels(C, h_rgb2y));
    const size_t HW = (size_t)width * height;
    if (C == 3 && chan_stride < HW) return grad_fail(FVVDP_EINVAL, "chan_stride %zu is below the image size %zu", chan_stride, HW);
    GRAD_CHECK(grad_check_closed_form(eotf));
    GRAD_CHECK(grad_check_exponents({pool->beta_sch, pool->beta_tch, pool->beta_jod, prm->beta}));
    GRAD_CHECK(grad_check_maps(maps, n_bands));
    GRAD_CHECK(check_slopes(h_slope_ptrs, n_bands));
    for (int k = 0; k < n; ++k) {
        if (!h_ref_ptrs[k] || !h_grad_ptrs[k]) return grad_fail(FVVDP_EINVAL, "null image pointer at pair %d", k);
        if ((reinterpret_cast<uintptr_t>(h_ref_ptrs[k]) | reinterpret_cast<uintptr_t>(h_grad_ptrs[k])) % es != 0)
            return grad_fail(FVVDP_EINVAL, "image pointers must be aligned to %zu bytes (pair %d)", es, k);
    }
    RefGradLayout R;
    ref_grad_layout(width, height, n_bands, n, 1, R);
    GRAD_CHECK(grad_check_workspace(d_work, work_bytes, R.L));
    float* ws = static_cast<float*>(d_work);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    GRAD_HIP_TRY(grad_coef_launch(d_Q, q_stride, q_col0, d_gamma, ws + R.L.coef, n, n_bands, prm, pool, R.L, st));
    GRAD_CHECK(ref_layers_and_sweep<1>(maps, h_slope_ptrs, ws, R, n_bands, n, prm, st));
    // level 0 (GLR_0 + Reduce^T(GG_1)) and the display model's derivative at the reference's samples
    GRAD_HIP_TRY(grad_input_launch(ws, R.L, n, h_ref_ptrs, h_grad_ptrs, dtype, C, chan_stride, eotf, h_rgb2y, st));
    return FVVDP_OK;
}

extern "C" int fvvdp_video_ref_grad_frames(int width, int height, int n_bands, int n, const fvvdp_params* prm,
                                           const fvvdp_pool_params* pool, const float* d_Q, int n_frames, int f0,
                                           const float* d_gamma, const fvvdp_band_maps* maps, const float* const* h_slope_ptrs,
                                           float* d_g0, void* d_work, size_t work_bytes, void* stream) {
    if (!prm || !pool || !d_Q || !d_gamma || !maps || !d_g0 || !d_work) return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(grad_check_dims(width, height, n_bands, n, 16384, 65535, "frames"));
    if (n_frames < 1 || f0 < 0 || f0 + n > n_frames)
        return grad_fail(FVVDP_EINVAL, "frames [%d, %d) lie outside the clip of %d frames", f0, f0 + n, n_frames);
    GRAD_CHECK(grad_check_exponents({pool->beta_sch, pool->beta_tch, pool->beta_t, pool->beta_jod, prm->beta}));
    GRAD_CHECK(grad_check_maps(maps, n_bands));
    GRAD_CHECK(check_slopes(h_slope_ptrs, n_bands));
    if (reinterpret_cast<uintptr_t>(d_g0) % 4 != 0) return grad_fail(FVVDP_EINVAL, "d_g0 must be aligned to 4 bytes");
    RefGradLayout R;
    ref_grad_layout(width, height, n_bands, n, 2, R);
    GRAD_CHECK(grad_check_workspace(d_work, work_bytes, R.L));
    float* ws = static_cast<float*>(d_work);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t HW = (size_t)width * height;

    GRAD_HIP_TRY(video_coef_launch(d_Q, d_gamma, ws + R.L.coef, n, n_bands, n_frames, f0, prm, pool, R.L, st));
    GRAD_CHECK(ref_layers_and_sweep<2>(maps, h_slope_ptrs, ws, R, n_bands, n, prm, st));
    // level 0 into the clip-long buffer: video_level0_kernel reads L.gl[0] (GLR_0 here) and L.gg[1]
    GRAD_HIP_TRY(video_level0_launch(ws, R.L, d_g0 + (size_t)f0 * 2 * HW, n, st));
    return FVVDP_OK;
}
