// Gradients of the video JOD under many gazes (include/fvvdp_hip_gaze_grad.h): argument checks, workspace layout and launches
// of gaze_layer_kernel (gaze_grad_kernels.hpp) and, through video_grad_launch.hip and grad_launch.hip, of video_coef_kernel,
// adj_sweep_kernel and video_level0_kernel.  A translation unit of its own: it reads only what the caller passes, never a
// context, and changes nothing the forward path or the other backward passes compile.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "fvvdp_hip.h"
#include "fvvdp_hip_gaze.h"
#include "fvvdp_hip_gaze_grad.h"
#include "device_common.hpp"
#include "temporal_kernels.hpp"
#include "grad_common.hpp"
#include "gaze_grad_kernels.hpp"
#include "grad_host.hpp"
#include "pyramid_host.hpp"

// the limits of fvvdp_video_grad_frames: the 2n planes of a batch and the rows of level 0 are grid dimensions
static int check_dims(int width, int height, int n_bands, int n, int n_gazes) {
    GRAD_CHECK(grad_check_dims(width, height, n_bands, n, 16384, 65535, "frames"));
    if (n_gazes < 1) return grad_fail(FVVDP_EINVAL, "n_gazes must be at least 1, got %d", n_gazes);
    return FVVDP_OK;
}

// floats of one gaze's coefficients [n][2][n_bands], 256-byte aligned; they follow the single-gaze layout
static size_t coef_floats(int n, int n_bands) { return align64((size_t)n * 2 * n_bands); }

extern "C" int fvvdp_gaze_grad_workspace(int width, int height, int n_bands, int n, int n_gazes, size_t* bytes) {
    if (!bytes) return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(check_dims(width, height, n_bands, n, n_gazes));
    GradLayout L;
    grad_layout(width, height, n_bands, n, 2, L);
    *bytes = (L.total + (size_t)n_gazes * coef_floats(n, n_bands)) * sizeof(float);
    return FVVDP_OK;
}

template <int NG>
static void launch_layer(const GazeLayerArgs& la, int blocks, int n, hipStream_t st) {
    hipLaunchKernelGGL((gaze_layer_kernel<NG>), dim3(blocks, n), dim3(256), 0, st, la);
}

extern "C" int fvvdp_gaze_grad_frames(int width, int height, int n_bands, int n, int n_gazes, int group_max,
                                      const fvvdp_params* prm, const fvvdp_pool_params* pool, const fvvdp_geom* geom,
                                      const double* h_rho_band,
                                      const float* d_S_log0, const float* d_S_log1, const float* d_axes, const float* h_axes,
                                      const float* d_gaze, size_t gaze_stride, const float* d_Q, int n_frames, int f0,
                                      const float* d_gamma, const fvvdp_band_maps* maps, float* d_g0, void* d_work,
                                      size_t work_bytes, void* stream) {
    if (!prm || !pool || !geom || !h_rho_band || !d_gaze || !d_Q || !d_gamma || !maps || !d_g0 || !d_work)
        return grad_fail(FVVDP_EINVAL, "null argument");
    if (!d_S_log0 || !d_S_log1 || !d_axes || !h_axes) return grad_fail(FVVDP_EINVAL, "null CSF table or axis");
    GRAD_CHECK(check_dims(width, height, n_bands, n, n_gazes));
    if (group_max != 0 && group_max != 1 && group_max != 2 && group_max != 4 && group_max != FVVDP_GAZE_GROUP_MAX)
        return grad_fail(FVVDP_EINVAL, "group_max must be 0 (the default, %d), 1, 2, 4 or %d, got %d", FVVDP_GAZE_GROUP_MAX,
                         FVVDP_GAZE_GROUP_MAX, group_max);
    if (n_frames < 1 || f0 < 0 || f0 + n > n_frames)
        return grad_fail(FVVDP_EINVAL, "frames [%d, %d) lie outside the clip of %d frames", f0, f0 + n, n_frames);
    if (gaze_stride < (size_t)2 * n)
        return grad_fail(FVVDP_EINVAL, "gaze_stride %zu is below the %d floats of a batch of %d frames", gaze_stride, 2 * n, n);
    if (!(geom->display_size_m[0] > 0.0f) || !(geom->display_size_m[1] > 0.0f) || !(geom->distance_m > 0.0f) ||
        !(geom->ppd_centre > 0.0f))
        return grad_fail(FVVDP_EINVAL, "display geometry must be positive");
    GRAD_CHECK(grad_check_exponents({pool->beta_sch, pool->beta_tch, pool->beta_t, pool->beta_jod, prm->beta}));
    GRAD_CHECK(grad_check_maps(maps, n_bands));
    for (int ax = 0; ax < 3; ++ax)
        if (!(h_axes[ax * FVVDP_LUT_N + FVVDP_LUT_N - 1] > h_axes[ax * FVVDP_LUT_N]))
            return grad_fail(FVVDP_EINVAL, "axis %d of the CSF tables must be ascending", ax);
    const uintptr_t ptrs = reinterpret_cast<uintptr_t>(d_g0) | reinterpret_cast<uintptr_t>(d_S_log0) |
                           reinterpret_cast<uintptr_t>(d_S_log1) | reinterpret_cast<uintptr_t>(d_axes) |
                           reinterpret_cast<uintptr_t>(d_gaze) | reinterpret_cast<uintptr_t>(d_Q) |
                           reinterpret_cast<uintptr_t>(d_gamma);
    if (ptrs % 4 != 0) return grad_fail(FVVDP_EINVAL, "device pointers must be aligned to 4 bytes");
    GradLayout L;
    grad_layout(width, height, n_bands, n, 2, L);
    const size_t csz = coef_floats(n, n_bands);
    GradLayout need = L;                             // the single-gaze layout, then the coefficients of every gaze
    need.total = L.total + (size_t)n_gazes * csz;
    GRAD_CHECK(grad_check_workspace(d_work, work_bytes, need));
    float* ws = static_cast<float*>(d_work);
    float* coef = ws + L.total;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t HW = (size_t)width * height;

    // 1. coefficients of the batch's frames, per gaze: its Q_per_ch, its upstream gradient
    const size_t q_gaze = (size_t)n_bands * 2 * n_frames;
    for (int g = 0; g < n_gazes; ++g)
        GRAD_HIP_TRY(video_coef_launch(d_Q + g * q_gaze, d_gamma + g, coef + g * csz, n, n_bands, n_frames, f0, prm, pool, L, st));

    // 2. layer gradients of every band, summed over the gazes: one launch per group of gazes
    GazeLayerArgs la;
    memset(&la, 0, sizeof(la));
    int blocks = 0;
    for (int b = 0; b < n_bands; ++b) {
        GazeBand& B = la.band[b];
        B.Cn = maps[b].d_contrast;
        B.L = maps[b].d_lbkg;
        B.GL = ws + L.gl[b];
        B.w = L.w[b];
        B.h = L.h[b];
        B.blk0 = blocks;
        B.m = b == 0 ? 1.0f : 2.0f;                  // lpyr.get_band (fvvdp_lpyr_dec.py:57-63)
        B.rho_band = (float)h_rho_band[b];
        B.kx = geom->display_size_m[0] / (float)L.w[b] / geom->distance_m;     // as band_item forms them
        B.kyb = geom->display_size_m[1] / (float)L.h[b] / geom->distance_m;
        blocks += (int)(((size_t)L.w[b] * L.h[b] + 255) / 256);
    }
    la.lut0 = d_S_log0;
    la.lut1 = d_S_log1;
    la.axes = d_axes;
    la.coef_stride = (long long)csz;
    la.gaze_stride = (long long)gaze_stride;
    la.n_bands = n_bands;
    la.frame_w = width;
    la.frame_h = height;
    la.p = prm->mask_p;
    la.q[0] = prm->mask_q[0];
    la.q[1] = prm->mask_q[1];
    la.k_mask = prm->mask_k;
    la.beta = prm->beta;
    la.gain = prm->sens_gain;
    la.cmax_hi = prm->contrast_max * (1.0f - 0x1p-20f);     // as grad_fill_layer
    la.dmax_hi = prm->d_max * (1.0f - 0x1p-20f);
    la.size_m0 = geom->display_size_m[0];
    la.size_m1 = geom->display_size_m[1];
    la.dist_m = geom->distance_m;
    {   // the constants the forward's kernels take (fill_band_args, fvvdp_ctx_set_csf_3d in fvvdp_hip.hip)
        const FovAxes fx = fov_axes(h_axes, geom);
        la.delta_rad = fx.delta_rad;
        la.cos_delta = fx.cos_delta;
        // log2f of the float that exp2f of the knot rounds to, not the knot itself: the value the forward forms from its y_lo / y_hi
        la.ly_lo = log2f(fx.y_lo);
        la.ly_hi = log2f(fx.y_hi);
        la.rho_lo = fx.rho_lo;
        la.rho_hi = fx.rho_hi;
        la.ecc_lo = fx.ecc_lo;
        la.ecc_hi = fx.ecc_hi;
        for (int ax = 0; ax < 3; ++ax) {
            la.first[ax] = fx.first[ax];
            la.inv_step[ax] = fx.inv_step[ax];
        }
    }
    const int cap = group_max ? group_max : FVVDP_GAZE_GROUP_MAX;      // smaller groups, more launches: same bits (tests, A/B runs)
    for (int g = 0; g < n_gazes;) {
        int ng = FVVDP_GAZE_GROUP_MAX;               // the largest instantiation that the gazes left fill: 8, 4, 2, 1
        while (ng > cap || ng > n_gazes - g) ng >>= 1;
        la.coef = coef + (size_t)g * csz;
        la.gaze = d_gaze + (size_t)g * gaze_stride;
        la.accumulate = g > 0 ? 1 : 0;
        switch (ng) {
            case 8: launch_layer<8>(la, blocks, n, st); break;
            case 4: launch_layer<4>(la, blocks, n, st); break;
            case 2: launch_layer<2>(la, blocks, n, st); break;
            default: launch_layer<1>(la, blocks, n, st); break;
        }
        GRAD_HIP_TRY(hipGetLastError());
        g += ng;
    }

    // 3. coarse to fine on the 2n planes, 4. level 0 into the clip-long buffer: once, whatever the number of gazes
    GRAD_HIP_TRY(grad_sweep_levels(ws, L, n_bands, 2 * n, st));
    GRAD_HIP_TRY(video_level0_launch(ws, L, d_g0 + (size_t)f0 * 2 * HW, n, st));
    return FVVDP_OK;
}
