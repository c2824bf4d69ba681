// Gradients of the difference map (include/fvvdp_hip_diffmap.h): argument checks, workspace layout and launches of
// map_level_kernel (map_grad_kernels.hpp), then -- through grad_host.hpp -- the sweep and the level-0 kernels of the JOD's
// backward passes.  A translation unit of its own: it reads only what the caller passes, never a context, and changes nothing
// the forward path or the other backward passes compile.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "fvvdp_hip.h"
#include "fvvdp_hip_diffmap.h"
#include "device_common.hpp"
#include "temporal_kernels.hpp"
#include "grad_common.hpp"
#include "map_grad_kernels.hpp"
#include "grad_host.hpp"

// n and the rows of a level are grid dimensions of map_level_kernel (65535 at most each)
static int check_dims(int width, int height, int n_bands, int n, int channels) {
    if (channels != 1 && channels != 2) return grad_fail(FVVDP_EINVAL, "channels must be 1 (image pairs) or 2 (video frames)");
    return grad_check_dims(width, height, n_bands, n, channels == 2 ? 16384 : 65535, 65535, channels == 2 ? "frames" : "pairs");
}

// the workspace of the JOD's backward (grad_layout on `channels` planes per entry) followed by A_b [n][h_b][w_b], b in [0, n_bands)
struct MapLayout {
    GradLayout g;
    size_t a[FVVDP_MAX_BANDS], total;
};

static void map_layout(int width, int height, int n_bands, int n, int channels, MapLayout& M) {
    grad_layout(width, height, n_bands, n, channels, M.g);
    size_t off = M.g.total;
    for (int b = 0; b < n_bands; ++b) {
        M.a[b] = off;
        off += align64((size_t)n * M.g.w[b] * M.g.h[b]);
    }
    M.total = off;
}

extern "C" int fvvdp_diffmap_grad_workspace(int width, int height, int n_bands, int n, int channels, size_t* h_gl_offsets,
                                            size_t* h_a_offsets, size_t* bytes) {
    if (!bytes) return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(check_dims(width, height, n_bands, n, channels));
    MapLayout M;
    map_layout(width, height, n_bands, n, channels, M);
    *bytes = M.total * sizeof(float);
    for (int b = 0; b < n_bands; ++b) {
        if (h_gl_offsets) h_gl_offsets[b] = M.g.gl[b];
        if (h_a_offsets) h_a_offsets[b] = M.a[b];
    }
    return FVVDP_OK;
}

// what every gradient function checks, and the layout
static int check_common(int width, int height, int n_bands, int n, int channels, const fvvdp_params* prm,
                        const fvvdp_pool_params* pool, int units, const float* d_G, const float* d_v0, const fvvdp_band_maps* maps,
                        const void* d_work, size_t work_bytes, MapLayout& M) {
    if (!prm || !pool || !d_G || !maps || !d_work) return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(check_dims(width, height, n_bands, n, channels));
    if (units != FVVDP_DIFFMAP_JOD && units != FVVDP_DIFFMAP_LINEAR)
        return grad_fail(FVVDP_EINVAL, "units must be FVVDP_DIFFMAP_JOD or FVVDP_DIFFMAP_LINEAR, got %d", units);
    if (units == FVVDP_DIFFMAP_JOD && !d_v0) return grad_fail(FVVDP_EINVAL, "units FVVDP_DIFFMAP_JOD need d_v0");
    if ((reinterpret_cast<uintptr_t>(d_G) | reinterpret_cast<uintptr_t>(d_v0)) % 4 != 0)
        return grad_fail(FVVDP_EINVAL, "d_G and d_v0 must be aligned to 4 bytes");
    if (units == FVVDP_DIFFMAP_JOD) GRAD_CHECK(grad_check_exponents({pool->beta_jod}));
    if (!std::isfinite(pool->w_transient) || !std::isfinite(pool->jod_a))
        return grad_fail(FVVDP_EINVAL, "w_transient and jod_a must be finite");
    GRAD_CHECK(grad_check_maps(maps, n_bands));
    map_layout(width, height, n_bands, n, channels, M);
    if (reinterpret_cast<uintptr_t>(d_work) % 256 != 0) return grad_fail(FVVDP_EINVAL, "workspace must be 256-byte aligned");
    if (work_bytes < M.total * sizeof(float))
        return grad_fail(FVVDP_EINVAL, "workspace of %zu bytes is below the %zu needed", work_bytes, M.total * sizeof(float));
    return FVVDP_OK;
}

// A_b and GL_b of every band, fine to coarse: each launch reads the A of the one before it
static hipError_t map_levels(int n_bands, int n, int channels, const fvvdp_params* prm, const fvvdp_pool_params* pool, int units,
                             const float* d_G, const float* d_v0, const fvvdp_band_maps* maps, float* ws, const MapLayout& M,
                             hipStream_t st) {
    const GradLayout& L = M.g;
    for (int b = 0; b < n_bands; ++b) {
        MapLevelArgs a;
        memset(&a, 0, sizeof(a));
        a.G = d_G;
        a.v0 = units == FVVDP_DIFFMAP_JOD ? d_v0 : nullptr;
        a.Af = b == 0 ? nullptr : ws + M.a[b - 1];
        a.A = ws + M.a[b];
        a.D = maps[b].d_D;
        a.Cn = maps[b].d_contrast;
        a.L = maps[b].d_lbkg;
        a.S = maps[b].d_S;
        a.GL = ws + L.gl[b];
        a.w = L.w[b];
        a.h = L.h[b];
        a.wf = b == 0 ? 0 : L.w[b - 1];
        a.hf = b == 0 ? 0 : L.h[b - 1];
        a.m = b == 0 ? 1.0f : 2.0f;                      // lpyr.get_band / set_band (fvvdp_lpyr_dec.py:57-71)
        a.inv_m = b == 0 ? 1.0f : 0.5f;
        a.w_cc[0] = 1.0f;
        a.w_cc[1] = pool->w_transient;
        a.q[0] = prm->mask_q[0];
        a.q[1] = prm->mask_q[1];
        a.jod_scale = pool->beta_jod * fabsf(pool->jod_a);
        a.jod_exp = pool->beta_jod - 1.0f;
        a.p = prm->mask_p;
        a.k_mask = prm->mask_k;
        a.beta = prm->beta;
        a.gain = prm->sens_gain;
        // the maps hold the clamped values, rounded: a value within 2^-20 of a clamp counts as clamped (grad_fill_layer)
        a.cmax_hi = prm->contrast_max * (1.0f - 0x1p-20f);
        a.dmax_hi = prm->d_max * (1.0f - 0x1p-20f);
        const dim3 grid((a.w + 255) / 256, a.h, n);
        if (channels == 2) hipLaunchKernelGGL(map_level_kernel<2>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(map_level_kernel<1>, grid, dim3(256), 0, st, a);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

extern "C" int fvvdp_diffmap_grad_levels(int width, int height, int n_bands, int n, int channels, const fvvdp_params* prm,
                                         const fvvdp_pool_params* pool, int units, const float* d_G, const float* d_v0,
                                         const fvvdp_band_maps* maps, void* d_work, size_t work_bytes, void* stream) {
    MapLayout M;
    GRAD_CHECK(check_common(width, height, n_bands, n, channels, prm, pool, units, d_G, d_v0, maps, d_work, work_bytes, M));
    GRAD_HIP_TRY(map_levels(n_bands, n, channels, prm, pool, units, d_G, d_v0, maps, static_cast<float*>(d_work), M,
                            reinterpret_cast<hipStream_t>(stream)));
    return FVVDP_OK;
}

extern "C" int fvvdp_diffmap_images_grad(int width, int height, int n_bands, int n, const fvvdp_params* prm,
                                         const fvvdp_pool_params* pool, int units, const float* d_G, const float* d_v0,
                                         const fvvdp_band_maps* maps, const void* const* h_test_ptrs, int dtype, int C,
                                         size_t chan_stride, const fvvdp_eotf* eotf, const float* h_rgb2y, void* const* h_grad_ptrs,
                                         void* d_work, size_t work_bytes, void* stream) {
    if (!h_test_ptrs || !eotf || !h_grad_ptrs) return grad_fail(FVVDP_EINVAL, "null argument");
    MapLayout M;
    GRAD_CHECK(check_common(width, height, n_bands, n, 1, prm, pool, units, d_G, d_v0, maps, d_work, work_bytes, M));
    size_t es = 4;
    GRAD_CHECK(grad_check_sample_type(dtype, &es));
    GRAD_CHECK(grad_check_channels(C, h_rgb2y));
    const size_t HW = (size_t)width * height;
    if (C == 3 && chan_stride < HW) return grad_fail(FVVDP_EINVAL, "chan_stride %zu is below the image size %zu", chan_stride, HW);
    GRAD_CHECK(grad_check_closed_form(eotf));
    for (int k = 0; k < n; ++k) {
        if (!h_test_ptrs[k] || !h_grad_ptrs[k]) return grad_fail(FVVDP_EINVAL, "null image pointer at pair %d", k);
        if ((reinterpret_cast<uintptr_t>(h_test_ptrs[k]) | reinterpret_cast<uintptr_t>(h_grad_ptrs[k])) % es != 0)
            return grad_fail(FVVDP_EINVAL, "image pointers must be aligned to %zu bytes (pair %d)", es, k);
    }
    float* ws = static_cast<float*>(d_work);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    // 1. A_b and the layer gradients, fine to coarse
    GRAD_HIP_TRY(map_levels(n_bands, n, 1, prm, pool, units, d_G, d_v0, maps, ws, M, st));
    // 2. coarse to fine: G_{n_bands} (base band) ... G_1
    GRAD_HIP_TRY(grad_sweep_levels(ws, M.g, n_bands, n, st));
    // 3. level 0 and the display model
    GRAD_HIP_TRY(grad_input_launch(ws, M.g, n, h_test_ptrs, h_grad_ptrs, dtype, C, chan_stride, eotf, h_rgb2y, st));
    return FVVDP_OK;
}

extern "C" int fvvdp_diffmap_video_grad_frames(int width, int height, int n_bands, int n, const fvvdp_params* prm,
                                               const fvvdp_pool_params* pool, int units, const float* d_G, const float* d_v0,
                                               int n_frames, int f0, const fvvdp_band_maps* maps, float* d_g0, void* d_work,
                                               size_t work_bytes, void* stream) {
    if (!d_g0) return grad_fail(FVVDP_EINVAL, "null argument");
    MapLayout M;
    GRAD_CHECK(check_common(width, height, n_bands, n, 2, prm, pool, units, d_G, d_v0, maps, d_work, work_bytes, M));
    if (n_frames < 1 || f0 < 0 || f0 + n > n_frames)
        return grad_fail(FVVDP_EINVAL, "frames [%d, %d) lie outside the clip of %d frames", f0, f0 + n, n_frames);
    if (reinterpret_cast<uintptr_t>(d_g0) % 4 != 0) return grad_fail(FVVDP_EINVAL, "d_g0 must be aligned to 4 bytes");
    float* ws = static_cast<float*>(d_work);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t HW = (size_t)width * height;

    // 1. A_b and the layer gradients of both temporal channels, fine to coarse
    GRAD_HIP_TRY(map_levels(n_bands, n, 2, prm, pool, units, d_G, d_v0, maps, ws, M, st));
    // 2. coarse to fine on the 2n planes
    GRAD_HIP_TRY(grad_sweep_levels(ws, M.g, n_bands, 2 * n, st));
    // 3. level 0 into the clip-long buffer
    GRAD_HIP_TRY(video_level0_launch(ws, M.g, d_g0 + (size_t)f0 * 2 * HW, n, st));
    return FVVDP_OK;
}
