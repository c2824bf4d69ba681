// Gradients of the still-image JOD (include/fvvdp_hip_grad.h): argument checks, workspace layout and launches of the kernels of
// grad_kernels.hpp.  A translation unit of its own: it reads only what the caller passes (the maps of a forward pass with
// maps, the forward's Q_per_ch, the test images), never a context, and changes nothing the forward path compiles.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "fvvdp_hip.h"
#include "fvvdp_hip_grad.h"
#include "fvvdp_hip_half.h"
#include "device_common.hpp"
#include "temporal_kernels.hpp"
#include "grad_kernels.hpp"
#include "grad_host.hpp"

// adj_sweep_kernel is defined in this translation unit only: both backward passes launch it through here (grad_host.hpp)
hipError_t grad_sweep_launch(const GradSweepArgs& sa, int planes, hipStream_t st) {
    const size_t hw = (size_t)sa.w * sa.h;
    hipLaunchKernelGGL(adj_sweep_kernel, dim3((unsigned int)((hw + 255) / 256), planes), dim3(256), 0, st, sa);
    return hipGetLastError();
}

// grad_coef_kernel and grad_input_kernel are defined here only as well: the backward with respect to the reference
// (ref_grad_launch.hip) launches them through these two functions
hipError_t grad_coef_launch(const float* d_Q, int q_stride, int q_col0, const float* d_gamma, float* d_coef, int n, int n_bands,
                            const fvvdp_params* prm, const fvvdp_pool_params* pool, const GradLayout& L, hipStream_t st) {
    GradCoefArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.Q = d_Q;
    ca.gamma = d_gamma;
    ca.coef = d_coef;
    ca.n = n;
    ca.n_bands = n_bands;
    ca.q_stride = q_stride;
    ca.q_col0 = q_col0;
    ca.beta = prm->beta;
    ca.beta_sch = pool->beta_sch;
    ca.beta_tch = pool->beta_tch;
    ca.jod_a = pool->jod_a;
    ca.beta_jod = pool->beta_jod;
    for (int b = 0; b < n_bands; ++b) ca.inv_npx[b] = (float)(1.0 / ((double)L.w[b] * L.h[b]));
    hipLaunchKernelGGL(grad_coef_kernel, dim3((n + 63) / 64), dim3(64), 0, st, ca);
    return hipGetLastError();
}

// level 0 of the sweep (ws + L.gl[0], ws + L.gg[1]) and the display model's derivative at the samples `h_img_ptrs`
hipError_t grad_input_launch(const float* ws, const GradLayout& L, int n, const void* const* h_img_ptrs, void* const* h_grad_ptrs,
                             int dtype, int C, size_t chan_stride, const fvvdp_eotf* eotf, const float* h_rgb2y, hipStream_t st) {
    const size_t HW = (size_t)L.w[0] * L.h[0];
    GradInputArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.chan_stride = C == 3 ? chan_stride : HW;
    ia.C = C;
    ia.w = L.w[0];
    ia.h = L.h[0];
    ia.wc = L.w[1];
    ia.hc = L.h[1];
    grad_fill_eotf(ia.e, ia.wgt, eotf, C, h_rgb2y);
    for (int k0 = 0; k0 < n; k0 += GRAD_MAX_PAIRS) {
        const int nk = (n - k0) < GRAD_MAX_PAIRS ? (n - k0) : GRAD_MAX_PAIRS;
        for (int k = 0; k < GRAD_MAX_PAIRS; ++k) {
            ia.test[k] = k < nk ? static_cast<const float*>(h_img_ptrs[k0 + k]) : nullptr;
            ia.grad[k] = k < nk ? static_cast<float*>(h_grad_ptrs[k0 + k]) : nullptr;
        }
        ia.GL0 = ws + L.gl[0] + (size_t)k0 * HW;
        ia.GG1 = ws + L.gg[1] + (size_t)k0 * L.w[1] * L.h[1];
        const dim3 grid((unsigned int)((HW + 255) / 256), nk);
        if (dtype == FVVDP_F16) hipLaunchKernelGGL(grad_input_half_kernel<SRC_F16>, grid, dim3(256), 0, st, ia);
        else if (dtype == FVVDP_BF16) hipLaunchKernelGGL(grad_input_half_kernel<SRC_BF16>, grid, dim3(256), 0, st, ia);
        else hipLaunchKernelGGL(grad_input_kernel, grid, dim3(256), 0, st, ia);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

// Steps 1 to 3 of fvvdp_images_grad in the workspace `ws` laid out as L: the per-band coefficients, the layer gradients of every
// band and the sweep from the base band down to G_1.  adj_layer_kernel is defined here only: the sums for the display's gradient
// (display_grad_launch.hip) make the same launches through this function
int grad_images_sweep(int n_bands, int n, const fvvdp_params* prm, const fvvdp_pool_params* pool, const float* d_Q, int q_stride,
                      int q_col0, const float* d_gamma, const fvvdp_band_maps* maps, float* ws, const GradLayout& L,
                      hipStream_t st) {
    // 1. per-band coefficients
    GRAD_HIP_TRY(grad_coef_launch(d_Q, q_stride, q_col0, d_gamma, ws + L.coef, n, n_bands, prm, pool, L, st));

    // 2. layer gradients of every band
    GradLayerArgs la;
    memset(&la, 0, sizeof(la));
    const int blocks = grad_fill_layer(la, maps, ws, L, n_bands, prm);
    la.q = prm->mask_q[0];
    hipLaunchKernelGGL(adj_layer_kernel, dim3(blocks, n), dim3(256), 0, st, la);
    GRAD_HIP_TRY(hipGetLastError());

    // 3. coarse to fine: G_{n_bands} (base band) ... G_1
    GRAD_HIP_TRY(grad_sweep_levels(ws, L, n_bands, n, st));
    return FVVDP_OK;
}

// an image pair is one plane of the workspace; n is a grid dimension of its own, so the shape has no limit beyond int
static int check_dims(int width, int height, int n_bands, int n) {
    return grad_check_dims(width, height, n_bands, n, INT_MAX, INT_MAX, "pairs");
}

extern "C" int fvvdp_images_grad_workspace(int width, int height, int n_bands, int n, size_t* bytes) {
    if (!bytes) return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(check_dims(width, height, n_bands, n));
    GradLayout L;
    grad_layout(width, height, n_bands, n, 1, L);
    *bytes = L.total * sizeof(float);
    return FVVDP_OK;
}

extern "C" int fvvdp_images_grad(int width, int height, int n_bands, int n, const fvvdp_params* prm,
                                 const fvvdp_pool_params* pool, const float* d_Q, int q_stride, int q_col0, const float* d_gamma,
                                 const fvvdp_band_maps* maps, const void* const* h_test_ptrs, int C, size_t chan_stride,
                                 const fvvdp_eotf* eotf, const float* h_rgb2y, void* const* h_grad_ptrs, void* d_work,
                                 size_t work_bytes, void* stream) {
    return fvvdp_images_grad_st(width, height, n_bands, n, prm, pool, d_Q, q_stride, q_col0, d_gamma, maps, h_test_ptrs, FVVDP_F32,
                                C, chan_stride, eotf, h_rgb2y, h_grad_ptrs, d_work, work_bytes, stream);
}

extern "C" int fvvdp_images_grad_st(int width, int height, int n_bands, int n, const fvvdp_params* prm,
                                    const fvvdp_pool_params* pool, const float* d_Q, int q_stride, int q_col0, const float* d_gamma,
                                    const fvvdp_band_maps* maps, const void* const* h_test_ptrs, int dtype, int C,
                                    size_t chan_stride, const fvvdp_eotf* eotf, const float* h_rgb2y, void* const* h_grad_ptrs,
                                    void* d_work, size_t work_bytes, void* stream) {
    if (!prm || !pool || !d_Q || !d_gamma || !maps || !h_test_ptrs || !eotf || !h_grad_ptrs || !d_work)
        return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(check_dims(width, height, n_bands, n));
    size_t es = 4;
    GRAD_CHECK(grad_check_sample_type(dtype, &es));
    if (q_col0 < 0 || q_stride < 1 || q_col0 + n > q_stride) return grad_fail(FVVDP_EINVAL, "Q columns out of range");
    GRAD_CHECK(grad_check_channels(C, h_rgb2y));
    const size_t HW = (size_t)width * height;
    if (C == 3 && chan_stride < HW) return grad_fail(FVVDP_EINVAL, "chan_stride %zu is below the image size %zu", chan_stride, HW);
    GRAD_CHECK(grad_check_closed_form(eotf));
    GRAD_CHECK(grad_check_exponents({pool->beta_sch, pool->beta_tch, pool->beta_jod, prm->beta}));
    GRAD_CHECK(grad_check_maps(maps, n_bands));
    for (int k = 0; k < n; ++k) {
        if (!h_test_ptrs[k] || !h_grad_ptrs[k]) return grad_fail(FVVDP_EINVAL, "null image pointer at pair %d", k);
        if ((reinterpret_cast<uintptr_t>(h_test_ptrs[k]) | reinterpret_cast<uintptr_t>(h_grad_ptrs[k])) % es != 0)
            return grad_fail(FVVDP_EINVAL, "image pointers must be aligned to %zu bytes (pair %d)", es, k);
    }
    GradLayout L;
    grad_layout(width, height, n_bands, n, 1, L);
    GRAD_CHECK(grad_check_workspace(d_work, work_bytes, L));
    float* ws = static_cast<float*>(d_work);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    // 1. - 3. coefficients, layer gradients, sweep down to G_1
    GRAD_CHECK(grad_images_sweep(n_bands, n, prm, pool, d_Q, q_stride, q_col0, d_gamma, maps, ws, L, st));

    // 4. level 0 and the display model, 128 pairs per launch (pointer tables in the kernel arguments)
    GRAD_HIP_TRY(grad_input_launch(ws, L, n, h_test_ptrs, h_grad_ptrs, dtype, C, chan_stride, eotf, h_rgb2y, st));
    return FVVDP_OK;
}
