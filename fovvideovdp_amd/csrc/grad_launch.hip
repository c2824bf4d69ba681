// Gradients of the still-image JOD (include/fvvdp_hip_grad.h): argument checks, workspace layout and launches of the kernels of
// grad_kernels.hpp.  A translation unit of its own: it reads only what the caller passes (the maps of a forward pass with
// maps, the forward's Q_per_ch, the test images), never a context, and changes nothing the forward path compiles.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "fvvdp_hip.h"
#include "fvvdp_hip_grad.h"
#include "device_common.hpp"
#include "temporal_kernels.hpp"
#include "grad_kernels.hpp"

int fvvdp_fail_from(int code, const char* msg);      // fvvdp_hip.hip: sets the message of fvvdp_last_error

static int gfail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static int gfail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return fvvdp_fail_from(code, buf);
}

#define GRAD_HIP_TRY(expr)                                                                               \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return gfail(FVVDP_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

// adj_sweep_kernel on `planes` planes of one level, for the video backward (video_grad_launch.hip): the kernel is defined in
// this translation unit only, so the other one launches it through here
hipError_t grad_sweep_launch(const GradSweepArgs& sa, int planes, hipStream_t st) {
    const size_t hw = (size_t)sa.w * sa.h;
    hipLaunchKernelGGL(adj_sweep_kernel, dim3((unsigned int)((hw + 255) / 256), planes), dim3(256), 0, st, sa);
    return hipGetLastError();
}

// Workspace, in floats, each part 64-float (256 B) aligned:
//   coef [n][n_bands] | GL_b [n][h_b][w_b] for b in [0, n_bands) | GG_L [n][h_L][w_L] for L in [1, n_bands]
struct GradLayout {
    int w[FVVDP_MAX_BANDS + 1], h[FVVDP_MAX_BANDS + 1];
    size_t coef, gl[FVVDP_MAX_BANDS], gg[FVVDP_MAX_BANDS + 1], total;
};

static size_t align64(size_t x) { return (x + 63) & ~(size_t)63; }

static void grad_layout(int width, int height, int n_bands, int n, GradLayout& L) {
    L.w[0] = width;
    L.h[0] = height;
    for (int b = 1; b <= n_bands; ++b) {            // ceil(/2), as the context's levels (fvvdp_lpyr_dec.py:198)
        L.w[b] = (L.w[b - 1] + 1) / 2;
        L.h[b] = (L.h[b - 1] + 1) / 2;
    }
    size_t off = 0;
    L.coef = off;
    off += align64((size_t)n * n_bands);
    for (int b = 0; b < n_bands; ++b) {
        L.gl[b] = off;
        off += align64((size_t)n * L.w[b] * L.h[b]);
    }
    L.gg[0] = 0;
    for (int b = 1; b <= n_bands; ++b) {
        L.gg[b] = off;
        off += align64((size_t)n * L.w[b] * L.h[b]);
    }
    L.total = off;
}

static bool bad_dims(int width, int height, int n_bands, int n) {
    return width < 1 || height < 1 || n < 1 || n_bands < 1 || n_bands > FVVDP_MAX_BANDS;
}

extern "C" int fvvdp_images_grad_workspace(int width, int height, int n_bands, int n, size_t* bytes) {
    if (!bytes) return gfail(FVVDP_EINVAL, "null argument");
    if (bad_dims(width, height, n_bands, n)) return gfail(FVVDP_EINVAL, "bad shape %dx%d, %d bands, %d pairs", width, height, n_bands, n);
    GradLayout L;
    grad_layout(width, height, n_bands, n, L);
    *bytes = L.total * sizeof(float);
    return FVVDP_OK;
}

extern "C" int fvvdp_images_grad(int width, int height, int n_bands, int n, const fvvdp_params* prm,
                                 const fvvdp_pool_params* pool, const float* d_Q, int q_stride, int q_col0, const float* d_gamma,
                                 const fvvdp_band_maps* maps, const void* const* h_test_ptrs, int C, size_t chan_stride,
                                 const fvvdp_eotf* eotf, const float* h_rgb2y, void* const* h_grad_ptrs, void* d_work,
                                 size_t work_bytes, void* stream) {
    if (!prm || !pool || !d_Q || !d_gamma || !maps || !h_test_ptrs || !eotf || !h_grad_ptrs || !d_work)
        return gfail(FVVDP_EINVAL, "null argument");
    if (bad_dims(width, height, n_bands, n)) return gfail(FVVDP_EINVAL, "bad shape %dx%d, %d bands, %d pairs", width, height, n_bands, n);
    if (q_col0 < 0 || q_stride < 1 || q_col0 + n > q_stride) return gfail(FVVDP_EINVAL, "Q columns out of range");
    if (C != 1 && C != 3) return gfail(FVVDP_EINVAL, "The content must have either 1 or 3 colour channels.");
    if (C == 3 && !h_rgb2y) return gfail(FVVDP_EINVAL, "rgb2y weights required for C == 3");
    const size_t HW = (size_t)width * height;
    if (C == 3 && chan_stride < HW) return gfail(FVVDP_EINVAL, "chan_stride %zu is below the image size %zu", chan_stride, HW);
    if (eotf->kind < FVVDP_EOTF_SRGB || eotf->kind > FVVDP_EOTF_ABSOLUTE)
        return gfail(FVVDP_EINVAL, "gradients need a closed-form display model (SRGB, GAMMA, PQ, LINEAR or ABSOLUTE)");
    if (!(pool->beta_sch > 0.0f && pool->beta_tch > 0.0f && pool->beta_jod > 0.0f && prm->beta > 0.0f))
        return gfail(FVVDP_EINVAL, "pooling exponents must be positive");
    for (int b = 0; b < n_bands; ++b)
        if (!maps[b].d_D || !maps[b].d_contrast || !maps[b].d_lbkg || !maps[b].d_S)
            return gfail(FVVDP_EINVAL, "band %d: every map (D, contrast, L_bkg, S) is required", b);
    for (int k = 0; k < n; ++k) {
        if (!h_test_ptrs[k] || !h_grad_ptrs[k]) return gfail(FVVDP_EINVAL, "null image pointer at pair %d", k);
        if ((reinterpret_cast<uintptr_t>(h_test_ptrs[k]) | reinterpret_cast<uintptr_t>(h_grad_ptrs[k])) % 4 != 0)
            return gfail(FVVDP_EINVAL, "image pointers must be aligned to 4 bytes (pair %d)", k);
    }
    if (reinterpret_cast<uintptr_t>(d_work) % 256 != 0) return gfail(FVVDP_EINVAL, "workspace must be 256-byte aligned");
    GradLayout L;
    grad_layout(width, height, n_bands, n, L);
    if (work_bytes < L.total * sizeof(float))
        return gfail(FVVDP_EINVAL, "workspace of %zu bytes is below the %zu needed", work_bytes, L.total * sizeof(float));
    float* ws = static_cast<float*>(d_work);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    // 1. per-band coefficients
    GradCoefArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.Q = d_Q;
    ca.gamma = d_gamma;
    ca.coef = ws + L.coef;
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
    GRAD_HIP_TRY(hipGetLastError());

    // 2. layer gradients of every band
    GradLayerArgs la;
    memset(&la, 0, sizeof(la));
    int blocks = 0;
    for (int b = 0; b < n_bands; ++b) {
        GradBand& B = la.band[b];
        B.D = maps[b].d_D;
        B.Cn = maps[b].d_contrast;
        B.L = maps[b].d_lbkg;
        B.S = maps[b].d_S;
        B.GL = ws + L.gl[b];
        B.w = L.w[b];
        B.h = L.h[b];
        B.blk0 = blocks;
        B.m = b == 0 ? 1.0f : 2.0f;                  // lpyr.get_band (fvvdp_lpyr_dec.py:57-63)
        blocks += (int)(((size_t)L.w[b] * L.h[b] + 255) / 256);
    }
    la.coef = ws + L.coef;
    la.n_bands = n_bands;
    la.p = prm->mask_p;
    la.q = prm->mask_q[0];
    la.k_mask = prm->mask_k;
    la.beta = prm->beta;
    la.gain = prm->sens_gain;
    // the maps hold the clamped values, rounded: a value within 2^-20 of a clamp counts as clamped
    la.cmax_hi = prm->contrast_max * (1.0f - 0x1p-20f);
    la.dmax_hi = prm->d_max * (1.0f - 0x1p-20f);
    hipLaunchKernelGGL(adj_layer_kernel, dim3(blocks, n), dim3(256), 0, st, la);
    GRAD_HIP_TRY(hipGetLastError());

    // 3. coarse to fine: G_{n_bands} (base band) ... G_1
    for (int lv = n_bands; lv >= 1; --lv) {
        GradSweepArgs sa;
        sa.GL = lv < n_bands ? ws + L.gl[lv] : nullptr;
        sa.GLf = ws + L.gl[lv - 1];
        sa.GGc = lv < n_bands ? ws + L.gg[lv + 1] : nullptr;
        sa.GG = ws + L.gg[lv];
        sa.w = L.w[lv];
        sa.h = L.h[lv];
        sa.wf = L.w[lv - 1];
        sa.hf = L.h[lv - 1];
        sa.wc = lv < n_bands ? L.w[lv + 1] : 0;
        sa.hc = lv < n_bands ? L.h[lv + 1] : 0;
        const size_t hw = (size_t)sa.w * sa.h;
        hipLaunchKernelGGL(adj_sweep_kernel, dim3((unsigned int)((hw + 255) / 256), n), dim3(256), 0, st, sa);
        GRAD_HIP_TRY(hipGetLastError());
    }

    // 4. level 0 and the display model, 128 pairs per launch (pointer tables in the kernel arguments)
    GradInputArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.chan_stride = C == 3 ? chan_stride : HW;
    ia.C = C;
    ia.w = width;
    ia.h = height;
    ia.wc = L.w[1];
    ia.hc = L.h[1];
    ia.e.kind = eotf->kind;
    ia.e.scale = eotf->Y_peak - eotf->Y_black;
    ia.e.y_black = eotf->Y_black;
    ia.e.y_peak = eotf->Y_peak;
    ia.e.gamma = eotf->gamma;
    ia.e.l_min = eotf->L_min;
    ia.e.l_max = eotf->L_max;
    ia.e.lut = nullptr;
    if (C == 3) { ia.wgt[0] = h_rgb2y[0]; ia.wgt[1] = h_rgb2y[1]; ia.wgt[2] = h_rgb2y[2]; } else { ia.wgt[0] = 1.0f; }
    for (int k0 = 0; k0 < n; k0 += GRAD_MAX_PAIRS) {
        const int nk = (n - k0) < GRAD_MAX_PAIRS ? (n - k0) : GRAD_MAX_PAIRS;
        for (int k = 0; k < GRAD_MAX_PAIRS; ++k) {
            ia.test[k] = k < nk ? static_cast<const float*>(h_test_ptrs[k0 + k]) : nullptr;
            ia.grad[k] = k < nk ? static_cast<float*>(h_grad_ptrs[k0 + k]) : nullptr;
        }
        ia.GL0 = ws + L.gl[0] + (size_t)k0 * HW;
        ia.GG1 = ws + L.gg[1] + (size_t)k0 * L.w[1] * L.h[1];
        hipLaunchKernelGGL(grad_input_kernel, dim3((unsigned int)((HW + 255) / 256), nk), dim3(256), 0, st, ia);
        GRAD_HIP_TRY(hipGetLastError());
    }
    return FVVDP_OK;
}
