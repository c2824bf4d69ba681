// Host code that the still-image backward (grad_launch.hip) and the video backward (video_grad_launch.hip) share: the failure
// helper, the workspace layout, the argument checks both entry points make, and the fills of the kernel argument blocks that
// have the same members in both.  No device code.  Include it after temporal_kernels.hpp (EotfDev).
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "grad_common.hpp"     // GradSweepArgs
#include "ingest_host.hpp"     // the display block and the luminance weights
#include "transpose_host.hpp"  // TransposeVerdict

int fvvdp_fail_from(int code, const char* msg);      // fvvdp_hip.hip: sets the message of fvvdp_last_error
// adj_sweep_kernel on `planes` planes of one level.  The kernel is defined in grad_launch.hip only, so is this function
hipError_t grad_sweep_launch(const GradSweepArgs& sa, int planes, hipStream_t st);

static int grad_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static int grad_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return fvvdp_fail_from(code, buf);
}
// the verdict of a check of transpose_host.hpp (host code without the library's message), for GRAD_CHECK
static inline int grad_verdict(const TransposeVerdict& v) { return v.code == FVVDP_OK ? FVVDP_OK : grad_fail(v.code, "%s", v.msg); }

#define GRAD_HIP_TRY(expr)                                                                                  \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) return grad_fail(FVVDP_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));  \
    } while (0)

// returns the code of a grad_check_* that refused
#define GRAD_CHECK(expr)                  \
    do {                                  \
        const int rc_ = (expr);           \
        if (rc_ != FVVDP_OK) return rc_;  \
    } while (0)

// Workspace, in floats, each part 64-float (256 B) aligned; P = planes per batch entry (1: an image pair, 2: a video frame):
//   coef [n][P][n_bands] | GL_b [n][P][h_b][w_b] for b in [0, n_bands) | GG_L [n][P][h_L][w_L] for L in [1, n_bands]
struct GradLayout {
    int w[FVVDP_MAX_BANDS + 1], h[FVVDP_MAX_BANDS + 1];
    size_t coef, gl[FVVDP_MAX_BANDS], gg[FVVDP_MAX_BANDS + 1], total;
};

static size_t align64(size_t x) { return (x + 63) & ~(size_t)63; }

static void grad_layout(int width, int height, int n_bands, int n, int planes, GradLayout& L) {
    L.w[0] = width;
    L.h[0] = height;
    for (int b = 1; b <= n_bands; ++b) {            // ceil(/2), as the context's levels (fvvdp_lpyr_dec.py:198)
        L.w[b] = (L.w[b - 1] + 1) / 2;
        L.h[b] = (L.h[b - 1] + 1) / 2;
    }
    const size_t np = (size_t)n * planes;
    size_t off = 0;
    L.coef = off;
    off += align64(np * n_bands);
    for (int b = 0; b < n_bands; ++b) {
        L.gl[b] = off;
        off += align64(np * L.w[b] * L.h[b]);
    }
    L.gg[0] = 0;
    for (int b = 1; b <= n_bands; ++b) {
        L.gg[b] = off;
        off += align64(np * L.w[b] * L.h[b]);
    }
    L.total = off;
}

// The workspace of the reference's backward (ref_grad_launch.hip, tests_grad_launch.hip): the test side's layout (coef | GLR in
// the place of GL | GG) followed by the GX maps
struct RefGradLayout {
    GradLayout L;
    size_t gx[FVVDP_MAX_BANDS];
};

static void ref_grad_layout(int width, int height, int n_bands, int n, int planes, RefGradLayout& R) {
    grad_layout(width, height, n_bands, n, planes, R.L);
    size_t off = R.L.total;
    for (int b = 0; b < n_bands; ++b) {
        R.gx[b] = off;
        off += align64((size_t)n * planes * R.L.w[b] * R.L.h[b]);
    }
    R.L.total = off;
}

// video_coef_kernel for the n frames [f0, f0 + n) of a clip of n_frames (coefficients [n][2][n_bands] into d_coef) and
// video_level0_kernel on the batch's 2n planes (level 0 of the workspace `ws` into d_g0_batch).  The kernels are defined in
// video_grad_launch.hip only, so are these functions
hipError_t video_coef_launch(const float* d_Q, const float* d_gamma, float* d_coef, int n, int n_bands, int n_frames, int f0,
                             const fvvdp_params* prm, const fvvdp_pool_params* pool, const GradLayout& L, hipStream_t st);
hipError_t video_level0_launch(const float* ws, const GradLayout& L, float* d_g0_batch, int n, hipStream_t st);

// grad_coef_kernel for n pairs (coefficients [n][n_bands] into d_coef) and grad_input_kernel on the n planes of level 0 of the
// workspace `ws`.  The kernels are defined in grad_launch.hip only, so are these functions
hipError_t grad_coef_launch(const float* d_Q, int q_stride, int q_col0, const float* d_gamma, float* d_coef, int n, int n_bands,
                            const fvvdp_params* prm, const fvvdp_pool_params* pool, const GradLayout& L, hipStream_t st);
// dtype: the type of the samples and of the gradient (FVVDP_F32, FVVDP_F16 or FVVDP_BF16; grad_check_sample_type)
hipError_t grad_input_launch(const float* ws, const GradLayout& L, int n, const void* const* h_img_ptrs, void* const* h_grad_ptrs,
                             int dtype, int C, size_t chan_stride, const fvvdp_eotf* eotf, const float* h_rgb2y, hipStream_t st);

// fvvdp_images_grad's launches before its last, in a workspace laid out as L (defined in grad_launch.hip, with adj_layer_kernel),
// and the reference side's counterpart with the size of its workspace in floats (defined in ref_grad_launch.hip, with
// ref_layer_kernel; *layout receives the test side's part of the layout: coefficients, GLR in the place of GL, GG)
int grad_images_sweep(int n_bands, int n, const fvvdp_params* prm, const fvvdp_pool_params* pool, const float* d_Q, int q_stride,
                      int q_col0, const float* d_gamma, const fvvdp_band_maps* maps, float* ws, const GradLayout& L,
                      hipStream_t st);
size_t ref_images_workspace_floats(int width, int height, int n_bands, int n);
int ref_images_sweep(int width, int height, int n_bands, int n, const fvvdp_params* prm, const fvvdp_pool_params* pool,
                     const float* d_Q, int q_stride, int q_col0, const float* d_gamma, const fvvdp_band_maps* maps,
                     const float* const* h_slope_ptrs, float* ws, GradLayout* layout, hipStream_t st);

// `unit`: what n counts in the message ("pairs", "frames"); max_n, max_height: what the caller's launch grids reach
static int grad_check_dims(int width, int height, int n_bands, int n, int max_n, int max_height, const char* unit) {
    if (width < 1 || height < 1 || n < 1 || n > max_n || n_bands < 1 || n_bands > FVVDP_MAX_BANDS || height > max_height)
        return grad_fail(FVVDP_EINVAL, "bad shape %dx%d, %d bands, %d %s", width, height, n_bands, n, unit);
    return FVVDP_OK;
}

static int grad_check_exponents(std::initializer_list<float> exponents) {
    for (float x : exponents)
        if (!(x > 0.0f)) return grad_fail(FVVDP_EINVAL, "pooling exponents must be positive");
    return FVVDP_OK;
}

static int grad_check_maps(const fvvdp_band_maps* maps, int n_bands) {
    for (int b = 0; b < n_bands; ++b)
        if (!maps[b].d_D || !maps[b].d_contrast || !maps[b].d_lbkg || !maps[b].d_S)
            return grad_fail(FVVDP_EINVAL, "band %d: every map (D, contrast, L_bkg, S) is required", b);
    return FVVDP_OK;
}

// the slope planes of the reference's backward: a host array of one device pointer per band
static int check_slopes(const float* const* h_slope_ptrs, int n_bands) {
    if (!h_slope_ptrs) return grad_fail(FVVDP_EINVAL, "null argument");
    for (int b = 0; b < n_bands; ++b)
        if (!h_slope_ptrs[b] || reinterpret_cast<uintptr_t>(h_slope_ptrs[b]) % 4 != 0)
            return grad_fail(FVVDP_EINVAL, "band %d: the slope plane is required, aligned to 4 bytes", b);
    return FVVDP_OK;
}

static int grad_check_workspace(const void* d_work, size_t work_bytes, const GradLayout& L) {
    if (reinterpret_cast<uintptr_t>(d_work) % 256 != 0) return grad_fail(FVVDP_EINVAL, "workspace must be 256-byte aligned");
    if (work_bytes < L.total * sizeof(float))
        return grad_fail(FVVDP_EINVAL, "workspace of %zu bytes is below the %zu needed", work_bytes, L.total * sizeof(float));
    return FVVDP_OK;
}

static int grad_check_channels(int C, const float* h_rgb2y) {
    if (C != 1 && C != 3) return grad_fail(FVVDP_EINVAL, "The content must have either 1 or 3 colour channels.");
    if (C == 3 && !h_rgb2y) return grad_fail(FVVDP_EINVAL, "rgb2y weights required for C == 3");
    return FVVDP_OK;
}

// the sample types the *_st entry points take; *es receives the bytes per sample
static int grad_check_sample_type(int dtype, size_t* es) {
    if (dtype != FVVDP_F32 && dtype != FVVDP_F16 && dtype != FVVDP_BF16)
        return grad_fail(FVVDP_EINVAL, "gradients are written for float32, float16 and bfloat16 samples (dtype %d)", dtype);
    *es = dtype == FVVDP_F32 ? 4 : 2;
    return FVVDP_OK;
}

static int grad_check_closed_form(const fvvdp_eotf* eotf) {
    if (eotf->kind < FVVDP_EOTF_SRGB || eotf->kind > FVVDP_EOTF_ABSOLUTE)
        return grad_fail(FVVDP_EINVAL, "gradients need a closed-form display model (SRGB, GAMMA, PQ, LINEAR or ABSOLUTE)");
    return FVVDP_OK;
}

// The members GradLayerArgs and VideoLayerArgs have in common (a zeroed block; the masking exponents q stay with the caller):
// every band's maps, its layer gradient in the workspace and its range of workgroups.  Returns the workgroups of one plane.
template <class LayerArgs>
static int grad_fill_layer(LayerArgs& la, const fvvdp_band_maps* maps, float* ws, const GradLayout& L, int n_bands,
                           const fvvdp_params* prm) {
    int blocks = 0;
    for (int b = 0; b < n_bands; ++b) {
        auto& B = la.band[b];
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
    la.k_mask = prm->mask_k;
    la.beta = prm->beta;
    la.gain = prm->sens_gain;
    // the maps hold the clamped values, rounded: a value within 2^-20 of a clamp counts as clamped
    la.cmax_hi = prm->contrast_max * (1.0f - 0x1p-20f);
    la.dmax_hi = prm->d_max * (1.0f - 0x1p-20f);
    return blocks;
}

// coarse to fine on `planes` planes per level: G_{n_bands} (base band) ... G_1.  gl_fine: where the map that goes back through
// Expand lives, per band, when it is not the layer gradient itself (the reference's backward: GX, ref_grad_kernels.hpp)
static hipError_t grad_sweep_levels(float* ws, const GradLayout& L, int n_bands, int planes, hipStream_t st,
                                    const size_t* gl_fine = nullptr) {
    if (!gl_fine) gl_fine = L.gl;
    for (int lv = n_bands; lv >= 1; --lv) {
        GradSweepArgs sa;
        sa.GL = lv < n_bands ? ws + L.gl[lv] : nullptr;
        sa.GLf = ws + gl_fine[lv - 1];
        sa.GGc = lv < n_bands ? ws + L.gg[lv + 1] : nullptr;
        sa.GG = ws + L.gg[lv];
        sa.w = L.w[lv];
        sa.h = L.h[lv];
        sa.wf = L.w[lv - 1];
        sa.hf = L.h[lv - 1];
        sa.wc = lv < n_bands ? L.w[lv + 1] : 0;
        sa.hc = lv < n_bands ? L.h[lv + 1] : 0;
        const hipError_t err = grad_sweep_launch(sa, planes, st);
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

// a closed-form display model and the luminance weights of C channels, into a zeroed argument block
static void grad_fill_eotf(EotfDev& e, float (&wgt)[3], const fvvdp_eotf* eotf, int C, const float* h_rgb2y) {
    ingest_fill_display(e, eotf);
    e.lut = nullptr;
    ingest_fill_weights(wgt, C, h_rgb2y);
}
