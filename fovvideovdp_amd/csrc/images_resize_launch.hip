// Still images whose stacks have image sizes of their own (include/fvvdp_hip_images_resize.h): the two kernels, their argument
// checks and launches.  A translation unit of its own, as resize_launch.hip: it instantiates the per-pixel functions of
// resize_clip_kernels.hpp (rz_setup, rz_interp, rz_lum) without the register ring, is compiled without contraction of multiplies
// and adds for the reason given there -- the two stacks are two copies of scalar code, and fvvdp_resize_grad recomputes a stack's
// values to decide the clip as this ingest decided it -- and asks fvvdp_hip.hip for the context's side of the ingest
// (fvvdp_ctx_ingest_begin), grad_launch.hip and ref_grad_launch.hip for the still-image backward's launches before its last.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "fvvdp_hip.h"
#include "fvvdp_hip_images_resize.h"
#include "device_common.hpp"
#include "temporal_launch.hpp"     // fvvdp_ctx_ingest_begin
#include "grad_common.hpp"
#include "resize_clip_kernels.hpp"
#include "grad_host.hpp"

static_assert(FVVDP_RESIZE_MAX_AXIS == RZ_MAX_AXIS, "resize_axis.hpp");

// ---- ingest ----------------------------------------------------------------------------------------------------------------------
struct StillResizedArgs {
    RzStream src[2];        // test, reference; image k of a stack is its frame k
    int Wo, Ho;
    EotfDev e;
    float w[3];
    L0Addr out;             // level 0 of a still-image context: slot k of the launch at l0_frame(out, k), [HW][2] floats
};

// The per-pixel body of resized_ring_kernel without the ring.  grid (ceil(Ho Wo / (256 PX)), n): one thread owns PX target pixels
// 256 apart of pair blockIdx.y, sets up each stack's taps once per pixel and stores {L_test, L_ref}.  A stack of the target's size
// takes the identity variant (a wave-uniform branch per stack).
template <int PX, int MODE>
__global__ __launch_bounds__(256) void still_resized_kernel(const StillResizedArgs a) {
    const int HW = a.Wo * a.Ho;
    const int k = blockIdx.y;
    OobMax bad;                     // never set: every value is clipped before the display model
    float* o = l0_frame(a.out, k);
#pragma unroll
    for (int i = 0; i < PX; ++i) {
        const int q = blockIdx.x * (256 * PX) + i * 256 + threadIdx.x;
        if (q >= HW) continue;
        const int oy = q / a.Wo, ox = q - oy * a.Wo;
        float L[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const size_t base = (size_t)k * a.src[s].fs;
            if (a.src[s].identity) {
                RzTaps<RZ_IDENTITY> ti;
                ti.off = q;                                                     // (an identity stack has the target's size)
                L[s] = rz_lum<RZ_IDENTITY>(a.src[s], base, ti, a.e, a.w, bad);
            } else {
                RzTaps<MODE> t;
                rz_setup<MODE>(t, a.src[s], oy, ox, a.Wo, a.Ho);
                L[s] = rz_lum<MODE>(a.src[s], base, t, a.e, a.w, bad);
            }
        }
        *reinterpret_cast<float2*>(o + (size_t)q * 2) = make_float2(L[0], L[1]);
    }
}

// ---- level 0 of the still-image sweep: grad_input_kernel without the display model ----------------------------------------------
struct ImagesLevel0Args {
    const float* GL0;       // [n][h][w] layer gradient of level 0
    const float* GG1;       // [n][hc][wc] gradient of G_1
    float* gL;              // [n][h][w] out, dense
    int w, h, wc, hc;
};

// grid (ceil(h w / 256), n): one thread per target pixel and pair, every output written once
__global__ __launch_bounds__(256) void images_level0_kernel(const ImagesLevel0Args a) {
    const int k = blockIdx.y;
    const size_t hw = (size_t)a.w * a.h;
    const size_t px = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (px >= hw) return;
    const int y = (int)(px / (size_t)a.w), x = (int)(px - (size_t)y * a.w);
    a.gL[(size_t)k * hw + px] = a.GL0[(size_t)k * hw + px] + reduce_t(a.GG1 + (size_t)k * a.wc * a.hc, a.wc, a.hc, a.w, a.h, y, x);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// (the checks of resize_launch.hip, in its words)
static int check_mode(int mode) {
    if (mode < FVVDP_RESIZE_NEAREST || mode > FVVDP_RESIZE_AREA) return grad_fail(FVVDP_EINVAL, "unknown resize mode %d", mode);
    return FVVDP_OK;
}

static int check_axes(int width, int height, const char* what) {
    if (width > RZ_MAX_AXIS || height > RZ_MAX_AXIS)
        return grad_fail(FVVDP_EINVAL, "frame size out of range (1..%d per axis): %dx%d (%s)", RZ_MAX_AXIS, width, height, what);
    return FVVDP_OK;
}

static int check_stream(const fvvdp_resize_stream* s, const char* what) {
    if (!s->d_data) return grad_fail(FVVDP_EINVAL, "null data pointer (%s)", what);
    if (s->dtype != FVVDP_F32 && s->dtype != FVVDP_U8)
        return grad_fail(FVVDP_EINVAL, "the %s must be float32 or uint8 (dtype %d)", what, s->dtype);
    if (s->dtype == FVVDP_F32 && reinterpret_cast<uintptr_t>(s->d_data) % 4 != 0)
        return grad_fail(FVVDP_EINVAL, "data pointer must be aligned to 4 bytes (%s)", what);
    if (s->channels != 1 && s->channels != 3) return grad_fail(FVVDP_EINVAL, "The content must have either 1 or 3 colour channels.");
    if (s->width < 1 || s->height < 1) return grad_fail(FVVDP_EINVAL, "bad frame size %dx%d (%s)", s->width, s->height, what);
    GRAD_CHECK(check_axes(s->width, s->height, what));
    const size_t hw = (size_t)s->width * s->height;
    if (s->plane_stride < hw) return grad_fail(FVVDP_EINVAL, "plane_stride %zu is below the plane size %zu (%s)", s->plane_stride, hw, what);
    if (s->frame_stride < hw) return grad_fail(FVVDP_EINVAL, "frame_stride %zu is below the plane size %zu (%s)", s->frame_stride, hw, what);
    return FVVDP_OK;
}

static RzStream dev_stream(const fvvdp_resize_stream* s, int Wo, int Ho) {
    RzStream r;
    memset(&r, 0, sizeof(r));
    r.p = s->d_data;
    r.u8 = s->dtype == FVVDP_U8 ? 1 : 0;
    r.C = s->channels;
    r.W = s->width;
    r.H = s->height;
    r.identity = (s->width == Wo && s->height == Ho) ? 1 : 0;
    r.fs = s->frame_stride;
    r.ps = s->plane_stride;
    r.sx = (float)s->width / (float)Wo;
    r.sy = (float)s->height / (float)Ho;
    return r;
}

// pixels per lane: two for the modes with few taps, as the short rings of the clip kernel; bicubic (16 indices and 8 coefficients
// per stack and pixel) and area (a loop over its window per pixel) keep one
template <int MODE>
static void launch_still(const StillResizedArgs& a, int n, hipStream_t st) {
    constexpr int PX = MODE <= FVVDP_RESIZE_BILINEAR ? 2 : 1;
    const size_t HW = (size_t)a.Wo * a.Ho;
    const dim3 grid((unsigned int)((HW + 256 * PX - 1) / (256 * PX)), (unsigned int)n), block(256);
    hipLaunchKernelGGL((still_resized_kernel<PX, MODE>), grid, block, 0, st, a);
}

extern "C" int fvvdp_images_channels_resized(fvvdp_ctx* ctx, const fvvdp_resize_stream* test, const fvvdp_resize_stream* ref, int n,
                                             int mode, const fvvdp_eotf* eotf, const float* h_rgb2y, int slot0, void* stream) {
    if (!ctx || !test || !ref || !eotf || !h_rgb2y) return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(check_mode(mode));
    if (eotf->kind < FVVDP_EOTF_SRGB || eotf->kind > FVVDP_EOTF_ABSOLUTE)
        return grad_fail(FVVDP_EINVAL, "resized sources need a closed-form display model (samples are fractional after the resize)");
    GRAD_CHECK(check_stream(test, "test"));
    GRAD_CHECK(check_stream(ref, "reference"));
    if (test->channels != ref->channels)
        return grad_fail(FVVDP_EINVAL, "test and reference differ in their channel counts (%d and %d)", test->channels, ref->channels);
    // (the context's frame size is the target of the resize; one tap of 1 per channel, as fvvdp_images_channels)
    static const float taps[2] = {1.0f, 1.0f};
    IngestBegin b;
    GRAD_CHECK(fvvdp_ctx_ingest_begin(ctx, nullptr, false, test->channels, eotf, h_rgb2y, taps, 1, n, slot0, &b));
    if (b.planes != 2) return grad_fail(FVVDP_EINVAL, "fvvdp_images_channels_resized needs a still-image context (planes == 2)");
    GRAD_CHECK(check_axes(b.W, b.H, "target"));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    StillResizedArgs a;
    memset(&a, 0, sizeof(a));
    a.src[0] = dev_stream(test, b.W, b.H);
    a.src[1] = dev_stream(ref, b.W, b.H);
    a.Wo = b.W;
    a.Ho = b.H;
    grad_fill_eotf(a.e, a.w, eotf, test->channels, h_rgb2y);
    const L0Addr out0 = b.out;
    for (int k0 = 0; k0 < n; k0 += 65535) {                     // (grid axis y)
        const int nk = (n - k0) < 65535 ? (n - k0) : 65535;
        a.out = out0;
        a.out.slot0 = out0.slot0 + k0;
        a.src[0].p = static_cast<const char*>(test->d_data) + (size_t)k0 * test->frame_stride * (test->dtype == FVVDP_U8 ? 1 : 4);
        a.src[1].p = static_cast<const char*>(ref->d_data) + (size_t)k0 * ref->frame_stride * (ref->dtype == FVVDP_U8 ? 1 : 4);
        switch (mode) {
            case FVVDP_RESIZE_NEAREST: launch_still<FVVDP_RESIZE_NEAREST>(a, nk, st); break;
            case FVVDP_RESIZE_BILINEAR: launch_still<FVVDP_RESIZE_BILINEAR>(a, nk, st); break;
            case FVVDP_RESIZE_BICUBIC: launch_still<FVVDP_RESIZE_BICUBIC>(a, nk, st); break;
            default: launch_still<FVVDP_RESIZE_AREA>(a, nk, st); break;
        }
        GRAD_HIP_TRY(hipGetLastError());
    }
    return FVVDP_OK;
}

static int check_dims(int width, int height, int n_bands, int n) {
    return grad_check_dims(width, height, n_bands, n, INT_MAX, INT_MAX, "pairs");
}

extern "C" int fvvdp_images_grad_luminance_workspace(int width, int height, int n_bands, int n, int reference, size_t* bytes) {
    if (!bytes) return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(check_dims(width, height, n_bands, n));
    if (reference) {
        *bytes = ref_images_workspace_floats(width, height, n_bands, n) * sizeof(float);
    } else {
        GradLayout L;
        grad_layout(width, height, n_bands, n, 1, L);
        *bytes = L.total * sizeof(float);
    }
    return FVVDP_OK;
}

extern "C" int fvvdp_images_grad_luminance(int width, int height, int n_bands, int n, const fvvdp_params* prm,
                                           const fvvdp_pool_params* pool, const float* d_Q, int q_stride, int q_col0,
                                           const float* d_gamma, const fvvdp_band_maps* maps, const float* const* h_slope_ptrs,
                                           float* d_gL, void* d_work, size_t work_bytes, void* stream) {
    if (!prm || !pool || !d_Q || !d_gamma || !maps || !d_gL || !d_work) return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(check_dims(width, height, n_bands, n));
    if (q_col0 < 0 || q_stride < 1 || q_col0 + n > q_stride) return grad_fail(FVVDP_EINVAL, "Q columns out of range");
    GRAD_CHECK(grad_check_exponents({pool->beta_sch, pool->beta_tch, pool->beta_jod, prm->beta}));
    GRAD_CHECK(grad_check_maps(maps, n_bands));
    if (reinterpret_cast<uintptr_t>(d_gL) % 4 != 0) return grad_fail(FVVDP_EINVAL, "d_gL must be aligned to 4 bytes");
    const bool reference = h_slope_ptrs != nullptr;
    GradLayout L;
    grad_layout(width, height, n_bands, n, 1, L);
    if (reference) {
        GRAD_CHECK(check_slopes(h_slope_ptrs, n_bands));
        L.total = ref_images_workspace_floats(width, height, n_bands, n);
    }
    GRAD_CHECK(grad_check_workspace(d_work, work_bytes, L));
    float* ws = static_cast<float*>(d_work);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    // coefficients, layer kernel, sweep down to G_1: the gradient entry point's launches before its last
    if (reference) {
        GRAD_CHECK(ref_images_sweep(width, height, n_bands, n, prm, pool, d_Q, q_stride, q_col0, d_gamma, maps, h_slope_ptrs, ws, &L, st));
    } else {
        GRAD_CHECK(grad_images_sweep(n_bands, n, prm, pool, d_Q, q_stride, q_col0, d_gamma, maps, ws, L, st));
    }

    // level 0 (GL_0, or GLR_0 in its place, + Reduce^T(GG_1)), dense
    const size_t HW = (size_t)width * height;
    ImagesLevel0Args la;
    la.w = L.w[0];
    la.h = L.h[0];
    la.wc = L.w[1];
    la.hc = L.h[1];
    for (int k0 = 0; k0 < n; k0 += 65535) {                     // (grid axis y)
        const int nk = (n - k0) < 65535 ? (n - k0) : 65535;
        la.GL0 = ws + L.gl[0] + (size_t)k0 * HW;
        la.GG1 = ws + L.gg[1] + (size_t)k0 * L.w[1] * L.h[1];
        la.gL = d_gL + (size_t)k0 * HW;
        hipLaunchKernelGGL(images_level0_kernel, dim3((unsigned int)((HW + 255) / 256), (unsigned int)nk), dim3(256), 0, st, la);
        GRAD_HIP_TRY(hipGetLastError());
    }
    return FVVDP_OK;
}
