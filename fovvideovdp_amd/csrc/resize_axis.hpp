// The index arithmetic of one axis of torch.nn.functional.interpolate (align_corners=False, no antialiasing), for every resize of
// the library: the per-frame resize of the integer YUV source class (resize_kernels.hpp: its `area` windows), the clips resized
// inside the ingest, the weights of the resize's adjoint and the host's candidate ranges (resize_clip_kernels.hpp,
// resize_launch.hip).  Host and device code; nothing of HIP is needed: under a plain host compiler RZ_HD is `inline`
// (tests/resize_axis_check.cpp includes this file alone).
//
// Sizes: 1 <= n, n_out <= RZ_MAX_AXIS on every axis -- the entry points refuse anything else.  With that every product of an
// index and a size stays below 2^31 and 32-bit arithmetic is exact.
#pragma once

#include <math.h>

#include "fvvdp_hip.h"                  // FVVDP_RESIZE_NEAREST .. AREA

constexpr int RZ_IDENTITY = 4;          // beside FVVDP_RESIZE_NEAREST .. AREA: the stream has the target's size
constexpr int RZ_MAX_AXIS = 32768;      // the largest width or height of a source or a target

#if defined(__HIPCC__)
#define RZ_HD __host__ __device__ __forceinline__
#else
#define RZ_HD inline
#endif
#if defined(__clang__)
#define RZ_UNROLL _Pragma("unroll")
#else
#define RZ_UNROLL
#endif

// torch's cubic convolution coefficients, A = -0.75 (cubic_coeffs of resize_kernels.hpp, callable from the host as well)
RZ_HD void rz_cubic_coeffs(float t, float (&c)[4]) {
    const float A = -0.75f;
    const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = 2.0f - t;
    c[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    c[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
    c[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    c[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}
// nearest_neighbor_compute_source_index: min(floor(dst * scale), in - 1)
RZ_HD int rz_nearest_axis(int o, int n, float scale) {
    const int i = (int)floorf((float)o * scale);
    return i < n - 1 ? i : n - 1;
}
// area_pixel_compute_source_index(cubic=false) and guard_index_and_lambda: lower index, upper index, weight of the upper one
RZ_HD void rz_bilinear_axis(int o, int n, float scale, int& i0, int& i1, float& l1) {
    const float f = fmaxf(scale * ((float)o + 0.5f) - 0.5f, 0.0f);
    i0 = (int)f;
    if (i0 > n - 1) i0 = n - 1;
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
    l1 = fminf(fmaxf(f - (float)i0, 0.0f), 1.0f);
}
// area_pixel_compute_source_index(cubic=true): the coordinate is not clamped, every tap's index is
RZ_HD void rz_cubic_axis(int o, int n, float scale, int (&idx)[4], float (&c)[4]) {
    const float r = scale * ((float)o + 0.5f) - 0.5f;
    const float fl = floorf(r);
    const int i = (int)fl;
    rz_cubic_coeffs(r - fl, c);
    RZ_UNROLL
    for (int k = 0; k < 4; ++k) {
        const int j = i - 1 + k;
        idx[k] = j < 0 ? 0 : (j > n - 1 ? n - 1 : j);
    }
}
// adaptive average pooling, in integers as ATen has it (AdaptiveAveragePooling.cpp: start_index = (o * in) / out, end_index =
// 1 + ((o + 1) * in - 1) / out).  0 <= a0 < a1 <= n for every o in [0, n_out); the products are below 2^31 (RZ_MAX_AXIS) and not
// negative, so the divisions are unsigned
RZ_HD void rz_area_axis(int o, int n, int n_out, int& a0, int& a1) {
    a0 = (int)((unsigned int)(o * n) / (unsigned int)n_out);
    a1 = 1 + (int)((unsigned int)((o + 1) * n - 1) / (unsigned int)n_out);
}

// the weight target sample o of one axis gives source sample `src` (0: o does not reach it); taps folded onto one index add up
template <int MODE>
RZ_HD float rz_axis_weight(int o, int src, int n, int n_out, float scale) {
    if constexpr (MODE == FVVDP_RESIZE_NEAREST) {
        return rz_nearest_axis(o, n, scale) == src ? 1.0f : 0.0f;
    } else if constexpr (MODE == FVVDP_RESIZE_BILINEAR) {
        int i0, i1;
        float l1;
        rz_bilinear_axis(o, n, scale, i0, i1, l1);
        return (i0 == src ? 1.0f - l1 : 0.0f) + (i1 == src ? l1 : 0.0f);
    } else if constexpr (MODE == FVVDP_RESIZE_BICUBIC) {
        int idx[4];
        float c[4];
        rz_cubic_axis(o, n, scale, idx, c);
        float w = 0.0f;
        RZ_UNROLL
        for (int k = 0; k < 4; ++k) w += idx[k] == src ? c[k] : 0.0f;
        return w;
    } else if constexpr (MODE == FVVDP_RESIZE_AREA) {
        int a0, a1;
        rz_area_axis(o, n, n_out, a0, a1);
        return (src >= a0 && src < a1) ? 1.0f / (float)(a1 - a0) : 0.0f;
    } else {
        return o == src ? 1.0f : 0.0f;
    }
}

// the lowest and highest source index target sample o of one axis reads (host: the candidate ranges of the gather)
template <int MODE>
RZ_HD void rz_axis_reach(int o, int n, int n_out, float scale, int& lo, int& hi) {
    if constexpr (MODE == FVVDP_RESIZE_NEAREST) {
        lo = hi = rz_nearest_axis(o, n, scale);
    } else if constexpr (MODE == FVVDP_RESIZE_BILINEAR) {
        float l1;
        rz_bilinear_axis(o, n, scale, lo, hi, l1);
    } else if constexpr (MODE == FVVDP_RESIZE_BICUBIC) {
        int idx[4];
        float c[4];
        rz_cubic_axis(o, n, scale, idx, c);
        lo = idx[0];
        hi = idx[3];
    } else if constexpr (MODE == FVVDP_RESIZE_AREA) {
        rz_area_axis(o, n, n_out, lo, hi);
        hi -= 1;
    } else {
        lo = hi = o;
    }
}
