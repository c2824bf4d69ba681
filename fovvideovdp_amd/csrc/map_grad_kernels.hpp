// Backward of the difference map (include/fvvdp_hip_diffmap.h): the transpose of the heat-map reconstruction joined to a layer
// gradient whose weight is a plane.  Instantiated and launched by map_grad_launch.hip.
//
// Forward, per pair or frame (heat_level_kernel, aux_kernels.hpp; fvvdp_lpyr_dec.py:65-71, 94-101; fvvdp.py:469-473):
//   v_b = Expand(v_{b+1}) + (D_b[0] + w_transient D_b[1]) / m_b        (m_0 = 1, m_b = 2; the coarsest band has no coarse term;
//                                                                        a still image has channel 0 only)
//   map = v_0^beta_jod |jod_a|  (units "jod"),   map = v_0  (units "linear")
// Backward for a cotangent G of the map, one launch of map_level_kernel per level, fine to coarse:
//   A_0     = G beta_jod |jod_a| v_0^(beta_jod - 1)  ("jod"; 0 where v_0 == 0),   A_0 = G  ("linear")
//   A_b     = Expand^T(A_{b-1})                                          (expand_t, grad_common.hpp: the exact transposed gather)
//   GL_b[cc] = (A_b w_cc / m_b) dD/dT' S gain m_b / L_bkg                (w_0 = 1, w_1 = w_transient)
// GL_b is adj_layer_kernel's / video_layer_one's formula with the per-pixel weight A_b w_cc / m_b in the place of
// c D^(beta - 1): layer_term (grad_common.hpp) is the one copy of it.  The sweep and level 0 that follow are the existing
// kernels on the workspace of grad_layout.  Every output is a fixed sum per pixel: no atomics, and an entry's result does not
// depend on the batch it ran in.
#pragma once

#include "grad_common.hpp"

struct MapLevelArgs {
    const float* G;         // [n][h][w] cotangent of the map (level 0 only)
    const float* v0;        // [n][h][w] pre-power reconstruction (level 0, units "jod"; nullptr: units "linear")
    const float* Af;        // [n][hf][wf] A of the next finer level (nullptr at level 0)
    float* A;               // [n][h][w] out
    const float* D;         // [n][2][h][w]     plane cc
    const float* Cn;        // [n][2 NC][h][w]  plane 2cc: test contrast x m_b, plane 2cc + 1: reference
    const float* L;         // [n][h][w]
    const float* S;         // [n][2][h][w]     plane cc: sensitivity before the gain
    float* GL;              // [n][NC][h][w] out
    int w, h, wf, hf;
    float m, inv_m;         // band multiplier and 1 / m
    float w_cc[2];          // {1, w_transient}
    float q[2];
    float jod_scale, jod_exp;       // beta_jod |jod_a|, beta_jod - 1
    float p, k_mask, beta, gain, cmax_hi, dmax_hi;
};

// NC: temporal channels (1: a still image, 2: a video frame).  grid (ceil(w / 256), h, n): the row comes from the block, no
// division per pixel (as video_level0_kernel).
template <int NC>
__global__ __launch_bounds__(256) void map_level_kernel(const MapLevelArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, k = blockIdx.z;
    if (x >= a.w) return;
    const size_t hw = (size_t)a.w * a.h;
    const size_t o = (size_t)y * a.w + x;
    float A;
    if (a.Af) {
        A = expand_t(a.Af + (size_t)k * a.wf * a.hf, a.wf, a.hf, a.w, a.h, y, x);
    } else {
        A = a.G[(size_t)k * hw + o];
        if (a.v0) {
            const float v = a.v0[(size_t)k * hw + o];
            A = v > 0.0f ? A * a.jod_scale * powf(v, a.jod_exp) : 0.0f;      // an identical pair: 0, not inf * 0
        }
    }
    a.A[(size_t)k * hw + o] = A;
    const float m_lb = a.m / a.L[(size_t)k * hw + o];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) {
        const float T = a.Cn[((size_t)k * 2 * NC + 2 * cc) * hw + o];
        const float R = a.Cn[((size_t)k * 2 * NC + 2 * cc + 1) * hw + o];
        const float Dm = a.D[((size_t)k * 2 + cc) * hw + o];
        const float s = a.S[((size_t)k * 2 + cc) * hw + o] * a.gain;
        a.GL[((size_t)k * NC + cc) * hw + o] = layer_term<true>(A * a.w_cc[cc] * a.inv_m, T, R, Dm, s, m_lb, a.q[cc], a.m, a);
    }
}
