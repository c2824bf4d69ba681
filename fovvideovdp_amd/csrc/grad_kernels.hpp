// Backward of the still-image JOD (include/fvvdp_hip_grad.h): the adjoint of fvvdp_images_channels + fvvdp_images_forward_pool
// with respect to the test image.  Instantiated and launched by grad_launch.hip.
//
// Forward, per pair (fvvdp_lpyr_dec.py:246-273, fvvdp.py:337-357, 395-467, 574-596):
//   G_0 = sum_c w_c EOTF(V_c),  G_{b+1} = Reduce(G_b),  layer_b = G_b - Expand(G_{b+1})
//   T_b = m_b min(layer_b / L_bkg_b, cmax),  T' = T S gain,  D = min(|T'-R'|^p / (1 + (k min(|T'|,|R'|))^q), d_max)
//   Q_b = (mean D^beta)^(1/beta),  JOD = pool(Q_per_ch)
// L_bkg and S come from the reference only (plane 1), so they are constants here.  Backward, per pair:
//   grad_coef_kernel   c[b]      = gamma dJOD/dQ_b Q_b^(1-beta) / n_b                                  (one thread per pair)
//   adj_layer_kernel   GL_b      = c[b] D^(beta-1) dD/dT' S gain m_b / L_bkg     (pointwise on the maps, every band, one launch)
//   adj_sweep_kernel   GG_L      = GL_L - Expand^T(GL_{L-1}) + Reduce^T(GG_{L+1})                 (one launch per level L >= 1)
//   grad_input_kernel  dtest_c   = w_c EOTF'(V_c) (GL_0 + Reduce^T(GG_1))                          (level 0, 128 pairs a launch)
// The transposes are gathers over the exact forward stencils (edge fix-ups and the row-parity quirk of the reduce's last
// column included), so every output is a fixed sum per pixel: no atomics, and a pair's result does not depend on its batch.
#pragma once

#define GRAD_MAX_PAIRS 128      // pointer-table entries of one grad_input_kernel launch (2 x 1 KB of kernel arguments)

#include "grad_common.hpp"     // stencil transposes, GradSweepArgs, eotf_grad: shared with the video backward

// ---- per-band coefficients --------------------------------------------------------------------------------------------
struct GradCoefArgs {
    const float* Q;         // Q_per_ch of the forward, [n_bands][2][q_stride], pair k in column q_col0 + k
    const float* gamma;     // [n] upstream gradient of each JOD
    float* coef;            // [n][n_bands]
    int n, n_bands, q_stride, q_col0;
    float beta, beta_sch, beta_tch, jod_a, beta_jod;
    float inv_npx[FVVDP_MAX_BANDS];     // 1 / (h_b w_b)
};

// JOD = sgn(a) (|a|^(1/beta_jod) Q)^beta_jod + 10, Q = Q_tc of the single frame (beta_t drops out), Q_tc = (Q_sc^beta_tch +
// 0)^(1/beta_tch) (the transient column of an image is 0), Q_sc = (sum_b Q_b^beta_sch)^(1/beta_sch)  (pool_frame, aux_kernels.hpp).
// Zero where Q or Q_b is 0 (an identical pair), as the reference's norm backward gives.  In double: one thread per pair.
__global__ __launch_bounds__(64) void grad_coef_kernel(const GradCoefArgs a) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= a.n) return;
    const int col = a.q_col0 + k;
    double qb[FVVDP_MAX_BANDS];
    double qsc = 0.0;
    for (int b = 0; b < a.n_bands; ++b) {
        qb[b] = fabs((double)a.Q[(size_t)b * 2 * a.q_stride + col]);
        qsc += pow(qb[b], (double)a.beta_sch);
    }
    qsc = pow(qsc, 1.0 / a.beta_sch);
    const double qtc = pow(pow(qsc, (double)a.beta_tch), 1.0 / a.beta_tch);
    double g = 0.0;
    if (qsc > 0.0 && qtc > 0.0) {
        const double sgn = a.jod_a < 0.0f ? -1.0 : 1.0;
        const double aq = pow(fabs((double)a.jod_a), 1.0 / a.beta_jod) * qtc;
        g = (double)a.gamma[k] * sgn * a.beta_jod * pow(aq, (double)a.beta_jod) / qtc;     // dJOD/dQ
        g *= pow(qsc / qtc, a.beta_tch - 1.0);                                              // dQ_tc/dQ_sc
    }
    for (int b = 0; b < a.n_bands; ++b) {
        double c = 0.0;
        if (qb[b] > 0.0 && g != 0.0)
            c = g * pow(qb[b] / qsc, a.beta_sch - 1.0) * pow(qb[b], 1.0 - a.beta) * a.inv_npx[b];
        a.coef[(size_t)k * a.n_bands + b] = (float)c;
    }
}

// ---- layer gradients: pointwise on the maps, every band in one launch ----------------------------------------------------
struct GradBand {
    const float* D;         // [n][2][h][w]  plane 0: sustained (the only channel of an image)
    const float* Cn;        // [n][2][h][w]  plane 0: test contrast x m_b, plane 1: reference
    const float* L;         // [n][h][w]
    const float* S;         // [n][2][h][w]  plane 0: sensitivity before the gain
    float* GL;              // [n][h][w]     out
    int w, h, blk0;         // first workgroup of this band in blockIdx.x
    float m;                // band multiplier
};
struct GradLayerArgs {
    GradBand band[FVVDP_MAX_BANDS];
    const float* coef;      // [n][n_bands]
    int n_bands;
    float p, q, k_mask, beta, gain, cmax_hi, dmax_hi;
};

__global__ __launch_bounds__(256) void adj_layer_kernel(const GradLayerArgs a) {
    int b = 0;
    while (b + 1 < a.n_bands && (int)blockIdx.x >= a.band[b + 1].blk0) ++b;
    const GradBand& B = a.band[b];
    const int k = blockIdx.y;
    const size_t hw = (size_t)B.w * B.h;
    const size_t px = (size_t)((int)blockIdx.x - B.blk0) * 256 + threadIdx.x;
    if (px >= hw) return;
    const float c = a.coef[(size_t)k * a.n_bands + b];
    const float T = B.Cn[(size_t)k * 2 * hw + px];
    const float R = B.Cn[((size_t)k * 2 + 1) * hw + px];
    const float Dm = B.D[(size_t)k * 2 * hw + px];
    float g = 0.0f;
    // zero: no pooling weight, D == 0 (an identical pixel), the d_max clamp or the contrast clamp binds
    if (c != 0.0f && Dm > 0.0f && Dm < a.dmax_hi && T < B.m * a.cmax_hi) {
        const float s = B.S[(size_t)k * 2 * hw + px] * a.gain;
        const float Tp = T * s, Rp = R * s;
        const float u = Tp - Rp, au = fabsf(u);
        // the maps hold the contrasts rounded: a difference the rounding collapsed is an identical pixel too, whatever D the
        // forward stored for it (ref_layer_one, layer_term: the three layer kernels agree on every map).  The rounded products
        // are compared as well: where the compiler fuses T s - R s into a multiply-add, u is a rounding residual, not zero
        if (au > 0.0f && Tp != Rp) {
            const float aT = fabsf(Tp), aR = fabsf(Rp);
            const float M = a.k_mask * fminf(aT, aR);
            const float Mq = M > 0.0f ? powf(M, a.q) : 0.0f;
            const float den = 1.0f + Mq;
            const float num = powf(au, a.p);
            const float D = num / den;
            // dD/dT': the difference term, and the masker term where |T'| is the smaller (ties split, as torch.minimum's backward)
            float dD = copysignf(a.p * num / au, u) / den;
            if (M > 0.0f && aT <= aR) {
                const float share = aT < aR ? 1.0f : 0.5f;
                dD -= share * copysignf(D / den * a.q * Mq / aT, Tp);
            }
            const float lb = B.L[(size_t)k * hw + px];
            g = c * powf(D, a.beta - 1.0f) * dD * s * (B.m / lb);
        }
    }
    B.GL[(size_t)k * hw + px] = g;
}

// ---- coarse-to-fine sweep, one level L >= 1 (GradSweepArgs: grad_common.hpp) ---------------------------------------------
__global__ __launch_bounds__(256) void adj_sweep_kernel(const GradSweepArgs a) {
    const int k = blockIdx.y;
    const size_t hw = (size_t)a.w * a.h;
    const size_t px = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (px >= hw) return;
    const int y = (int)(px / (size_t)a.w), x = (int)(px - (size_t)y * a.w);
    float g = -expand_t(a.GLf + (size_t)k * a.wf * a.hf, a.wf, a.hf, a.w, a.h, y, x);
    if (a.GL) g += a.GL[(size_t)k * hw + px];
    if (a.GGc) g += reduce_t(a.GGc + (size_t)k * a.wc * a.hc, a.wc, a.hc, a.w, a.h, y, x);
    a.GG[(size_t)k * hw + px] = g;
}

// ---- input gradient: level 0 of the sweep and the display model's derivative (eotf_grad: grad_common.hpp) -------------------
struct GradInputArgs {
    const float* test[GRAD_MAX_PAIRS];
    float* grad[GRAD_MAX_PAIRS];
    const float* GL0;       // [n][h][w] layer gradient of level 0, pair 0 of the launch
    const float* GG1;       // [n][hc][wc] gradient of G_1
    size_t chan_stride;
    int C, w, h, wc, hc;
    EotfDev e;
    float wgt[3];
};

// ST: the type of the caller's samples and gradient (SRC_F32; SRC_F16 / SRC_BF16: the pointer tables hold 16-bit samples).  The
// arithmetic is fp32 whatever ST; a 16-bit result is rounded once, to nearest even (float16 subnormals kept).
template <int ST>
__device__ __forceinline__ void grad_input_body(const GradInputArgs& a) {
    const int k = blockIdx.y;
    const size_t hw = (size_t)a.w * a.h;
    const size_t px = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (px >= hw) return;
    const int y = (int)(px / (size_t)a.w), x = (int)(px - (size_t)y * a.w);
    const float g0 = a.GL0[(size_t)k * hw + px] +
                     reduce_t(a.GG1 + (size_t)k * a.wc * a.hc, a.wc, a.hc, a.w, a.h, y, x);
    const float* V = a.test[k];
    float* out = a.grad[k];
    for (int c = 0; c < a.C; ++c) {
        const size_t o = (size_t)c * a.chan_stride + px;
        if constexpr (ST == SRC_F32) {
            out[o] = a.wgt[c] * eotf_grad(V[o], a.e) * g0;
        } else {
            const float v = half_widen<ST>(reinterpret_cast<const unsigned short*>(V)[o]);
            reinterpret_cast<unsigned short*>(out)[o] = half_narrow<ST>(a.wgt[c] * eotf_grad(v, a.e) * g0);
        }
    }
}

__global__ __launch_bounds__(256) void grad_input_kernel(const GradInputArgs a) {
    grad_input_body<SRC_F32>(a);
}
// float16 / bfloat16 samples and gradient: an entry point of its own on the same body
template <int ST>
__global__ __launch_bounds__(256) void grad_input_half_kernel(const GradInputArgs a) {
    static_assert(src_is_half(ST), "float16 / bfloat16");
    grad_input_body<ST>(a);
}
