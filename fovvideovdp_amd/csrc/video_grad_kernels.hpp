// Backward of the video JOD (include/fvvdp_hip_video_grad.h): the adjoint of fvvdp_temporal_channels + fvvdp_bands_forward +
// fvvdp_pool_jod with respect to the test clip.  Instantiated and launched by video_grad_launch.hip.
//
// Forward, per output frame f and temporal channel cc (fvvdp.py:258-300, 337-357, 395-467, 574-596):
//   X_cc[f] = sum_k taps[cc][k] Lum[idx[f + fl - 1 - k]],  Lum[j] = sum_c w_c EOTF(V_c[j])           (level 0, test plane of cc)
//   pyramid, contrast, masking and spatial pooling per plane as for a still image (grad_kernels.hpp) -> Q[b, cc, f]
//   Q_sc[cc, f] = (sum_b (w_cc Q)^beta_sch)^(1/beta_sch),  Q_tc[f] = (sum_cc Q_sc^beta_tch)^(1/beta_tch),
//   Q = (sum_f Q_tc^beta_t / N)^(1/beta_t),  JOD = sgn(a) (|a|^(1/beta_jod) Q)^beta_jod + 10
// Backward, per batch of n frames:
//   video_coef_kernel    c[f][cc][b] = gamma dJOD/dQ dQ/dQ_tc[f] dQ_tc/dQ_sc[cc] dQ_sc/dQ[b,cc,f] Q^(1-beta) / n_b   (one workgroup)
//   video_layer_kernel   GL_b[f][cc]  = c D^(beta-1) dD/dT' S gain m_b / L_bkg        (both channels of a pixel per thread)
//   adj_sweep_kernel     GG_L = GL_L - Expand^T(GL_{L-1}) + Reduce^T(GG_{L+1})        (grad_kernels.hpp, on the 2n planes)
//   video_level0_kernel  g0[f][cc]    = GL_0 + Reduce^T(GG_1)                          (into the clip-long buffer)
// and once per clip:
//   video_input_kernel   dtest_c[j]   = w_c EOTF'(V_c[j]) sum_{p : idx[p] = j} A[p],  A[p] = sum_cc sum_k taps[cc][k] g0[p-(fl-1)+k][cc]
#pragma once

// ---- coefficients ---------------------------------------------------------------------------------------------------------
struct VideoCoefArgs {
    const float* Q;         // Q_per_ch of the forward, [n_bands][2][N]
    const float* gamma;     // [1] upstream gradient of the JOD
    float* coef;            // [n][2][n_bands]
    int n, n_bands, N, f0;
    float beta, beta_sch, beta_tch, beta_t, w_transient, jod_a, beta_jod;
    float inv_npx[FVVDP_MAX_BANDS];     // 1 / (h_b w_b)
};

// Q_sc of both channels and Q_tc of frame f, as pool_frame (aux_kernels.hpp) in double
__device__ __forceinline__ double video_qtc(const VideoCoefArgs& a, int f, double (&qsc)[2]) {
    double qt = 0.0;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
        const double wc = cc == 1 ? (double)a.w_transient : 1.0;
        double qs = 0.0;
        for (int b = 0; b < a.n_bands; ++b)
            qs += pow(fabs((double)a.Q[((size_t)b * 2 + cc) * a.N + f] * wc), (double)a.beta_sch);
        qsc[cc] = pow(qs, 1.0 / a.beta_sch);
        qt += pow(qsc[cc], (double)a.beta_tch);
    }
    return pow(qt, 1.0 / a.beta_tch);
}

// One workgroup.  First the clip-level norm over all N frames (thread t sums frames t, t + 256, ... in order, then a fixed
// tree: the same value in every batch of the clip), then thread k the coefficients of frame f0 + k.  A factor is zero where
// the norm it divides by is zero (an identical clip or frame), as the reference's norm backward gives.
__global__ __launch_bounds__(256) void video_coef_kernel(const VideoCoefArgs a) {
    __shared__ double s_part[256];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int f = tid; f < a.N; f += 256) {
        double qsc[2];
        acc += pow(video_qtc(a, f, qsc), (double)a.beta_t);
    }
    s_part[tid] = acc;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) s_part[tid] += s_part[tid + o];
        __syncthreads();
    }
    const double q_all = pow(s_part[0] / (double)a.N, 1.0 / a.beta_t);
    double dj = 0.0;                                                                    // gamma dJOD/dQ
    if (q_all > 0.0) {
        const double sgn = a.jod_a < 0.0f ? -1.0 : 1.0;
        const double aq = pow(fabs((double)a.jod_a), 1.0 / a.beta_jod) * q_all;
        dj = (double)a.gamma[0] * sgn * a.beta_jod * pow(aq, (double)a.beta_jod) / q_all;
    }
    for (int k = tid; k < a.n; k += 256) {
        const int f = a.f0 + k;
        double qsc[2];
        const double qtc = video_qtc(a, f, qsc);
        const double gf = (qtc > 0.0 && dj != 0.0) ? dj * pow(qtc / q_all, a.beta_t - 1.0) / (double)a.N : 0.0;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const double wc = cc == 1 ? (double)a.w_transient : 1.0;
            const double gc = (qsc[cc] > 0.0 && gf != 0.0) ? gf * pow(qsc[cc] / qtc, a.beta_tch - 1.0) : 0.0;
            for (int b = 0; b < a.n_bands; ++b) {
                const double qb = fabs((double)a.Q[((size_t)b * 2 + cc) * a.N + f]);
                double c = 0.0;
                if (qb * wc > 0.0 && gc != 0.0)
                    c = gc * wc * pow(qb * wc / qsc[cc], a.beta_sch - 1.0) * pow(qb, 1.0 - a.beta) * a.inv_npx[b];
                a.coef[((size_t)k * 2 + cc) * a.n_bands + b] = (float)c;
            }
        }
    }
}

// ---- layer gradients: pointwise on the maps, every band in one launch, both temporal channels per thread --------------------
struct VideoBand {
    const float* D;         // [n][2][h][w]  plane cc
    const float* Cn;        // [n][4][h][w]  plane 2cc: test contrast x m_b, plane 2cc + 1: reference
    const float* L;         // [n][h][w]
    const float* S;         // [n][2][h][w]  plane cc: sensitivity before the gain
    float* GL;              // [n][2][h][w]  out
    int w, h, blk0;         // first workgroup of this band in blockIdx.x
    float m;                // band multiplier
};
struct VideoLayerArgs {
    VideoBand band[FVVDP_MAX_BANDS];
    const float* coef;      // [n][2][n_bands]
    int n_bands;
    float p, q[2], k_mask, beta, gain, cmax_hi, dmax_hi;
};

// adj_layer_kernel's formula for one temporal channel with the band's pooling coefficient c as the weight: layer_term
// (grad_common.hpp), which the difference map's backward shares with a plane as the weight.
__device__ __forceinline__ float video_layer_one(float c, float T, float R, float Dm, float s, float m_lb, float q, float m,
                                                 const VideoLayerArgs& a) {
    return layer_term<false>(c, T, R, Dm, s, m_lb, q, m, a);
}

__global__ __launch_bounds__(256) void video_layer_kernel(const VideoLayerArgs a) {
    int b = 0;
    while (b + 1 < a.n_bands && (int)blockIdx.x >= a.band[b + 1].blk0) ++b;
    const VideoBand& B = a.band[b];
    const int k = blockIdx.y;
    const size_t hw = (size_t)B.w * B.h;
    const size_t px = (size_t)((int)blockIdx.x - B.blk0) * 256 + threadIdx.x;
    if (px >= hw) return;
    const float m_lb = B.m / B.L[(size_t)k * hw + px];
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
        const float c = a.coef[((size_t)k * 2 + cc) * a.n_bands + b];
        const float T = B.Cn[((size_t)k * 4 + 2 * cc) * hw + px];
        const float R = B.Cn[((size_t)k * 4 + 2 * cc + 1) * hw + px];
        const float Dm = B.D[((size_t)k * 2 + cc) * hw + px];
        const float s = B.S[((size_t)k * 2 + cc) * hw + px] * a.gain;
        B.GL[((size_t)k * 2 + cc) * hw + px] = video_layer_one(c, T, R, Dm, s, m_lb, a.q[cc], B.m, a);
    }
}

// ---- level 0 of the sweep: grad_input_kernel without the display model ------------------------------------------------------
struct VideoLevel0Args {
    const float* GL0;       // [2n][h][w] layer gradient of level 0
    const float* GG1;       // [2n][hc][wc] gradient of G_1
    float* g0;              // [2n][h][w] out: the batch's columns of the clip-long buffer
    int w, h, wc, hc;
};

// grid (ceil(w / 256), h, 2n): the row comes from the block, no division per pixel
__global__ __launch_bounds__(256) void video_level0_kernel(const VideoLevel0Args a) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, k = blockIdx.z;
    if (x >= a.w) return;
    const size_t o = ((size_t)k * a.h + y) * a.w + x;
    a.g0[o] = a.GL0[o] + reduce_t(a.GG1 + (size_t)k * a.wc * a.hc, a.wc, a.hc, a.w, a.h, y, x);
}

// ---- temporal transpose + display model: the mirror image of temporal_vec_kernel ---------------------------------------------
// The transpose of transpose_kernels.hpp (the walk, the ring, the head side buffer and the fold cursor are described there) with
// the display model's derivative as its tail: grad_c[j] = w_c EOTF'(V_c[j]) s[j] (VideoInputArgs is defined there as well).
// FL, PX: see TransposeRing.  ST: the type of the caller's samples and gradient (SRC_F32; SRC_F16 / SRC_BF16: `test` and `grad`
// point at 16-bit samples, PX-sample aligned); g0, head and all arithmetic are fp32 whatever ST.
template <int FL, int PX, int ST>
__device__ __forceinline__ void video_input_body(const VideoInputArgs a) {
    const size_t px = ((size_t)blockIdx.x * 256 + threadIdx.x) * PX;
    if (px >= (size_t)a.t.HW) return;
    TransposeRing<FL, PX> ring = transpose_ring<FL, PX>();
    const size_t HW = (size_t)a.t.HW;
    FoldCursor<PX> fold(a.t.head, HW, px, a.t.fl);
    const int total = a.t.N + a.t.fl - 1;
    for (int p = 0; p < total; ++p) {
        const int j = p - (a.t.fl - 1);         // the frame that is complete after this step
        LaneVec<PX> gs, gt;
        transpose_inputs<PX>(a.t.g0, p, a.t.N, HW, px, gs, gt);
        LaneVec<PX> V[3];                       // the test samples of frame j, requested before the arithmetic
        if (j >= 0) {
            const size_t t = (size_t)j * a.frame_stride + px;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (c < a.C) {
                    if constexpr (ST == SRC_F32) V[c] = lane_load<PX>(a.test + t + (size_t)c * a.chan_stride);
                    else V[c] = lane_load16<PX, ST>(reinterpret_cast<const unsigned short*>(a.test) + t + (size_t)c * a.chan_stride);
                }
        }
        const LaneVec<PX> done = transpose_step<FL, PX>(ring, gs, gt);
        if (p < a.t.fl) lane_store<PX>(a.t.head + (size_t)p * HW + px, done);
        if (j >= 0) {
            const LaneVec<PX> s = fold.frame_sum(j, done);
            const size_t o = (size_t)j * a.frame_stride + px;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c < a.C) {
                    LaneVec<PX> r;
#pragma unroll
                    for (int i = 0; i < PX; ++i) r.v[i] = a.wgt[c] * eotf_grad(V[c].v[i], a.e) * s.v[i];
                    if constexpr (ST == SRC_F32) lane_store<PX>(a.grad + o + (size_t)c * a.chan_stride, r);
                    else lane_store16<PX, ST>(reinterpret_cast<unsigned short*>(a.grad) + o + (size_t)c * a.chan_stride, r);
                }
            }
        }
    }
}

template <int FL, int PX>
__global__ __launch_bounds__(256) void video_input_kernel(const VideoInputArgs a) {
    video_input_body<FL, PX, SRC_F32>(a);
}
// float16 / bfloat16 samples and gradient: an entry point of its own on the same body
template <int FL, int PX, int ST>
__global__ __launch_bounds__(256) void video_input_half_kernel(const VideoInputArgs a) {
    static_assert(src_is_half(ST), "float16 / bfloat16");
    video_input_body<FL, PX, ST>(a);
}
