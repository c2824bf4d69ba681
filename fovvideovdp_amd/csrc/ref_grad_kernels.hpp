// Backward of the JOD with respect to the REFERENCE (include/fvvdp_hip_ref_grad.h): the layer kernels.  Everything behind
// them -- adj_sweep_kernel, grad_input_kernel, video_level0_kernel, video_input_kernel -- is the test side's, launched on the
// reference's planes.  Instantiated and launched by ref_grad_launch.hip.
//
// The reference enters a band pixel three ways (fvvdp_lpyr_dec.py:246-273, fvvdp.py:392-467, 520-537, 574-596, interp.py:11-59):
// through its own band contrast, as the adaptation luminance L_bkg that divides both contrasts, and through L_bkg as the
// luminance argument of the CSF look-up.  Per band b, temporal channel cc and band pixel, in the notation of grad_kernels.hpp:
//   E  = Expand(G^RS_{b+1})                   (RS: the reference's sustained plane of the same frame)
//   L  = max(E, lbkg_min),  t = layer^T / L,  r = layer^R / L,  T = m_b min(t, cmax),  R = m_b min(r, cmax)
//   s  = S_cc(rho, L, ecc) gain,  T' = T s,  R' = R s,  u = T' - R',  M = k min(|T'|, |R'|),  D = min(|u|^p / (1 + M^q), d_max)
//   w  = c[cc][b] D^(beta-1)                  (0 where c = 0, D = 0 or the d_max clamp binds, as on the test side)
//   A_T = dD/dT',  A_R = dD/dR'               (mirror images; torch.minimum's backward splits a tie)
//   kappa_cc = d log2 S_cc / d log2 L         (the slope plane of the map-writing pyramid pass, band_kernel.hpp)
// and the two maps a pixel writes per channel:
//   GLR_cc = w A_R s m_b / L [r < cmax]                                                       gradient of layer^R_cc
//   GB     = [E > lbkg_min] / L sum_cc w (A_T T' (kappa_cc - [t < cmax]) + A_R R' (kappa_cc - [r < cmax]))    gradient of E beyond the layer's
//   GX_0   = GLR_0 - GB,  GX_1 = GLR_1                                                        what goes back through Expand
// adj_sweep_kernel takes the level's own map (GLR) and the finer level's (GX) as separate pointers:
//   GG_L = GLR_L - Expand^T(GX_{L-1}) + Reduce^T(GG_{L+1}),   g0R = GLR_0 + Reduce^T(GG_1)
// Pointwise on the maps, every band of a batch in one launch, every output a fixed sum per pixel: no atomics.
#pragma once

struct RefBand {
    const float* D;         // [n][2][h][w]  plane cc
    const float* Cn;        // [n][2 CH][h][w]  plane 2cc: test contrast x m_b, plane 2cc + 1: reference
    const float* L;         // [n][h][w]
    const float* S;         // [n][2][h][w]  plane cc: sensitivity before the gain
    const float* K;         // [n][2][h][w]  plane cc: slope kappa
    float* GL;              // [n][CH][h][w] out: GLR (the name grad_fill_layer fills)
    float* GX;              // [n][CH][h][w] out
    int w, h, blk0;         // first workgroup of this band in blockIdx.x
    float m;                // band multiplier
};
struct RefLayerArgs {
    RefBand band[FVVDP_MAX_BANDS];
    const float* coef;      // [n][CH][n_bands]
    int n_bands;
    float p, q[2], k_mask, beta, gain, cmax_hi, dmax_hi, lbkg_min;
};

// One temporal channel of one band pixel: glr = GLR_cc, gb = the channel's term of GB L.  The powers in the forward's
// log2 / exp2 form, as video_layer_one.  s = S gain, m_lb = m / L.
__device__ __forceinline__ void ref_layer_one(float c, float T, float R, float Dm, float s, float kap, float m_lb, float q, float m,
                                              const RefLayerArgs& a, float& glr, float& gb) {
    glr = 0.0f;
    gb = 0.0f;
    // zero: no pooling weight, D == 0 (an identical pixel) or the d_max clamp binds
    if (!(c != 0.0f && Dm > 0.0f && Dm < a.dmax_hi)) return;
    const float Tp = T * s, Rp = R * s;
    const float u = Tp - Rp, au = fabsf(u);
    // the maps hold the contrasts rounded: a difference the rounding collapsed is an identical pixel too (its log below is
    // -inf, and D^(beta-1) = inf times a zero would be NaN).  The rounded products are compared as well: the compiler fuses
    // T s - R s into a multiply-add here, which leaves a rounding residual of the collapsed pair in u instead of a zero
    if (!(au > 0.0f) || Tp == Rp) return;
    const float aT = fabsf(Tp), aR = fabsf(Rp);
    const float M = a.k_mask * fminf(aT, aR);
    const float Mq = M > 0.0f ? fast_exp2(q * fast_log2(M)) : 0.0f;
    const float den = 1.0f + Mq;
    const float lnum = a.p * fast_log2(au);
    const float num = fast_exp2(lnum);
    const float rden = fast_rcp(den);
    const float D = num * rden;
    // the difference term of dD/dT' (dD/dR' has the opposite sign) and the masker term, which goes to the smaller of
    // |T'|, |R'| (ties split, as torch.minimum's backward): mk / |X'| sign(X') is its derivative, mk its product with X'
    const float dif = copysignf(a.p * num * fast_rcp(au), u) * rden;
    const float mk = M > 0.0f ? D * rden * q * Mq : 0.0f;
    const float shT = aT < aR ? 1.0f : (aT == aR ? 0.5f : 0.0f), shR = 1.0f - shT;
    const float Db = fast_exp2((a.beta - 1.0f) * (lnum - fast_log2(den)));      // D^(beta - 1)
    const float w = c * Db;
    const bool t_in = T < m * a.cmax_hi, r_in = R < m * a.cmax_hi;                // the contrast clamp does not bind
    if (r_in) {
        float AR = -dif;
        if (mk > 0.0f && shR > 0.0f) AR -= shR * copysignf(mk * fast_rcp(aR), Rp);
        glr = w * AR * s * m_lb;
    }
    // A_T T' cT + A_R R' cR with cX = kappa - [x < cmax]; A_T T' = dif T' - shT mk, A_R R' = -dif R' - shR mk
    const float cT = kap - (t_in ? 1.0f : 0.0f), cR = kap - (r_in ? 1.0f : 0.0f);
    const float du = cT == cR ? u * cT : Tp * cT - Rp * cR;
    gb = w * (dif * du - mk * (shT * cT + shR * cR));
}

// CH temporal channels of a band pixel per thread (1: a still image, 2: a clip), so that L, the [E > lbkg_min] mask and the
// sum over the channels in GB are formed once
template <int CH>
__global__ __launch_bounds__(256) void ref_layer_kernel(const RefLayerArgs a) {
    int b = 0;
    while (b + 1 < a.n_bands && (int)blockIdx.x >= a.band[b + 1].blk0) ++b;
    const RefBand& B = a.band[b];
    const int k = blockIdx.y;
    const size_t hw = (size_t)B.w * B.h;
    const size_t px = (size_t)((int)blockIdx.x - B.blk0) * 256 + threadIdx.x;
    if (px >= hw) return;
    const float lb = B.L[(size_t)k * hw + px];
    const float rlb = fast_rcp(lb);
    const float m_lb = B.m * rlb;
    float glr[CH], gbs = 0.0f;
#pragma unroll
    for (int cc = 0; cc < CH; ++cc) {
        const float c = a.coef[((size_t)k * CH + cc) * a.n_bands + b];
        const float T = B.Cn[((size_t)k * 2 * CH + 2 * cc) * hw + px];
        const float R = B.Cn[((size_t)k * 2 * CH + 2 * cc + 1) * hw + px];
        const float Dm = B.D[((size_t)k * 2 + cc) * hw + px];
        const float s = B.S[((size_t)k * 2 + cc) * hw + px] * a.gain;
        const float kap = B.K[((size_t)k * 2 + cc) * hw + px];
        float gb;
        ref_layer_one(c, T, R, Dm, s, kap, m_lb, a.q[cc], B.m, a, glr[cc], gb);
        gbs += gb;
    }
    const float GB = lb > a.lbkg_min ? gbs * rlb : 0.0f;
#pragma unroll
    for (int cc = 0; cc < CH; ++cc) {
        B.GL[((size_t)k * CH + cc) * hw + px] = glr[cc];
        B.GX[((size_t)k * CH + cc) * hw + px] = cc == 0 ? glr[cc] - GB : glr[cc];
    }
}
