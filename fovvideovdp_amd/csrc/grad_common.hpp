// Device functions and argument blocks that the still-image backward (grad_kernels.hpp, grad_launch.hip) and the video
// backward (video_grad_kernels.hpp, video_grad_launch.hip) share: the transposes of the pyramid's reduce / expand stencils, the
// arguments of adj_sweep_kernel and the display model's derivative -- for the sample (eotf_grad) and, for the sums of
// display_grad_kernels.hpp, for the display's own parameters (eotf_display_sens).  No kernel is defined here: the four kernels of
// grad_kernels.hpp stay in the one translation unit that compiles them.
#pragma once

// the 5-tap kernel of the pyramid (fvvdp_lpyr_dec.py:174-178, kernel_a = 0.4)
__device__ __forceinline__ float pyr_k(int k) {
    return (k == 0 || k == 4) ? 0.05f : (k == 2 ? 0.4f : 0.25f);
}

// Weight of fine sample j in coarse sample r of one axis of gausspyr_reduce (fvvdp_lpyr_dec.py:183-207): the zero-padded
// stride-2 5-tap filter plus the edge fix-ups.  n: fine size, nr: coarse size, odd_fix: the last fix-up's parity -- the
// row count of the fine level on BOTH axes (the reference tests x.shape[-2] for the columns too).
__device__ __forceinline__ float reduce_w(int r, int j, int n, int nr, bool odd_fix) {
    const int k = j - 2 * r + 2;
    float w = (k >= 0 && k <= 4) ? pyr_k(k) : 0.0f;
    if (r == 0) w += (j == 0 ? pyr_k(1) : 0.0f) + (j == 1 ? pyr_k(0) : 0.0f);
    if (r == nr - 1) {
        if (odd_fix) w += (j == n - 1 ? pyr_k(3) : 0.0f) + (j == n - 2 ? pyr_k(4) : 0.0f);
        else w += (j == n - 1 ? pyr_k(4) : 0.0f);
    }
    return w;
}

// Weight of coarse sample j in fine sample i of one axis of gausspyr_expand (fvvdp_lpyr_dec.py:126-142, 219-235; closed form
// of oracle _expand_axis): even i = 2c -> 2K0 x[c-1] + 2K2 x[c] + 2K4 x[c+1], odd i -> 2K1 x[c] + 2K3 x[c+1], indices
// clamped to [0, n).  n: coarse size.
__device__ __forceinline__ float expand_w(int i, int j, int n) {
    const int c = i >> 1, cm = max(c - 1, 0), cp = min(c + 1, n - 1);
    if ((i & 1) == 0)
        return (cm == j ? 2.0f * pyr_k(0) : 0.0f) + (c == j ? 2.0f * pyr_k(2) : 0.0f) + (cp == j ? 2.0f * pyr_k(4) : 0.0f);
    return (c == j ? 2.0f * pyr_k(1) : 0.0f) + (cp == j ? 2.0f * pyr_k(3) : 0.0f);
}

// Reduce^T of the coarse image G [hc][wc] at fine pixel (y, x) of a w x h level: the coarse samples whose stencil reads it
// (at most 3 per axis: r in [y/2 - 1, y/2 + 1])
__device__ __forceinline__ float reduce_t(const float* G, int wc, int hc, int w, int h, int y, int x) {
    const bool odd = (h & 1) != 0;
    float wy[3], wx[3];
    const int ry0 = (y >> 1) - 1, rx0 = (x >> 1) - 1;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int ry = ry0 + d, rx = rx0 + d;
        wy[d] = (ry >= 0 && ry < hc) ? reduce_w(ry, y, h, hc, odd) : 0.0f;
        wx[d] = (rx >= 0 && rx < wc) ? reduce_w(rx, x, w, wc, odd) : 0.0f;
    }
    float s = 0.0f;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        if (wy[dy] == 0.0f) continue;
        const float* row = G + (size_t)(ry0 + dy) * wc;
        float t = 0.0f;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
            if (wx[dx] != 0.0f) t = fmaf(wx[dx], row[rx0 + dx], t);
        s = fmaf(wy[dy], t, s);
    }
    return s;
}

// Expand^T of the fine image Y [hf][wf] at coarse pixel (y, x) of a wc x hc level: the fine samples whose stencil reads it
// (i in [2y - 2, 2y + 2] per axis; 2y + 3 never does, see expand_w)
__device__ __forceinline__ float expand_t(const float* Y, int wf, int hf, int wc, int hc, int y, int x) {
    float wy[5], wx[5];
    const int iy0 = 2 * y - 2, ix0 = 2 * x - 2;
#pragma unroll
    for (int d = 0; d < 5; ++d) {
        const int iy = iy0 + d, ix = ix0 + d;
        wy[d] = (iy >= 0 && iy < hf) ? expand_w(iy, y, hc) : 0.0f;
        wx[d] = (ix >= 0 && ix < wf) ? expand_w(ix, x, wc) : 0.0f;
    }
    float s = 0.0f;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
        if (wy[dy] == 0.0f) continue;
        const float* row = Y + (size_t)(iy0 + dy) * wf;
        float t = 0.0f;
#pragma unroll
        for (int dx = 0; dx < 5; ++dx)
            if (wx[dx] != 0.0f) t = fmaf(wx[dx], row[ix0 + dx], t);
        s = fmaf(wy[dy], t, s);
    }
    return s;
}

// ---- layer gradient of one band pixel and temporal channel ------------------------------------------------------------------
// adj_layer_kernel's formula (grad_kernels.hpp), the powers in the forward's log2 / exp2 form (band_kernel.hpp): three
// transcendental pairs per value instead of three powf.  s = S gain; s * m_lb = S gain m / L_bkg is d(T')/d(layer).  `a`: any
// argument block with p, k_mask, beta, cmax_hi and dmax_hi (grad_fill_layer's members).
//   PLANE_WEIGHT false: c is the band's pooling coefficient and the value is c D^(beta - 1) dD/dT' s m_lb (video_layer_one);
//   PLANE_WEIGHT true:  c is a per-pixel weight that stands in the place of c D^(beta - 1) (map_level_kernel).
template <bool PLANE_WEIGHT, class Args>
__device__ __forceinline__ float layer_term(float c, float T, float R, float Dm, float s, float m_lb, float q, float m,
                                            const Args& a) {
    // zero: no weight, D == 0 (an identical pixel), the d_max clamp or the contrast clamp binds
    if (!(c != 0.0f && Dm > 0.0f && Dm < a.dmax_hi && T < m * a.cmax_hi)) return 0.0f;
    const float Tp = T * s, Rp = R * s;
    const float u = Tp - Rp, au = fabsf(u);
    // The maps hold the contrasts rounded, and the forward forms D from the unrounded difference in the log2 domain
    // (band_kernel.hpp): two contrasts an ulp apart can collapse in T s - R s here while the stored D is tiny and positive.
    // Such a pixel is an identical pixel, as in ref_layer_one (its log below is -inf, and D^(beta-1) = inf times a zero is NaN).
    // The rounded products are compared as well: where the compiler fuses T s - R s into a multiply-add, u is a rounding
    // residual of the collapsed pair, not zero
    if (!(au > 0.0f) || Tp == Rp) return 0.0f;
    const float aT = fabsf(Tp), aR = fabsf(Rp);
    const float M = a.k_mask * fminf(aT, aR);
    const float Mq = M > 0.0f ? fast_exp2(q * fast_log2(M)) : 0.0f;
    const float den = 1.0f + Mq;
    const float lnum = a.p * fast_log2(au);
    const float num = fast_exp2(lnum);
    const float rden = fast_rcp(den);
    const float D = num * rden;
    // dD/dT': the difference term, and the masker term where |T'| is the smaller (ties split, as torch.minimum's backward)
    float dD = copysignf(a.p * num * fast_rcp(au), u) * rden;
    if (M > 0.0f && aT <= aR) {
        const float share = aT < aR ? 1.0f : 0.5f;
        dD -= share * copysignf(D * rden * q * Mq * fast_rcp(aT), Tp);
    }
    if constexpr (PLANE_WEIGHT) {
        return c * dD * s * m_lb;
    } else {
        const float Db = fast_exp2((a.beta - 1.0f) * (lnum - fast_log2(den)));      // D^(beta - 1)
        return c * Db * dD * s * m_lb;
    }
}

// ---- coarse-to-fine sweep, one level L >= 1 (adj_sweep_kernel, grad_kernels.hpp) -------------------------------------------
struct GradSweepArgs {
    const float* GL;        // [n][h][w] layer gradient of level L (nullptr: L is the base band, no layer of its own)
    const float* GLf;       // [n][hf][wf] layer gradient of level L - 1
    const float* GGc;       // [n][hc][wc] gradient of G_{L+1} (nullptr for the base band)
    float* GG;              // [n][h][w] out: gradient of G_L
    int w, h, wf, hf, wc, hc;
};

// dL/dV of eotf_one (temporal_kernels.hpp) with the reference's clamps: 0 where V lies outside [0, 1] for SRGB / GAMMA / PQ
// (fvvdp_display_model.py:147-150) and where the luminance clip of PQ, LINEAR or ABSOLUTE binds; sRGB takes the branch the
// forward takes (V > 0.04045).
__device__ __forceinline__ float eotf_grad(float V, const EotfDev& e) {
    switch (e.kind) {
        case FVVDP_EOTF_SRGB:
            if (!(V >= 0.0f && V <= 1.0f)) return 0.0f;
            return e.scale * (V > 0.04045f ? (2.4f / 1.055f) * powf((V + 0.055f) * (1.0f / 1.055f), 1.4f) : 1.0f / 12.92f);
        case FVVDP_EOTF_GAMMA:
            if (!(V > 0.0f && V <= 1.0f)) return 0.0f;
            return e.scale * e.gamma * powf(V, e.gamma - 1.0f);
        case FVVDP_EOTF_PQ: {
            if (!(V > 0.0f && V <= 1.0f)) return 0.0f;
            const float m = 78.843750000000000f, n = 0.15930175781250000f;
            const float c1 = 0.83593750000000000f, c2 = 18.851562500000000f, c3 = 18.687500000000000f;
            const float t = powf(V, 1.0f / m);
            if (!(t > c1)) return 0.0f;
            const float den = c2 - c3 * t;
            const float r = (t - c1) / den;
            const float L = 10000.0f * powf(r, 1.0f / n);
            if (!(L >= 0.005f && L <= e.y_peak)) return 0.0f;
            return L / (n * r) * ((c2 - c3 * c1) / (den * den)) * (t / (m * V));
        }
        case FVVDP_EOTF_LINEAR:
            return (V >= 0.005f && V <= e.y_peak) ? 1.0f : 0.0f;
        case FVVDP_EOTF_ABSOLUTE:
            return (V >= e.l_min && V <= e.l_max) ? 1.0f : 0.0f;
        default:
            return 0.0f;
    }
}

// The luminance of a channel sample differentiated for the display instead of the sample (display_grad_kernels.hpp).  With
// Y_black = E_ambient k_refl / pi + Y_peak / contrast and scale = Y_peak - Y_black the sample's luminance is
// scale f(clamp01 V) + Y_black (SRGB, GAMMA) or clip(g(V), 0.005, Y_peak) + Y_black (PQ, LINEAR); dL/dY_black = 1 throughout.
//   a1  SRGB / GAMMA: f(clamp01 V) = dL/dscale -- not zero at a clamped sample, unlike eotf_grad;
//       PQ / LINEAR: 1 where the upper luminance clip binds = dL/dY_peak at fixed Y_black, else 0;
//   a2  GAMMA: scale V^gamma ln V = dL/dgamma, exactly 0 at V <= 0 (and at V >= 1); 0 for every other model.
// powf / logf, not the forward's fast log2 / exp2 pair: the value is a factor of a sum that is compared with float64.
__device__ __forceinline__ void eotf_display_sens(float V, const EotfDev& e, float& a1, float& a2) {
    a1 = 0.0f;
    a2 = 0.0f;
    switch (e.kind) {
        case FVVDP_EOTF_SRGB: {
            const float v = fminf(fmaxf(V, 0.0f), 1.0f);
            a1 = v > 0.04045f ? powf((v + 0.055f) * (1.0f / 1.055f), 2.4f) : v * (1.0f / 12.92f);
            break;
        }
        case FVVDP_EOTF_GAMMA: {
            const float v = fminf(fmaxf(V, 0.0f), 1.0f);
            if (v > 0.0f) {
                a1 = powf(v, e.gamma);
                a2 = e.scale * a1 * logf(v);
            }
            break;
        }
        case FVVDP_EOTF_PQ: {
            const float v = fminf(fmaxf(V, 0.0f), 1.0f);
            const float m = 78.843750000000000f, n = 0.15930175781250000f;
            const float c1 = 0.83593750000000000f, c2 = 18.851562500000000f, c3 = 18.687500000000000f;
            const float t = v > 0.0f ? powf(v, 1.0f / m) : 0.0f;
            const float r = fmaxf(t - c1, 0.0f) / (c2 - c3 * t);
            const float L = r > 0.0f ? 10000.0f * powf(r, 1.0f / n) : 0.0f;
            a1 = L > e.y_peak ? 1.0f : 0.0f;
            break;
        }
        case FVVDP_EOTF_LINEAR:
            a1 = V > e.y_peak ? 1.0f : 0.0f;
            break;
        default:
            break;
    }
}
