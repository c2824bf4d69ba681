// Backward of the video JOD under many gazes (include/fvvdp_hip_gaze_grad.h): the layer gradients of a loss
//   sum_g w_g JOD_g    (w_g = the upstream gradient of gaze g)
// summed over the gazes BEFORE the linear tail of the backward (adj_sweep_kernel, video_level0_kernel, video_input_kernel), which
// then runs once instead of once per gaze.  Instantiated and launched by gaze_grad_launch.hip.
//
// The gaze enters the backward in two places only: the coefficients c_g[f][cc][b] (video_coef_kernel, from gaze g's Q_per_ch and
// w_g) and the CSF sensitivity S_g of a band pixel, a function of its eccentricity.  Everything else video_layer_kernel reads
// (the four contrast planes, L_bkg) does not depend on the gaze, so one map-writing pyramid pass serves every gaze and
// gaze_layer_kernel evaluates S_g itself instead of reading it from a map:
//   per band pixel, once:  contrast x 4, L_bkg, m_b / L_bkg, the view direction and resolution magnification of the pixel
//                          (fvvdp_display_model.py:475-526), the rho and Y axes of the CSF query (interval and fraction);
//   per gaze of the group: eccentricity -> ecc axis -> trilinear blend of the 8 cells of each temporal channel's 32^3 table ->
//                          S = 2^(.) -> the layer term of video_layer_kernel's formula.
// The query is band_px's (band_kernel.hpp, the map-writing pass): clamp, interval from the uniform grid, fraction from the
// stored knots with interp.py:16's + 1e-6, blends in the association of interp3 -- on the full tables in global memory (2 x 128
// KiB, L2 resident) instead of a band's slice, so displays of any field of view take this kernel.
#pragma once

struct GazeBand {
    const float* Cn;        // [n][4][h][w]  plane 2cc: test contrast x m_b, plane 2cc + 1: reference
    const float* L;         // [n][h][w]     L_bkg (clamped from below by the forward)
    float* GL;              // [n][2][h][w]  sum over the gazes of the layer gradient
    int w, h, blk0;         // first workgroup of this band in blockIdx.x
    float m;                // band multiplier
    float rho_band;         // centre frequency of the band, cycles per degree
    float kx, kyb;          // display_size_m / band size / distance: pixel offset from the centre -> tangent of the view angle
};
struct GazeLayerArgs {
    GazeBand band[FVVDP_MAX_BANDS];
    const float* coef;      // gaze slot g of the group: coef + g * coef_stride, then [n][2][n_bands]
    const float* gaze;      // gaze slot g, frame k of the batch: gaze[g * gaze_stride + 2 k] = (x, y) in frame pixels
    const float* lut0;      // S_log of the sustained channel [Y][rho][ecc], 32^3
    const float* lut1;      // ... of the transient channel
    const float* axes;      // [3][32] knots: Y_log, rho_log, ecc_sqrt
    long long coef_stride, gaze_stride;
    int n_bands;
    int accumulate;         // 0: the first group of the batch stores; 1: a later group adds to what is there
    int frame_w, frame_h;
    float p, q[2], k_mask, beta, gain, cmax_hi, dmax_hi;
    float size_m0, size_m1, dist_m, cos_delta, delta_rad;
    float rho_lo, rho_hi, ly_lo, ly_hi, ecc_lo, ecc_hi;
    float first[3], inv_step[3];        // uniform-grid estimate of the interval on the three axes
};

// video_layer_one (video_grad_kernels.hpp) with one change: the forward's D is not read from a map but is the value formed
// here, and the d_max clamp and the D == 0 gate test that value.  s = S gain; s * m_lb = S gain m / L_bkg is d(T')/d(layer).
__device__ __forceinline__ float gaze_layer_one(float c, float T, float R, float s, float m_lb, float q, float m,
                                                const GazeLayerArgs& a) {
    const float Tp = T * s, Rp = R * s;
    const float u = Tp - Rp, au = fabsf(u);
    const float aT = fabsf(Tp), aR = fabsf(Rp);
    const float M = a.k_mask * fminf(aT, aR);
    const float Mq = M > 0.0f ? fast_exp2(q * fast_log2(M)) : 0.0f;
    const float den = 1.0f + Mq;
    const float lnum = a.p * fast_log2(au);                 // au == 0: -inf, num = 0, D = 0
    const float num = fast_exp2(lnum);
    const float rden = fast_rcp(den);
    const float D = num * rden;
    // zero: no pooling weight, D == 0 (an identical pixel), the d_max clamp or the contrast clamp binds
    if (!(c != 0.0f && D > 0.0f && D < a.dmax_hi && T < m * a.cmax_hi)) return 0.0f;
    // dD/dT': the difference term, and the masker term where |T'| is the smaller (ties split, as torch.minimum's backward)
    float dD = copysignf(a.p * num * fast_rcp(au), u) * rden;
    if (M > 0.0f && aT <= aR) {
        const float share = aT < aR ? 1.0f : 0.5f;
        dD -= share * copysignf(D * rden * q * Mq * fast_rcp(aT), Tp);
    }
    const float Db = fast_exp2((a.beta - 1.0f) * (lnum - fast_log2(den)));      // D^(beta - 1)
    return c * Db * dD * s * m_lb;
}

// interval k in [0, 30] and fraction f >= 0 of query q on axis ax (interp.py:11-20 on a uniform axis, as band_px)
__device__ __forceinline__ void gaze_axis(const GazeLayerArgs& a, const float2* s_ax, int ax, float q, int& k, float& f) {
    k = min(max((int)floorf((q - a.first[ax]) * a.inv_step[ax]), 0), FVVDP_LUT_N - 2);
    const float2 kn = s_ax[ax * FVVDP_LUT_N + k];
    f = fmaxf((q - kn.x) * kn.y, 0.0f);
}

// grid (workgroups of all bands, n frames), 256 threads, one band pixel per thread.  NG gazes per launch: 1, 2, 4 or 8.
// GL = sum_g term_g in ascending gaze order, starting from +0: the first group of a batch starts from zero, a later one from the
// value the groups before it left, so the sum is the same chain of additions whatever the group sizes.  No atomics.
template <int NG>
__global__ __launch_bounds__(256) void gaze_layer_kernel(const GazeLayerArgs a) {
    __shared__ float2 s_ax[3 * FVVDP_LUT_N];        // {knot k, 1 / (knot k+1 - knot k + 1e-6)}
    __shared__ float2 s_gz[NG];                     // view direction of the gazes in degrees
    const int tid = threadIdx.x;
    const int k = blockIdx.y;
    if (tid < 3 * FVVDP_LUT_N) {
        const int i = tid % FVVDP_LUT_N;
        const float x0 = a.axes[tid];
        const float x1 = a.axes[i + 1 < FVVDP_LUT_N ? tid + 1 : tid];
        s_ax[tid] = make_float2(x0, 1.0f / (x1 - x0 + 0.000001f));
    } else if (tid >= 128 && tid < 128 + NG) {
        // the gaze as band_item converts it (pix2view_direction at frame resolution, pixel centres at + 0.5)
        const float* fx = a.gaze + (size_t)(tid - 128) * a.gaze_stride + 2 * k;
        const float fxp = fx[0] + 0.5f, fyp = fx[1] + 0.5f;
        const float gxm = (fxp + (-(float)a.frame_w / 2.0f)) * a.size_m0 / (float)a.frame_w;
        const float gym = -(fyp + (-(float)a.frame_h / 2.0f)) * a.size_m1 / (float)a.frame_h;
        s_gz[tid - 128] = make_float2(atanf(gxm / a.dist_m) * 57.29577951308232f, atanf(gym / a.dist_m) * 57.29577951308232f);
    }
    __syncthreads();
    int b = 0;
    while (b + 1 < a.n_bands && (int)blockIdx.x >= a.band[b + 1].blk0) ++b;
    const GazeBand& B = a.band[b];
    const size_t hw = (size_t)B.w * B.h;
    const size_t px = (size_t)((int)blockIdx.x - B.blk0) * 256 + tid;
    if (px >= hw) return;
    const int y = (int)((unsigned int)px / (unsigned int)B.w), x = (int)px - y * B.w;

    // ---- once per band pixel ------------------------------------------------------------------------------------------------
    const float lb = B.L[(size_t)k * hw + px];
    const float m_lb = B.m / lb;
    float T[2], R[2];
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
        T[cc] = B.Cn[((size_t)k * 4 + 2 * cc) * hw + px];
        R[cc] = B.Cn[((size_t)k * 4 + 2 * cc + 1) * hw + px];
    }
    // pix2view_direction on the band grid and the resolution magnification at that angle, as band_item / fov_rho_map_kernel
    const float xa = ((float)x + 0.5f) + (-(float)B.w / 2.0f);
    const float yp = ((float)y + 0.5f) + (-(float)B.h / 2.0f);
    const float vx = atanf(xa * B.kx) * 57.29577951308232f;
    const float vy = atanf(-yp * B.kyb) * 57.29577951308232f;
    const float va = fminf(__builtin_amdgcn_sqrtf(vx * vx + vy * vy), 89.9f) * 0.017453292519943295f;
    const float rm = a.cos_delta * fast_rcp(__cosf(va) * __cosf(va + a.delta_rad));
    const float rq = fast_log2(fminf(fmaxf(B.rho_band * rm, a.rho_lo), a.rho_hi));
    const float yq = __builtin_amdgcn_fmed3f(fast_log2(lb), a.ly_lo, a.ly_hi);
    int kR, kY;
    float fR, fY;
    gaze_axis(a, s_ax, 1, rq, kR, fR);
    gaze_axis(a, s_ax, 0, yq, kY, fY);
    const float gY = 1.0f - fY;
    const int base = (kY * FVVDP_LUT_N + kR) * FVVDP_LUT_N;            // S_log[Y][rho][ecc]
    constexpr int sR = FVVDP_LUT_N, sY = FVVDP_LUT_N * FVVDP_LUT_N;

    float acc[2] = {0.0f, 0.0f};
    float* out = B.GL + (size_t)k * 2 * hw + px;
    if (a.accumulate) {
        acc[0] = out[0];
        acc[1] = out[hw];
    }

    // ---- once per gaze of the group -----------------------------------------------------------------------------------------
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const float2 gz = s_gz[g];
        const float dx = vx - gz.x, dy = vy - gz.y;
        const float ecc = __builtin_amdgcn_sqrtf(dx * dx + dy * dy);
        const float eq = __builtin_amdgcn_sqrtf(fminf(fmaxf(ecc, a.ecc_lo), a.ecc_hi));
        int kE;
        float fE;
        gaze_axis(a, s_ax, 2, eq, kE, fE);
        const float gE = 1.0f - fE;
        const float* cf = a.coef + (size_t)g * a.coef_stride + (size_t)k * 2 * a.n_bands + b;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const float* t = (cc == 0 ? a.lut0 : a.lut1) + base + kE;
            // interp3 (interp.py:53-57): rho blend, then Y, then ecc; the rho blend in slope form as the forward's slices
            const float v00 = t[0], v01 = t[1], w00 = t[sR], w01 = t[sR + 1];
            const float v10 = t[sY], v11 = t[sY + 1], w10 = t[sY + sR], w11 = t[sY + sR + 1];
            const float r00 = fmaf(w00 - v00, fR, v00), r01 = fmaf(w01 - v01, fR, v01);        // r[dY][dE]
            const float r10 = fmaf(w10 - v10, fR, v10), r11 = fmaf(w11 - v11, fR, v11);
            const float slog = (r00 * gY + r10 * fY) * gE + (r01 * gY + r11 * fY) * fE;
            const float s = fast_exp2(slog) * a.gain;
            const float term = gaze_layer_one(cf[cc * a.n_bands], T[cc], R[cc], s, m_lb, a.q[cc], B.m, a);
            acc[cc] = __fadd_rn(acc[cc], term);
        }
    }
    out[0] = acc[0];
    out[hw] = acc[1];
}
