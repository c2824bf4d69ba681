// Sums over the maps of a map-writing pyramid pass for the derivatives of the JOD with respect to the masking parameters
// (include/fvvdp_hip_params.h).  Instantiated and launched by param_launch.hip.
//
// Per band pixel and temporal channel (fvvdp.py:447, 574-596): T' = T S g, R' = R S g, u = |T' - R'|, M = k min(|T'|, |R'|),
// D = min(u^p / (1 + M^q), d_max), and the band's Q = (mean D^beta)^(1/beta).  Where 0 < D < d_max
//   dD/dp = D ln u,  dD/dq = -D a ln M,  dD/dc = -D a q ln 10,  dD/dsc = D (p - q a) ln 10 / 20,   a = M^q / (1 + M^q)
// so the derivatives of Q need sum D^beta {1, ln u, a ln M, a} over those pixels, and dQ/dbeta needs sum D^beta ln D over all.
//   param_sums_kernel     lanes own whole pixels (4 consecutive ones per 16-byte load, or 1); per-lane fp32 sums over at most 16
//                         pixels, then fp64: shuffles inside the wave, the four waves through the LDS, one partial per workgroup
//   param_finalize_kernel the band's partials of one slot added in a fixed order
// The logarithms are summed as log2 and scaled by ln 2 in fp64 at the end.
#pragma once

#define PS_SUMS FVVDP_PARAM_SUMS
#define PS_GROUPS 4                                   // 4-pixel groups (vector path) per lane
#define PS_BLOCK_PX FVVDP_PARAM_SUMS_BLOCK_PX         // 256 lanes x 4 pixels x PS_GROUPS
#define PS_FLT_MIN 1.17549435e-38f                    // v_log_f32 returns -inf below: such values count as 0

struct ParamBand {
    const float* D;         // [n][2][hw]   plane cc
    const float* Cn;        // [n][P][hw]   plane 2cc: test contrast x m_b, plane 2cc + 1: reference
    const float* S;         // [n][2][hw]   plane cc: sensitivity before the gain
    unsigned int hw;        // pixels of the band
    int blk0;               // first workgroup of this band in blockIdx.x
    int vec;                // 16-byte loads: hw % 4 == 0 and the three maps 16-byte aligned
};
struct ParamSumsArgs {
    ParamBand band[FVVDP_MAX_BANDS];
    double* partial;        // [blocks of all bands][n][2][PS_SUMS]
    int n_bands, n;
    float p, q[2], k_mask, beta, gain, dmax_hi;
};

// one pixel of one temporal channel into the lane's sums {D^b, D^b lg u, D^b a lg M, D^b a, D^b lg D}
__device__ __forceinline__ void ps_pixel(float D, float T, float R, float S, float q, const ParamSumsArgs& a, float (&acc)[PS_SUMS]) {
    const float s = S * a.gain;
    const float Tp = T * s, Rp = R * s;
    const float u = fabsf(Tp - Rp);
    const float M = a.k_mask * fminf(fabsf(Tp), fabsf(Rp));
    const bool pos = D >= PS_FLT_MIN;
    const bool live = pos && D < a.dmax_hi;
    const float lgD = fast_log2(D);
    const float Db = pos ? fast_exp2(a.beta * lgD) : 0.0f;
    acc[4] += pos ? Db * lgD : 0.0f;
    const float Dl = live ? Db : 0.0f;
    acc[0] += Dl;
    const float lgu = fast_log2(u);
    acc[1] += (live && u >= PS_FLT_MIN) ? Dl * lgu : 0.0f;
    const bool masked = live && M >= PS_FLT_MIN;
    const float lgM = fast_log2(M);
    const float Mq = fminf(fast_exp2(q * lgM), 0x1p100f);           // (inf * rcp(inf) would be NaN)
    const float da = masked ? Dl * (Mq * fast_rcp(1.0f + Mq)) : 0.0f;
    acc[3] += da;
    acc[2] += masked ? da * lgM : 0.0f;
}

// P: planes of the contrast map (2: still images, one temporal channel; 4: video, two).  grid (blocks of all bands, n)
template <int P>
__global__ __launch_bounds__(256) void param_sums_kernel(const ParamSumsArgs a) {
    constexpr int CH = P / 2;
    __shared__ double s_wave[4][CH * PS_SUMS];
    int b = 0;
    while (b + 1 < a.n_bands && (int)blockIdx.x >= a.band[b + 1].blk0) ++b;
    const ParamBand& B = a.band[b];
    const int k = blockIdx.y;
    const size_t hw = B.hw;
    const size_t px0 = (size_t)((int)blockIdx.x - B.blk0) * PS_BLOCK_PX;
    const float* pD = B.D + (size_t)k * 2 * hw;
    const float* pS = B.S + (size_t)k * 2 * hw;
    const float* pC = B.Cn + (size_t)k * P * hw;
    float acc[CH][PS_SUMS];
#pragma unroll
    for (int cc = 0; cc < CH; ++cc)
#pragma unroll
        for (int j = 0; j < PS_SUMS; ++j) acc[cc][j] = 0.0f;
    if (B.vec) {                                       // wave-uniform: a property of the band
#pragma unroll
        for (int g = 0; g < PS_GROUPS; ++g) {
            const size_t px = px0 + (size_t)g * 1024 + threadIdx.x * 4;
            if (px < hw) {                             // hw % 4 == 0: the whole group is inside
#pragma unroll
                for (int cc = 0; cc < CH; ++cc) {
                    const v4f D = *reinterpret_cast<const v4f*>(pD + cc * hw + px);
                    const v4f S = *reinterpret_cast<const v4f*>(pS + cc * hw + px);
                    const v4f T = *reinterpret_cast<const v4f*>(pC + (2 * cc) * hw + px);
                    const v4f R = *reinterpret_cast<const v4f*>(pC + (2 * cc + 1) * hw + px);
#pragma unroll
                    for (int i = 0; i < 4; ++i) ps_pixel(D[i], T[i], R[i], S[i], a.q[cc], a, acc[cc]);
                }
            }
        }
    } else {
#pragma unroll 4
        for (int g = 0; g < 4 * PS_GROUPS; ++g) {
            const size_t px = px0 + (size_t)g * 256 + threadIdx.x;
            if (px < hw) {
#pragma unroll
                for (int cc = 0; cc < CH; ++cc)
                    ps_pixel(pD[cc * hw + px], pC[(2 * cc) * hw + px], pC[(2 * cc + 1) * hw + px], pS[cc * hw + px], a.q[cc], a,
                             acc[cc]);
            }
        }
    }
    // fp64 from here: lanes of a wave in a fixed tree, then the four waves in order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int cc = 0; cc < CH; ++cc)
#pragma unroll
        for (int j = 0; j < PS_SUMS; ++j) {
            double v = (double)acc[cc][j];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) s_wave[wave][cc * PS_SUMS + j] = v;
        }
    __syncthreads();
    if (threadIdx.x < CH * PS_SUMS) {
        const int v = threadIdx.x;
        const double t = ((s_wave[0][v] + s_wave[1][v]) + s_wave[2][v]) + s_wave[3][v];
        a.partial[((size_t)blockIdx.x * a.n + k) * (2 * PS_SUMS) + v] = t;
    }
}

struct ParamFinalizeArgs {
    const double* partial;  // [blocks of all bands][n][2][PS_SUMS]
    double* sums;           // [n_bands][2][n][PS_SUMS]
    int blk0[FVVDP_MAX_BANDS + 1];
    int n, channels;
};

// grid (n_bands, n), 256 threads: thread t adds value t % 10 of the band's workgroups t / 10, t / 10 + 25, ... in order, thread
// v < 10 then the 25 rows in order.  The grouping depends on the band's size only.
#define PS_ROWS 25
__global__ __launch_bounds__(256) void param_finalize_kernel(const ParamFinalizeArgs a) {
    __shared__ double s_row[PS_ROWS][2 * PS_SUMS];
    const int b = blockIdx.x, k = blockIdx.y;
    const int v = threadIdx.x % (2 * PS_SUMS), row = threadIdx.x / (2 * PS_SUMS);
    const bool used = v < a.channels * PS_SUMS;
    if (row < PS_ROWS) {
        double acc = 0.0;
        if (used)
            for (int i = a.blk0[b] + row; i < a.blk0[b + 1]; i += PS_ROWS)
                acc += a.partial[((size_t)i * a.n + k) * (2 * PS_SUMS) + v];
        s_row[row][v] = acc;
    }
    __syncthreads();
    if (threadIdx.x < 2 * PS_SUMS) {
        double t = 0.0;
        for (int r = 0; r < PS_ROWS; ++r) t += s_row[r][v];
        const int cc = v / PS_SUMS, j = v % PS_SUMS;
        if (j == 1 || j == 2 || j == 4) t *= 0.69314718055994530942;          // log2 -> ln
        a.sums[(((size_t)b * 2 + cc) * a.n + k) * PS_SUMS + j] = t;
    }
}
