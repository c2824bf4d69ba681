// The sums behind the gradient of the JOD with respect to the display's photometry (include/fvvdp_hip_display.h).  Instantiated
// and launched by display_grad_launch.hip.
//
// The display model enters the metric only before level 0: the luminance of source frame j at pixel x is sum_c w_c L(V_c), and
// with s[j][x] = dJOD / d(that luminance) the display's gradient needs, per stream (test, reference),
//   U0 = sum s sum_c w_c            U1 = sum s sum_c w_c a1(V_c)            U2 = sum s sum_c w_c a2(V_c)
// (a1, a2: eotf_display_sens, grad_common.hpp).  s is what video_input_kernel (video_grad_kernels.hpp) forms in registers before
// it applies the display model's derivative, and g0 = GL_0 + Reduce^T(GG_1) of grad_input_kernel (grad_kernels.hpp) for stills.
//
//   display_video_sums_kernel   the mirror of video_input_kernel: the same shifting register ring, head side buffer and fold
//                               cursor; where that kernel stores w_c EOTF'(V) s it adds s w_c {1, a1, a2} to three sums.
//   display_image_sums_kernel   g0 of one pixel of one pair, the same three products.
//   display_finalize_kernel     the workgroups' partials of one output added in a fixed order.
// Accumulation as tap_grad_kernel (tap_grad_kernels.hpp): fp32 fused multiply-adds over at most DS_CHAIN terms (the PX pixels x
// C channels of one frame), then fp64 per lane, a fixed __shfl_down tree over the 64 lanes, the four waves through the LDS in
// order, one partial per workgroup.  No atomics: the result repeats bit for bit.
#pragma once

#define DS_MAX_PAIRS 128                // pointer-table entries of one display_image_sums_kernel launch
#define DS_SUMS FVVDP_DISPLAY_SUMS
#define DS_CHAIN 16                     // most fp32 terms a sum takes before it moves to fp64

// s w_c {1, a1(V), a2(V)} of the PX pixels x C channels of one frame: one fp32 chain of PX C <= 12 terms per sum, then fp64
template <int PX>
__device__ __forceinline__ void ds_accumulate(const LaneVec<PX>& s, const LaneVec<PX> (&V)[3], int C, const EotfDev& e,
                                              const float (&wgt)[3], double (&sum)[DS_SUMS]) {
    static_assert(PX * 3 <= DS_CHAIN, "a frame's terms are one fp32 chain");
    float acc[DS_SUMS] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c < C) {
#pragma unroll
            for (int i = 0; i < PX; ++i) {
                float a1, a2;
                eotf_display_sens(V[c].v[i], e, a1, a2);
                acc[0] = fmaf(s.v[i], wgt[c], acc[0]);
                acc[1] = fmaf(s.v[i], wgt[c] * a1, acc[1]);
                acc[2] = fmaf(s.v[i], wgt[c] * a2, acc[2]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < DS_SUMS; ++k) sum[k] += (double)acc[k];
}

// fp64 from here: the lanes of a wave in a fixed tree, then the four waves in order -> out[DS_SUMS] of this workgroup
__device__ __forceinline__ void ds_block_reduce(const double (&sum)[DS_SUMS], double* out) {
    __shared__ double s_wave[4][DS_SUMS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < DS_SUMS; ++k) {
        double v = sum[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) s_wave[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < DS_SUMS) {
        const int k = threadIdx.x;
        out[k] = ((s_wave[0][k] + s_wave[1][k]) + s_wave[2][k]) + s_wave[3][k];
    }
}

// ---- video: temporal transpose + the three products ------------------------------------------------------------------------
struct DisplayVideoSumsArgs {
    TransposeArgs t;        // g0, head, sizes, taps and fold list
    const float* src;       // element (c, f, px) at c * chan_stride + f * frame_stride + px
    double* partial;        // [gridDim.x][DS_SUMS]
    size_t chan_stride, frame_stride;
    int C;
    EotfDev e;
    float wgt[3];
};
static_assert(offsetof(DisplayVideoSumsArgs, t) == 0, "transpose_step and FoldCursor read the start of the kernel-argument segment");

// FL, PX: see TransposeRing.  The transpose of transpose_kernels.hpp, so s of frame j is the value video_input_kernel forms; a
// lane past the frame reads nothing, carries zeros and stays for the shuffles and the barrier of the reduction.
template <int FL, int PX>
__global__ __launch_bounds__(256) void display_video_sums_kernel(const DisplayVideoSumsArgs a) {
    const size_t px = ((size_t)blockIdx.x * 256 + threadIdx.x) * PX;
    const bool live = px < (size_t)a.t.HW;
    TransposeRing<FL, PX> ring = transpose_ring<FL, PX>();
    double sum[DS_SUMS] = {0.0, 0.0, 0.0};
    const size_t HW = (size_t)a.t.HW;
    FoldCursor<PX> fold(a.t.head, HW, px, a.t.fl, live);
    const int total = a.t.N + a.t.fl - 1;
    for (int p = 0; p < total; ++p) {
        const int j = p - (a.t.fl - 1);         // the frame that is complete after this step
        LaneVec<PX> gs, gt;
        transpose_inputs<PX>(a.t.g0, p, a.t.N, HW, px, gs, gt, live);
        LaneVec<PX> V[3];                       // the samples of frame j, requested before the arithmetic
        if (j >= 0) {
            const float* t = a.src + (size_t)j * a.frame_stride + px;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (c < a.C) V[c] = lane_load<PX>(t + (size_t)c * a.chan_stride, live);
        }
        const LaneVec<PX> done = transpose_step<FL, PX>(ring, gs, gt);
        if (p < a.t.fl && live) lane_store<PX>(a.t.head + (size_t)p * HW + px, done);
        if (j >= 0) ds_accumulate<PX>(fold.frame_sum(j, done), V, a.C, a.e, a.wgt, sum);
    }
    ds_block_reduce(sum, a.partial + (size_t)blockIdx.x * DS_SUMS);
}

// ---- still images: level 0 of the sweep + the three products -------------------------------------------------------------
struct DisplayImageSumsArgs {
    const float* img[DS_MAX_PAIRS];
    const float* GL0;       // [n][h][w] layer gradient of level 0, pair 0 of the launch
    const float* GG1;       // [n][hc][wc] gradient of G_1
    double* partial;        // [n][gridDim.x][DS_SUMS], pair 0 of the launch
    size_t chan_stride;
    int C, w, h, wc, hc;
    EotfDev e;
    float wgt[3];
};

// grid (ceil(h w / 256), pairs of the launch)
__global__ __launch_bounds__(256) void display_image_sums_kernel(const DisplayImageSumsArgs a) {
    const int k = blockIdx.y;
    const size_t hw = (size_t)a.w * a.h;
    const size_t px = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = px < hw;
    double sum[DS_SUMS] = {0.0, 0.0, 0.0};
    if (live) {
        const int y = (int)(px / (size_t)a.w), x = (int)(px - (size_t)y * a.w);
        LaneVec<1> s, V[3];
        s.v[0] = a.GL0[(size_t)k * hw + px] + reduce_t(a.GG1 + (size_t)k * a.wc * a.hc, a.wc, a.hc, a.w, a.h, y, x);
        const float* img = a.img[k];
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (c < a.C) V[c].v[0] = img[(size_t)c * a.chan_stride + px];
        ds_accumulate<1>(s, V, a.C, a.e, a.wgt, sum);
    }
    ds_block_reduce(sum, a.partial + ((size_t)k * gridDim.x + blockIdx.x) * DS_SUMS);
}

// ---- the partials of one output, in a fixed order ------------------------------------------------------------------------------
struct DisplayFinalizeArgs {
    const double* partial;  // [outputs][blocks][DS_SUMS]
    double* out;            // [outputs][DS_SUMS]
    int blocks;
};

// grid (outputs), 256 threads: thread t adds value t % 4 (the fourth is idle) of workgroups t / 4, t / 4 + 64, ... in order,
// thread v < DS_SUMS then the 64 rows in order.  The grouping depends on the frame size only.
#define DS_ROWS 64
__global__ __launch_bounds__(256) void display_finalize_kernel(const DisplayFinalizeArgs a) {
    __shared__ double s_row[DS_ROWS][4];
    const int g = blockIdx.x;
    const int v = threadIdx.x & 3, row = threadIdx.x >> 2;
    double acc = 0.0;
    if (v < DS_SUMS)
        for (int i = row; i < a.blocks; i += DS_ROWS) acc += a.partial[((size_t)g * a.blocks + i) * DS_SUMS + v];
    s_row[row][v] = acc;
    __syncthreads();
    if (threadIdx.x < DS_SUMS) {
        double t = 0.0;
        for (int r = 0; r < DS_ROWS; ++r) t += s_row[r][threadIdx.x];
        a.out[(size_t)g * DS_SUMS + threadIdx.x] = t;
    }
}
