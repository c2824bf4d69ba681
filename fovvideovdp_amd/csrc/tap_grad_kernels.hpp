// The temporal kernel differentiated for its taps (include/fvvdp_hip_taps.h): dJOD/dlevel0 of a batch of output frames
// correlated with the luminance frames under the sliding window.  Instantiated and launched by tap_grad_launch.hip.
//
//   out[cc][k] = sum_t sum_x ( g0[t][cc][x] Y_T[pos[t + fl - 1 - k]][x] + g0_r[t][cc][x] Y_R[pos[t + fl - 1 - k]][x] )
//
//   tap_grad_kernel      grid (pixel blocks, tap groups).  A lane owns PX consecutive pixels and walks the batch's output frames
//                        once for the R taps k0 .. k0 + R - 1 of its group.  Tap k0 + j of frame t multiplies list entry
//                        q = (fl - 1 - k0) + t - j: the R entries open at frame t live in a register ring per clip, entry q in
//                        slot (q - (fl - 1 - k0)) mod R, so the newest entry of frame t goes to slot t mod R and tap k0 + j reads
//                        slot (t - j) mod R.  The frame loop is unrolled R times: every slot index is a constant.  Entries
//                        before the list (taps past fl - 1 in the last group) read as 0 and their sums are not stored.
//                        Per frame and pixel: four gradient values, one new luminance sample per clip, 4 R fused multiply-adds
//                        into 2 R fp32 sums per lane.  A sum takes 2 PX terms per frame; after TG_CHAIN terms it moves to fp64
//                        (every 2 frames for PX = 4, every 8 for PX = 1), as param_sums_kernel does.  Then fp64 only: shuffles
//                        inside the wave, the four waves through the LDS in order, one partial per workgroup.
//   tap_finalize_kernel  the partials of a tap group added in a fixed order.
#pragma once

#define TG_R FVVDP_TAP_GROUP
#define TG_MAX_POS FVVDP_TAPS_MAX_POSITIONS
#define TG_CHAIN 16                                    // fp32 terms per sum before it moves to fp64

struct TapGradArgs {
    const float* g0;        // [n][2][HW] test side
    const float* g0r;       // [n][2][HW] reference side
    const float* yt;        // [frames][HW] luminance of the test clip
    const float* yr;        // [frames][HW] luminance of the reference clip
    double* partial;        // [groups][gridDim.x][2][TG_R]
    int HW, n, fl;
    int pos[TG_MAX_POS];    // [fl - 1 + n] luminance frame of every list entry
};

// what one output frame brings: the newest luminance sample of both clips and the four gradient planes
template <int PX>
struct TgStep {
    LaneVec<PX> vt, vr, gs, gt, hs, ht;
};
template <int PX, class POS>
__device__ __forceinline__ TgStep<PX> tg_step(const TapGradArgs& a, POS pos, int q0, int t, size_t HW, size_t px, bool live) {
    TgStep<PX> s;
    const size_t o = (size_t)pos[q0 + t] * HW + px;
    const size_t og = (size_t)t * 2 * HW + px;
    s.vt = lane_load<PX>(a.yt + o, live);
    s.vr = lane_load<PX>(a.yr + o, live);
    s.gs = lane_load<PX>(a.g0 + og, live);
    s.gt = lane_load<PX>(a.g0 + og + HW, live);
    s.hs = lane_load<PX>(a.g0r + og, live);
    s.ht = lane_load<PX>(a.g0r + og + HW, live);
    return s;
}

// R: taps per group.  PX: pixels per lane (4: HW a multiple of 4 and every pointer 16-byte aligned; 1: any size).
template <int R, int PX>
__global__ __launch_bounds__(256, 2) void tap_grad_kernel(const TapGradArgs a) {
    constexpr int FRAMES = TG_CHAIN / (2 * PX);       // frames per fp32 chain: 2 PX terms per frame and sum
    static_assert(R % FRAMES == 0 && (R & (R - 1)) == 0, "the flush points and the ring slots are constants of the unrolled loop");
    __shared__ double s_wave[4][2 * R];
    const size_t HW = (size_t)a.HW;
    const size_t px = ((size_t)blockIdx.x * 256 + threadIdx.x) * PX;
    const bool live = px < HW;                         // (PX = 4: HW % 4 == 0, the lane's pixels are all inside or all outside)
    const int q0 = a.fl - 1 - (int)blockIdx.y * R;     // list entry that tap k0 multiplies at frame 0: >= 0, k0 < fl
    typedef const int __attribute__((address_space(4)))* karg_int_p;
    typedef const char __attribute__((address_space(4)))* karg_p;
    const karg_int_p pos = (karg_int_p)((karg_p)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(TapGradArgs, pos));

    float rt[R][PX], rr[R][PX];                        // slot s: list entry q with (q - q0) mod R == s
#pragma unroll
    for (int m = 1; m < R; ++m) {                      // the R - 1 entries before frame 0's newest
        const int q = q0 - m;
        const bool in = live && q >= 0;
        const size_t o = in ? (size_t)pos[q >= 0 ? q : 0] * HW + px : 0;
        const LaneVec<PX> vt = lane_load<PX>(a.yt + o, in), vr = lane_load<PX>(a.yr + o, in);
#pragma unroll
        for (int i = 0; i < PX; ++i) { rt[R - m][i] = vt.v[i]; rr[R - m][i] = vr.v[i]; }
    }
    float acc[2][R];
    double sum[2][R];
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
#pragma unroll
        for (int j = 0; j < R; ++j) { acc[cc][j] = 0.0f; sum[cc][j] = 0.0; }

    // one frame in flight: the values of frame t + 1 are requested before the arithmetic of frame t, and the steps of the unrolled
    // loop stay apart (left alone, the compiler hoists the loads of all R steps and the kernel runs at one wave per SIMD)
    TgStep<PX> nx = tg_step<PX>(a, pos, q0, 0, HW, px, live);
    for (int tb = 0; tb < a.n; tb += R) {
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int t = tb + u;
            if (t < a.n) {                             // wave-uniform
                const TgStep<PX> c = nx;
                if (t + 1 < a.n) nx = tg_step<PX>(a, pos, q0, t + 1, HW, px, live);
#pragma unroll
                for (int i = 0; i < PX; ++i) { rt[u][i] = c.vt.v[i]; rr[u][i] = c.vr.v[i]; }
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    constexpr int M = R - 1;
                    const int s = (u - j) & M;
#pragma unroll
                    for (int i = 0; i < PX; ++i) {
                        acc[0][j] = fmaf(c.gs.v[i], rt[s][i], acc[0][j]);
                        acc[0][j] = fmaf(c.hs.v[i], rr[s][i], acc[0][j]);
                        acc[1][j] = fmaf(c.gt.v[i], rt[s][i], acc[1][j]);
                        acc[1][j] = fmaf(c.ht.v[i], rr[s][i], acc[1][j]);
                    }
                }
            }
            if (u % FRAMES == FRAMES - 1) {            // TG_CHAIN terms at the most: on to fp64
#pragma unroll
                for (int cc = 0; cc < 2; ++cc)
#pragma unroll
                    for (int j = 0; j < R; ++j) { sum[cc][j] += (double)acc[cc][j]; acc[cc][j] = 0.0f; }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // fp64 from here: lanes of a wave in a fixed tree, then the four waves in order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
#pragma unroll
        for (int j = 0; j < R; ++j) {
            double v = sum[cc][j];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) s_wave[wave][cc * R + j] = v;
        }
    __syncthreads();
    if (threadIdx.x < 2 * R) {
        const int v = threadIdx.x;
        const double t = ((s_wave[0][v] + s_wave[1][v]) + s_wave[2][v]) + s_wave[3][v];
        a.partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (2 * R) + v] = t;
    }
}

struct TapFinalizeArgs {
    const double* partial;  // [groups][blocks][2][TG_R]
    double* out;            // [2][fl]
    int blocks, fl;
};

// grid (groups), 256 threads: thread t adds value t % 16 of the group's workgroups t / 16, t / 16 + 16, ... in order, thread
// v < 16 then the 16 rows in order.  The grouping depends on the frame size only.
#define TG_ROWS (256 / (2 * TG_R))
__global__ __launch_bounds__(256) void tap_finalize_kernel(const TapFinalizeArgs a) {
    __shared__ double s_row[TG_ROWS][2 * TG_R];
    const int g = blockIdx.x;
    const int v = threadIdx.x % (2 * TG_R), row = threadIdx.x / (2 * TG_R);
    double acc = 0.0;
    for (int i = row; i < a.blocks; i += TG_ROWS) acc += a.partial[((size_t)g * a.blocks + i) * (2 * TG_R) + v];
    s_row[row][v] = acc;
    __syncthreads();
    if (threadIdx.x < 2 * TG_R) {
        double t = 0.0;
        for (int r = 0; r < TG_ROWS; ++r) t += s_row[r][v];
        const int cc = v / TG_R, k = g * TG_R + v % TG_R;
        if (k < a.fl) a.out[(size_t)cc * a.fl + k] = t;
    }
}
