// Clips whose two streams have frame counts of their own (include/fvvdp_hip_held.h): each stream is shown by sample-and-hold
// through a frame map, and the pair is judged at the display's rate.  Instantiated and launched by held_launch.hip.
//
// Forward: the register-ring ingest of temporal_kernels.hpp already reads one window index list per stream (TemporalArgs::idx /
// idx1); what a pair of clips with different frame counts adds is a second stride pair, because the channel stride of a planar
// clip is its frame count times the frame size.  held_vec_kernel / held_ring_kernel are the existing bodies (temporal_vec_body,
// temporal_ring_body) instantiated with S2 = true: stream 1 takes its strides from the two size_t behind the TemporalArgs.  Every
// arithmetic instruction is the one of temporal_vec_kernel / temporal_ring_kernel, so level 0 has the bits predict gives on the
// clips expanded with index_select.  A held frame is simply read again at every display step.
//
// Backward: video_input_held_kernel, the transpose of the temporal filter followed by the transpose of the hold (a sum over the
// display frames that show a source frame) and the display model's derivative, in one launch.
#pragma once

struct HeldTemporalArgs {
    TemporalArgs a;
    size_t chan_stride1, frame_stride1;     // stream 1 (read by stream1_strides<true>, temporal_kernels.hpp)
};
static_assert(offsetof(HeldTemporalArgs, chan_stride1) == sizeof(TemporalArgs), "stream1_strides reads behind the TemporalArgs");
static_assert(offsetof(HeldTemporalArgs, frame_stride1) == sizeof(TemporalArgs) + sizeof(size_t), "stream1_strides");

// temporal_vec_kernel's dispatch on the display model and the channel count (no ticket counter, no 64-slot ring), every sample type
template <int FL, int PX, int SRC>
__global__ __launch_bounds__(64 * k1_wpb(FL), k1_waves(FL, SRC))
void held_vec_kernel(const HeldTemporalArgs h_byval) {
    const TemporalArgs& a = *(const TemporalArgs*)__builtin_amdgcn_kernarg_segment_ptr();      // see temporal_vec_kernel
    (void)h_byval;
    static_assert(FL <= 32, "8 / 16 / 32 slots");
    constexpr int TD = 1;
    constexpr int WPB = k1_wpb(FL);
    __shared__ float lutw[SRC == SRC_U8 ? 768 : 1];
    __shared__ float4 s_t_all[WPB][64 * (PX + 1)];
    if constexpr (SRC == SRC_U8) {
        build_lutw(lutw, a.e, a.C, a.w, threadIdx.x, 64 * WPB);
        __syncthreads();
    }
    const int wave = WPB > 1 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
    float4* const s_t = s_t_all[wave];
    const int block0 = (int)blockIdx.x * WPB + wave;
    if constexpr (WPB > 1) {
        if (block0 * (64 * PX) >= a.HW) return;
    }
    if constexpr (SRC == SRC_U8) {
        temporal_vec_cc<FL, PX, SRC, TD, FVVDP_EOTF_LUT, true>(a, lutw, s_t, block0);
    } else {
        switch (a.e.kind) {
            case FVVDP_EOTF_SRGB: temporal_vec_cc<FL, PX, SRC, TD, FVVDP_EOTF_SRGB, true>(a, lutw, s_t, block0); break;
            case FVVDP_EOTF_GAMMA: temporal_vec_cc<FL, PX, SRC, TD, FVVDP_EOTF_GAMMA, true>(a, lutw, s_t, block0); break;
            case FVVDP_EOTF_PQ: temporal_vec_cc<FL, PX, SRC, TD, FVVDP_EOTF_PQ, true>(a, lutw, s_t, block0); break;
            case FVVDP_EOTF_LINEAR: temporal_vec_cc<FL, PX, SRC, TD, FVVDP_EOTF_LINEAR, true>(a, lutw, s_t, block0); break;
            case FVVDP_EOTF_ABSOLUTE: temporal_vec_cc<FL, PX, SRC, TD, FVVDP_EOTF_ABSOLUTE, true>(a, lutw, s_t, block0); break;
            case FVVDP_EOTF_LUT:
                if constexpr (SRC == SRC_U16) temporal_vec_cc<FL, PX, SRC, TD, FVVDP_EOTF_LUT, true>(a, lutw, s_t, block0);
                break;                               // (a table for a float source is refused by the host side)
            default: temporal_vec_cc<FL, PX, SRC, TD, FVVDP_EOTF_NONE, true>(a, lutw, s_t, block0); break;
        }
    }
}

// the per-pixel fallback (any frame size, any alignment)
template <int FL, int PX, int SRC>
__global__ __launch_bounds__(256) void held_ring_kernel(const HeldTemporalArgs h) {
    temporal_ring_body<FL, PX, SRC, true>(h.a);
}

// ---- backward: temporal transpose + transpose of the hold + display model ------------------------------------------------------
// The transpose of transpose_kernels.hpp with a frame map between the window list and the clip.  The display-rate list has
// n_display + fl - 1 positions; position p < fl belongs to the head (what the temporal padding shows before display frame 0),
// position p >= fl shows display frame p - fl + 1, which shows SOURCE frame map[p - fl + 1].  A lane walks the positions once
// with the shared ring step; a finished head position goes to the side buffer, a finished streaming position is added to the
// running sum of the source frame it shows.  The map is non-decreasing, so the streaming positions visit the source frames in
// ascending order: when the map moves on (or the list ends) the open frame is flushed -- its head positions first (fold list keyed
// by SOURCE frame: sorted by frame, then position; the shared cursor walks it), then its streaming positions in ascending order,
// then the display model's derivative at the frame's samples -- and so is every frame in between, which no streaming position
// shows: head positions only, or exact zeros.  Every source frame is written exactly once, in ascending order, by one lane per
// pixel: no atomics, and the bits do not depend on the launch geometry.  With the identity map the sums are video_input_body's.
struct VideoInputHeldArgs {
    VideoInputArgs a;       // t.N = display frames; test / grad / strides: the SOURCE clip; t.fold_frame: SOURCE frames
    const int* map;         // [N] device: display frame -> source frame
    int n_source;
};
static_assert(offsetof(VideoInputHeldArgs, a) == 0, "transpose_step and FoldCursor read the start of the kernel-argument segment");

template <int FL, int PX, int ST>
__global__ __launch_bounds__(256) void video_input_held_kernel(const VideoInputHeldArgs h_byval) {
    // every read of the argument block goes to the kernel-argument segment itself (scalar loads; see temporal_vec_kernel)
    const VideoInputHeldArgs& h = *(const VideoInputHeldArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    (void)h_byval;
    const size_t px = ((size_t)blockIdx.x * 256 + threadIdx.x) * PX;
    if (px >= (size_t)h.a.t.HW) return;
    const int N = h.a.t.N, fl = h.a.t.fl, C = h.a.C, n_source = h.n_source;
    const size_t HW = (size_t)h.a.t.HW, frame_stride = h.a.frame_stride, chan_stride = h.a.chan_stride;
    const float* const g0 = h.a.t.g0;
    float* const head = h.a.t.head;
    const int* const map = h.map;
    const EotfDev e = h.a.e;
    const float wgt[3] = {h.a.wgt[0], h.a.wgt[1], h.a.wgt[2]};
    const float* const src = h.a.test;
    float* const grad = h.a.grad;

    // (the two helpers below are inlined at every call: left to the inliner's budget they stay functions, and their closures --
    // captured addresses and values -- live in scratch)
    FoldCursor<PX> fold(head, HW, px, fl);
    // grad_c[f] = w_c EOTF'(V_c[f]) s
    auto flush = [&](int f, const LaneVec<PX>& s) __attribute__((always_inline)) {
        const size_t o = (size_t)f * frame_stride + px;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c < C) {
                LaneVec<PX> V, r;
                if constexpr (ST == SRC_F32) V = lane_load<PX>(src + o + (size_t)c * chan_stride);
                else V = lane_load16<PX, ST>(reinterpret_cast<const unsigned short*>(src) + o + (size_t)c * chan_stride);
#pragma unroll
                for (int i = 0; i < PX; ++i) r.v[i] = wgt[c] * eotf_grad(V.v[i], e) * s.v[i];
                if constexpr (ST == SRC_F32) lane_store<PX>(grad + o + (size_t)c * chan_stride, r);
                else lane_store16<PX, ST>(reinterpret_cast<unsigned short*>(grad) + o + (size_t)c * chan_stride, r);
            }
        }
    };
    // frames [from, to): no streaming position shows them
    auto flush_unstreamed = [&](int from, int to) __attribute__((always_inline)) {
        for (int f = from; f < to; ++f) {
            LaneVec<PX> s = lane_zero<PX>();
            fold.add_heads(f, s);
            flush(f, s);
        }
    };

    TransposeRing<FL, PX> ring = transpose_ring<FL, PX>();
    int open = -1;                              // the source frame whose sum is running (-1: none yet)
    LaneVec<PX> acc = lane_zero<PX>();
    const int total = N + fl - 1;
    for (int p = 0; p < total; ++p) {
        LaneVec<PX> gs, gt;
        transpose_inputs<PX>(g0, p, N, HW, px, gs, gt);
        const LaneVec<PX> done = transpose_step<FL, PX>(ring, gs, gt);
        if (p < fl) {
            lane_store<PX>(head + (size_t)p * HW + px, done);
        } else {
            const int j = map[p - fl + 1];      // wave-uniform; checked by the host: non-decreasing, inside [0, n_source)
            if (j != open) {
                if (open >= 0) flush(open, acc);
                flush_unstreamed(open + 1, j);
                acc = lane_zero<PX>();
                fold.add_heads(j, acc);
                open = j;
            }
#pragma unroll
            for (int i = 0; i < PX; ++i) acc.v[i] += done.v[i];
        }
    }
    if (open >= 0) flush(open, acc);
    flush_unstreamed(open + 1, n_source);
}
