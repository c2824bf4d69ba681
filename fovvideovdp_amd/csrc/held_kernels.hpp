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
// video_input_body (video_grad_kernels.hpp) with a frame map between the window list and the clip.  The display-rate list has
// n_display + fl - 1 positions; position p < fl belongs to the head (what the temporal padding shows before display frame 0),
// position p >= fl shows display frame p - fl + 1, which shows SOURCE frame map[p - fl + 1].  A lane owns PX consecutive pixels for
// the whole launch and walks the positions once with the same register ring, the same taps from the kernel-argument segment and
// the same multiply-add chain; a finished head position goes to the side buffer, a finished streaming position is added to the
// running sum of the source frame it shows.  The map is non-decreasing, so the streaming positions visit the source frames in
// ascending order: when the map moves on (or the list ends) the open frame is flushed -- its head positions first (fold list keyed
// by SOURCE frame: sorted by frame, then position; a cursor walks it), then its streaming positions in ascending order, then the
// display model's derivative at the frame's samples -- and so is every frame in between, which no streaming position shows: head
// positions only, or exact zeros.  Every source frame is written exactly once, in ascending order, by one lane per pixel: no
// atomics, and the bits do not depend on the launch geometry.  With the identity map the sums are video_input_body's.
struct VideoInputHeldArgs {
    VideoInputArgs a;       // N = display frames; test / grad / strides: the SOURCE clip; fold_frame: SOURCE frames
    const int* map;         // [N] device: display frame -> source frame
    int n_source;
};

template <int FL, int PX, int ST>
__global__ __launch_bounds__(256) void video_input_held_kernel(const VideoInputHeldArgs h_byval) {
    // every read of the argument block goes to the kernel-argument segment itself (scalar loads; see temporal_vec_kernel)
    const VideoInputHeldArgs& h = *(const VideoInputHeldArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    (void)h_byval;
    const size_t px = ((size_t)blockIdx.x * 256 + threadIdx.x) * PX;
    if (px >= (size_t)h.a.HW) return;
    // fold list and (long rings) taps straight from the kernel-argument segment, as video_input_body
    typedef const int __attribute__((address_space(4)))* karg_int_p;
    typedef const char __attribute__((address_space(4)))* karg_p;
    const karg_p ka = (karg_p)__builtin_amdgcn_kernarg_segment_ptr();
    const karg_int_p fold_frame = (karg_int_p)(ka + offsetof(VideoInputArgs, fold_frame));
    const karg_int_p fold_pos = (karg_int_p)(ka + offsetof(VideoInputArgs, fold_pos));
    static_assert(offsetof(VideoInputHeldArgs, a) == 0, "the block starts the kernel-argument segment");
    const int N = h.a.N, fl = h.a.fl, C = h.a.C, n_source = h.n_source;
    const size_t HW = (size_t)h.a.HW, frame_stride = h.a.frame_stride, chan_stride = h.a.chan_stride;
    const float* const g0 = h.a.g0;
    float* const head = h.a.head;
    const int* const map = h.map;
    const EotfDev e = h.a.e;
    const float wgt[3] = {h.a.wgt[0], h.a.wgt[1], h.a.wgt[2]};
    const float* const src = h.a.test;
    float* const grad = h.a.grad;

    // (the three helpers below are inlined at every call: left to the inliner's budget they stay functions, and their closures --
    // 272 bytes of captured addresses and values -- live in scratch)
    int cur = 0;                                // cursor in the fold list (wave-uniform)
    // s = the head positions of source frame f in ascending order, added to `s` as it comes
    auto add_heads = [&](int f, VgVec<PX>& s) __attribute__((always_inline)) {
        while (cur < fl && fold_frame[cur] == f) {
            const VgVec<PX> hd = vg_load<PX>(head + (size_t)fold_pos[cur] * HW + px);
#pragma unroll
            for (int i = 0; i < PX; ++i) s.v[i] += hd.v[i];
            ++cur;
        }
    };
    // grad_c[f] = w_c EOTF'(V_c[f]) s
    auto flush = [&](int f, const VgVec<PX>& s) __attribute__((always_inline)) {
        const size_t o = (size_t)f * frame_stride + px;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c < C) {
                VgVec<PX> V, r;
                if constexpr (ST == SRC_F32) V = vg_load<PX>(src + o + (size_t)c * chan_stride);
                else V = vg_load16<PX, ST>(reinterpret_cast<const unsigned short*>(src) + o + (size_t)c * chan_stride);
#pragma unroll
                for (int i = 0; i < PX; ++i) r.v[i] = wgt[c] * eotf_grad(V.v[i], e) * s.v[i];
                if constexpr (ST == SRC_F32) vg_store<PX>(grad + o + (size_t)c * chan_stride, r);
                else vg_store16<PX, ST>(reinterpret_cast<unsigned short*>(grad) + o + (size_t)c * chan_stride, r);
            }
        }
    };
    // frames [from, to): no streaming position shows them
    auto flush_unstreamed = [&](int from, int to) __attribute__((always_inline)) {
        for (int f = from; f < to; ++f) {
            VgVec<PX> s;
#pragma unroll
            for (int i = 0; i < PX; ++i) s.v[i] = 0.0f;
            add_heads(f, s);
            flush(f, s);
        }
    };

    float ring[FL - 1][PX];                     // before step p: slot m = position p + m
#pragma unroll
    for (int m = 0; m < FL - 1; ++m)
#pragma unroll
        for (int i = 0; i < PX; ++i) ring[m][i] = 0.0f;
    int open = -1;                              // the source frame whose sum is running (-1: none yet)
    VgVec<PX> acc;
#pragma unroll
    for (int i = 0; i < PX; ++i) acc.v[i] = 0.0f;
    const int total = N + fl - 1;
    for (int p = 0; p < total; ++p) {
        VgVec<PX> gs, gt;
        if (p < N) {
            gs = vg_load<PX>(g0 + (size_t)p * 2 * HW + px);
            gt = vg_load<PX>(g0 + ((size_t)p * 2 + 1) * HW + px);
        } else {                                // past the last display frame: the open positions only drain
#pragma unroll
            for (int i = 0; i < PX; ++i) gs.v[i] = gt.v[i] = 0.0f;
        }
        // taps: as video_input_body (chunks through a laundered pointer, one chunk in scalar registers at a time)
        karg_p tp = ka + offsetof(VideoInputArgs, tapsT);
        if constexpr (FL > 8) asm volatile("" : "+s"(tp));
        VgVec<PX> done;                         // position p
#pragma unroll
        for (int c = 0; c < FL / TAPC; ++c) {
            karg_p tpc = tp + c * (8 * TAPC);
            if constexpr (FL > 16) asm volatile("" : "+s"(tpc));
            const vtapf tc = *(karg_taps_p)tpc;
#pragma unroll
            for (int kk = 0; kk < TAPC; ++kk) {
                const int m = c * TAPC + kk;
                const float fs = tc[2 * kk], ft = tc[2 * kk + 1];
#pragma unroll
                for (int i = 0; i < PX; ++i) {
                    const float old = m < FL - 1 ? ring[m][i] : 0.0f;
                    float v = fmaf(fs, gs.v[i], fmaf(ft, gt.v[i], old));
                    asm volatile("" : "+v"(v));             // pinned where it is produced (see video_input_body)
                    if (m == 0) done.v[i] = v;
                    else ring[m - 1][i] = v;
                }
            }
            if constexpr (FL > 8) __builtin_amdgcn_sched_barrier(0);
        }
        if (p < fl) {
            vg_store<PX>(head + (size_t)p * HW + px, done);
        } else {
            const int j = map[p - fl + 1];      // wave-uniform; checked by the host: non-decreasing, inside [0, n_source)
            if (j != open) {
                if (open >= 0) flush(open, acc);
                flush_unstreamed(open + 1, j);
#pragma unroll
                for (int i = 0; i < PX; ++i) acc.v[i] = 0.0f;
                add_heads(j, acc);
                open = j;
            }
#pragma unroll
            for (int i = 0; i < PX; ++i) acc.v[i] += done.v[i];
        }
    }
    if (open >= 0) flush(open, acc);
    flush_unstreamed(open + 1, n_source);
}
