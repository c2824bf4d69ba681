// The temporal transpose of the clip backwards, once: what video_input_kernel (video_grad_kernels.hpp), video_lum_input_kernel
// (yuv_grad_kernels.hpp), display_video_sums_kernel (display_grad_kernels.hpp) and video_input_held_kernel (held_kernels.hpp) do
// before their own tails.  Include after temporal_kernels.hpp (TAPC, vtapf, karg_taps_p, half_widen / half_narrow).
//
// A lane owns PX consecutive pixels for the whole launch and walks the window-list positions p = 0 .. N + fl - 2 once.  Position
// p collects taps[cc][k] g0[t][cc] from the output frames t = p - (fl - 1) + k, i.e. step t adds to the positions t .. t + fl - 1;
// after step p nothing more arrives at position p.  The fl open positions live in a register ring that SHIFTS by one slot
// per step: slot m holds position p + m, and the shift is free because the multiply-add that adds step p's term to slot m
// writes its result to slot m - 1 (three-operand FMA) -- the loop over p is a plain loop, nothing is unrolled over time, and
// the code stays small whatever FL.  tapsT[m] = taps[.][fl - 1 - m] (zero for m >= fl) is the tap slot m receives.
// A finished position p < fl belongs to the head (the frames the temporal padding shows before frame 0): it goes to the side
// buffer head[p]; a finished position p >= fl is the one streaming term of frame p - fl + 1.  Frame j = p - (fl - 1) is
// complete after step p: its head positions (fold list: sorted by frame, then position -- a cursor walks it) are added in
// ascending order, then the streaming term, then the kernel's own tail -- a fixed order, no atomics.  A frame no window shows
// (circular padding, N > fl: frame 0) sums nothing and gets exact zeros.
//
// Every function here is inlined at every call: left to the inliner's budget a helper stays a function, and what it takes by
// reference -- the ring, the cursor -- lives in scratch.
#pragma once
#include "transpose_host.hpp"       // TransposeArgs, TRANSPOSE_MAX_FL

// ---- PX consecutive fp32 values of a lane, with non-temporal loads and stores ---------------------------------------------------
template <int PX>
struct LaneVec {
    float v[PX];
};
template <int PX>
__device__ __forceinline__ LaneVec<PX> lane_zero() {
    LaneVec<PX> r;
#pragma unroll
    for (int i = 0; i < PX; ++i) r.v[i] = 0.0f;
    return r;
}
// (the load writes into r in place: with the conditional form below assigning a whole loaded value, tap_grad_kernel<8, 4> takes
// four registers more)
template <int PX>
__device__ __forceinline__ void lane_read(LaneVec<PX>& r, const float* p) {
    if constexpr (PX == 4) {
        const v4f t = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else if constexpr (PX == 2) {
        const v2f t = __builtin_nontemporal_load(reinterpret_cast<const v2f*>(p));
        r.v[0] = t.x; r.v[1] = t.y;
    } else {
        r.v[0] = __builtin_nontemporal_load(p);
    }
}
template <int PX>
__device__ __forceinline__ LaneVec<PX> lane_load(const float* p) {
    LaneVec<PX> r;
    lane_read<PX>(r, p);
    return r;
}
// zeros when not live: a lane past the frame reads nothing, and stays for the shuffles and barriers of a reduction
template <int PX>
__device__ __forceinline__ LaneVec<PX> lane_load(const float* p, bool live) {
    LaneVec<PX> r = lane_zero<PX>();
    if (live) lane_read<PX>(r, p);
    return r;
}
template <int PX>
__device__ __forceinline__ void lane_store(float* p, const LaneVec<PX>& r) {
    if constexpr (PX == 4) __builtin_nontemporal_store(v4f{r.v[0], r.v[1], r.v[2], r.v[3]}, reinterpret_cast<v4f*>(p));
    else if constexpr (PX == 2) __builtin_nontemporal_store(v2f{r.v[0], r.v[1]}, reinterpret_cast<v2f*>(p));
    else __builtin_nontemporal_store(r.v[0], p);
}

// 16-bit forms for float16 / bfloat16 samples (ST = SRC_F16 / SRC_BF16): PX samples are 8 / 4 / 2 bytes, widened exactly on the
// way in and rounded once (to nearest even, float16 subnormals kept) on the way out; the same non-temporal hints
template <int PX, int ST>
__device__ __forceinline__ LaneVec<PX> lane_load16(const unsigned short* p) {
    typedef unsigned int u2v __attribute__((ext_vector_type(2)));
    LaneVec<PX> r;
    if constexpr (PX == 4) {
        const u2v t = __builtin_nontemporal_load(reinterpret_cast<const u2v*>(p));
        r.v[0] = half_widen<ST>(t.x); r.v[1] = half_widen<ST>(t.x >> 16); r.v[2] = half_widen<ST>(t.y); r.v[3] = half_widen<ST>(t.y >> 16);
    } else if constexpr (PX == 2) {
        const unsigned int t = __builtin_nontemporal_load(reinterpret_cast<const unsigned int*>(p));
        r.v[0] = half_widen<ST>(t); r.v[1] = half_widen<ST>(t >> 16);
    } else {
        r.v[0] = half_widen<ST>(__builtin_nontemporal_load(p));
    }
    return r;
}
template <int PX, int ST>
__device__ __forceinline__ void lane_store16(unsigned short* p, const LaneVec<PX>& r) {
    typedef unsigned int u2v __attribute__((ext_vector_type(2)));
    unsigned int h[PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) h[i] = half_narrow<ST>(r.v[i]);
    if constexpr (PX == 4) __builtin_nontemporal_store(u2v{h[0] | (h[1] << 16), h[2] | (h[3] << 16)}, reinterpret_cast<u2v*>(p));
    else if constexpr (PX == 2) __builtin_nontemporal_store(h[0] | (h[1] << 16), reinterpret_cast<unsigned int*>(p));
    else __builtin_nontemporal_store((unsigned short)h[0], p);
}

// ---- the ring -------------------------------------------------------------------------------------------------------------------
// FL: ring slots (fl rounded up to 8 / 16 / 32 / 64).  PX: pixels per lane (4 or 2: HW and the strides are multiples of PX and
// the pointers PX-value aligned, so a lane's pixels are all inside the frame or all outside; 1: any size).
template <int FL, int PX>
struct TransposeRing {
    float slot[FL - 1][PX];         // before step p: slot m = position p + m (slot FL - 1 is still empty: not kept)
};
template <int FL, int PX>
__device__ __forceinline__ TransposeRing<FL, PX> transpose_ring() {
    TransposeRing<FL, PX> r;
#pragma unroll
    for (int m = 0; m < FL - 1; ++m)
#pragma unroll
        for (int i = 0; i < PX; ++i) r.slot[m][i] = 0.0f;
    return r;
}

// the two gradient planes of output frame p; past the last output frame (or not live) zeros: the open positions only drain
template <int PX>
__device__ __forceinline__ void transpose_inputs(const float* g0, int p, int N, size_t HW, size_t px, LaneVec<PX>& gs, LaneVec<PX>& gt,
                                                 bool live = true) {
    const bool in = live && p < N;
    gs = lane_load<PX>(g0 + (size_t)p * 2 * HW + px, in);
    gt = lane_load<PX>(g0 + ((size_t)p * 2 + 1) * HW + px, in);
}

// One step: adds the term of output frame p to every open position and shifts the ring; returns position p, now finished.  The
// kernel's argument block starts with a TransposeArgs: the taps come straight from the kernel-argument segment with scalar loads.
template <int FL, int PX>
__device__ __forceinline__ LaneVec<PX> transpose_step(TransposeRing<FL, PX>& ring, const LaneVec<PX>& gs, const LaneVec<PX>& gt) {
    typedef const char __attribute__((address_space(4)))* karg_p;
    // taps: long rings re-read them in every step, TAPC at a time through a laundered pointer -- hoisted out of the loop,
    // 2 FL scalar values would stay alive and spill (see temporal_ring_kernel)
    karg_p tp = (karg_p)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(TransposeArgs, tapsT);
    if constexpr (FL > 8) asm volatile("" : "+s"(tp));
    LaneVec<PX> done;                           // position p
#pragma unroll
    for (int c = 0; c < FL / TAPC; ++c) {
        karg_p tpc = tp + c * (8 * TAPC);
        if constexpr (FL > 16) asm volatile("" : "+s"(tpc));       // (else the chunks' loads are merged back into one)
        const vtapf tc = *(karg_taps_p)tpc;
#pragma unroll
        for (int kk = 0; kk < TAPC; ++kk) {
            const int m = c * TAPC + kk;
            const float fs = tc[2 * kk], ft = tc[2 * kk + 1];
#pragma unroll
            for (int i = 0; i < PX; ++i) {
                const float old = m < FL - 1 ? ring.slot[m][i] : 0.0f;
                float v = fmaf(fs, gs.v[i], fmaf(ft, gt.v[i], old));
                asm volatile("" : "+v"(v));             // pinned where it is produced: left alone, the compiler sinks the ring
                                                        // updates below the branches that follow and keeps every tap alive
                if (m == 0) done.v[i] = v;              // position p: nothing more arrives
                else ring.slot[m - 1][i] = v;           // the shift: slot m becomes slot m - 1 of the next step
            }
        }
        if constexpr (FL > 8) __builtin_amdgcn_sched_barrier(0);      // one chunk of taps in scalar registers at a time
    }
    return done;
}

// ---- the fold cursor --------------------------------------------------------------------------------------------------------------
// Walks the fold list of the kernel-argument segment (scalar loads, no copy of the block to scratch); wave-uniform.
template <int PX>
struct FoldCursor {
    const float* head;      // the lane's pixels of the side buffer: head + px
    size_t HW;
    int fl;
    bool live;
    int cur;

    __device__ __forceinline__ FoldCursor(const float* head_, size_t HW_, size_t px, int fl_, bool live_ = true)
        : head(head_ + px), HW(HW_), fl(fl_), live(live_), cur(0) {}

    // adds the head positions of `frame` to s in ascending order; frames are asked for in ascending order
    __device__ __forceinline__ void add_heads(int frame, LaneVec<PX>& s) {
        typedef const int __attribute__((address_space(4)))* karg_int_p;
        typedef const char __attribute__((address_space(4)))* karg_p;
        const karg_p ka = (karg_p)__builtin_amdgcn_kernarg_segment_ptr();
        const karg_int_p fold_frame = (karg_int_p)(ka + offsetof(TransposeArgs, fold_frame));
        const karg_int_p fold_pos = (karg_int_p)(ka + offsetof(TransposeArgs, fold_pos));
        while (cur < fl && fold_frame[cur] == frame) {
            const LaneVec<PX> hd = lane_load<PX>(head + (size_t)fold_pos[cur] * HW, live);
#pragma unroll
            for (int i = 0; i < PX; ++i) s.v[i] += hd.v[i];
            ++cur;
        }
    }

    // the sum of frame j >= 0 where every position shows its own frame: the head positions, then (j >= 1) the streaming position
    // that has just finished
    __device__ __forceinline__ LaneVec<PX> frame_sum(int j, const LaneVec<PX>& done) {
        LaneVec<PX> s = lane_zero<PX>();
        add_heads(j, s);
        if (j >= 1) {
#pragma unroll
            for (int i = 0; i < PX; ++i) s.v[i] += done.v[i];
        }
        return s;
    }
};

// ---- the block of the two kernels whose tail is the display model's derivative -------------------------------------------------
// video_input_kernel (video_grad_kernels.hpp) and, with a frame map behind it, video_input_held_kernel (held_kernels.hpp)
struct VideoInputArgs {
    TransposeArgs t;        // g0, head, sizes, taps and fold list
    const float* test;      // element (c, f, px) at c * chan_stride + f * frame_stride + px
    float* grad;            // the same layout
    size_t chan_stride, frame_stride;
    int C;
    EotfDev e;
    float wgt[3];
};
static_assert(offsetof(VideoInputArgs, t) == 0, "transpose_step and FoldCursor read the start of the kernel-argument segment");
