// Host code the four clip backwards share for their temporal transpose (fvvdp_video_grad_input_st, fvvdp_video_grad_luminance,
// fvvdp_video_display_sums, fvvdp_video_grad_input_held; the device side is transpose_kernels.hpp): the argument block, the ring
// length and pixels per lane of a filter, the rule for the vector variant, the checks of the fold list and of the side buffer,
// and the fill of the block.  Host code only, and no HIP header: a plain C++ program can include it
// (tests/transpose_host_check.cpp does).  A check cannot reach the library's error message from here; it returns a verdict
// that the entry point hands to grad_verdict (grad_host.hpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "fvvdp_hip.h"

// the longest register ring: FVVDP_VIDEO_GRAD_MAX_TAPS of the public headers (asserted by the units that include them)
static constexpr int TRANSPOSE_MAX_FL = 64;

// What the transpose reads.  The first member of every argument block that has one (VideoInputArgs, LumInputArgs,
// DisplayVideoSumsArgs and, through VideoInputArgs, VideoInputHeldArgs), so that the taps and the fold list have one offset in
// the kernel-argument segment whatever the kernel.
struct TransposeArgs {
    const float* g0;        // [N][2][HW]
    float* head;            // [fl][HW]
    int HW, N, fl;
    float tapsT[TRANSPOSE_MAX_FL][2];       // {sustained, transient} tap of ring slot m
    int fold_frame[TRANSPOSE_MAX_FL];       // [fl] sorted; padded with -1
    int fold_pos[TRANSPOSE_MAX_FL];
};

// FL: the ring slots of a filter of fl taps, for kernels instantiated up to max_FL (32 or 64) slots
static constexpr int transpose_ring_length(int fl, int max_FL) {
    return fl <= 8 ? 8 : (fl <= 16 ? 16 : ((fl <= 32 || max_FL <= 32) ? 32 : 64));
}
// pixels per lane of the vector variant: the ring is FL x PX registers
static constexpr int transpose_px(int FL) { return FL <= 16 ? 4 : 2; }

// The vector variant needs a lane's transpose_px(FL) consecutive values naturally aligned wherever it reads or writes them.
// strides: every element stride of the caller, or-ed.  fp32_ptrs: the fp32 buffers, or-ed.  sample_ptrs: the caller's samples
// and gradient of es bytes each, or-ed (0: none).
static inline bool transpose_vector_ok(int FL, size_t HW, size_t strides, uintptr_t fp32_ptrs, uintptr_t sample_ptrs = 0,
                                       size_t es = 4) {
    const size_t pxv = (size_t)transpose_px(FL);
    return HW % pxv == 0 && strides % pxv == 0 && fp32_ptrs % (4 * pxv) == 0 && sample_ptrs % (es * pxv) == 0;
}

// FVVDP_OK, or the code and the text of a refusal
struct TransposeVerdict {
    int code;
    char msg[160];
};
static inline TransposeVerdict transpose_ok() {
    TransposeVerdict v;
    v.code = FVVDP_OK;
    v.msg[0] = 0;
    return v;
}
#define TRANSPOSE_REFUSE(...)                          \
    do {                                               \
        TransposeVerdict v_;                           \
        v_.code = FVVDP_EINVAL;                        \
        snprintf(v_.msg, sizeof(v_.msg), __VA_ARGS__); \
        return v_;                                     \
    } while (0)

// The fold list: every head position exactly once, frames inside the clip, sorted by frame and then by position.  what: "frame",
// or "source frame" where a frame map lies between the window list and the clip.
static inline TransposeVerdict transpose_check_fold(const int32_t* fold_frame, const int32_t* fold_pos, int fl, int n_frames,
                                                    const char* what) {
    bool seen[TRANSPOSE_MAX_FL] = {false};
    for (int i = 0; i < fl; ++i) {
        const int f = fold_frame[i], p = fold_pos[i];
        if (f < 0 || f >= n_frames) TRANSPOSE_REFUSE("fold list entry %d names %s %d outside [0, %d)", i, what, f, n_frames);
        if (p < 0 || p >= fl || seen[p])
            TRANSPOSE_REFUSE("fold list entry %d: head position %d is outside [0, %d) or listed twice", i, p, fl);
        seen[p] = true;
        if (i > 0 && (f < fold_frame[i - 1] || (f == fold_frame[i - 1] && p < fold_pos[i - 1])))
            TRANSPOSE_REFUSE("fold list must be sorted by frame, then by position (entry %d)", i);
    }
    return transpose_ok();
}

// the side buffer: fl fp32 frames behind what the caller keeps in front of them (before: bytes)
static inline TransposeVerdict transpose_check_head_bytes(size_t head_bytes, int fl, size_t HW, size_t before = 0) {
    const size_t need = before + (size_t)fl * HW * sizeof(float);
    if (head_bytes < need) TRANSPOSE_REFUSE("side buffer of %zu bytes is below the %zu needed", head_bytes, need);
    return transpose_ok();
}
#undef TRANSPOSE_REFUSE

// the transpose's part of a zeroed argument block
static inline void transpose_fill(TransposeArgs& t, const float* d_g0, float* d_head, size_t HW, int n_frames, int fl,
                                  const float* h_taps, const int32_t* h_fold_frame, const int32_t* h_fold_pos) {
    t.g0 = d_g0;
    t.head = d_head;
    t.HW = (int)HW;
    t.N = n_frames;
    t.fl = fl;
    for (int m = 0; m < fl; ++m) {                  // ring slot m of step p is position p + m: it receives tap fl - 1 - m
        t.tapsT[m][0] = h_taps[fl - 1 - m];
        t.tapsT[m][1] = h_taps[fl + fl - 1 - m];
    }
    for (int i = 0; i < TRANSPOSE_MAX_FL; ++i) {
        t.fold_frame[i] = i < fl ? h_fold_frame[i] : -1;
        t.fold_pos[i] = i < fl ? h_fold_pos[i] : 0;
    }
}

// f(std::integral_constant<int, FL>) for the ring length FL of a filter, among the lengths up to MAX_FL that the caller instantiates
template <int MAX_FL, class F>
static void transpose_dispatch(int FL, F&& f) {
    static_assert(MAX_FL == 32 || MAX_FL == 64, "8 / 16 / 32 slots, or 64 as well");
    if (FL == 8) f(std::integral_constant<int, 8>());
    else if (FL == 16) f(std::integral_constant<int, 16>());
    else if (FL == 32 || MAX_FL == 32) f(std::integral_constant<int, 32>());
    else if constexpr (MAX_FL == 64) f(std::integral_constant<int, 64>());
}
