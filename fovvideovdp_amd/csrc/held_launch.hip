// Clips whose streams have frame counts of their own (include/fvvdp_hip_held.h): argument checks and launches of the kernels of
// held_kernels.hpp.  Compiled once per HELD_PART, as temporal_launch.hip is per K1_PART: parts 0..4 instantiate the held ingest for
// one sample type each (uint8, uint16, float32, float16, bfloat16 -- the ring bodies are fully unrolled per ring length, channel
// count and display model); part 5 holds the C ABI, the dispatcher and the backward's kernel.  The one function that needs a
// context asks fvvdp_hip.hip for the context's side of the call (fvvdp_ctx_ingest_begin).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "fvvdp_hip.h"
#include "fvvdp_hip_held.h"
#include "device_common.hpp"
#include "temporal_launch.hpp"
#include "grad_common.hpp"
#include "transpose_kernels.hpp"   // the shared transpose and VideoInputArgs; no kernel of the video backward
#include "held_kernels.hpp"
#include "grad_host.hpp"

#ifndef HELD_PART
#error "compile with -DHELD_PART=0..5"
#endif

#if HELD_PART != 5
static constexpr int SRC = HELD_PART;            // SRC_U8 ... SRC_BF16 = FVVDP_U8 ... FVVDP_BF16
static_assert(SRC_U8 == FVVDP_U8 && SRC_BF16 == FVVDP_BF16, "the kernels' sample types are numbered as the ABI's");

template <int FL>
static void launch_vec(const HeldTemporalArgs& h, hipStream_t st) {
    constexpr int PX = k1_px(FL);
    constexpr int WPB = k1_wpb(FL);
    const int n_blocks = (h.a.HW + 64 * PX - 1) / (64 * PX);
    hipLaunchKernelGGL((held_vec_kernel<FL, PX, SRC>), dim3((n_blocks + WPB - 1) / WPB), dim3(64 * WPB), 0, st, h);
}
template <int FL, int PX>
static void launch_ring(const HeldTemporalArgs& h, hipStream_t st) {
    hipLaunchKernelGGL((held_ring_kernel<FL, PX, SRC>), dim3((h.a.HW + 256 * PX - 1) / (256 * PX)), dim3(256), 0, st, h);
}

#if HELD_PART == 0
#define HELD_NAME(f) f##_u8
#elif HELD_PART == 1
#define HELD_NAME(f) f##_u16
#elif HELD_PART == 2
#define HELD_NAME(f) f##_f32
#elif HELD_PART == 3
#define HELD_NAME(f) f##_f16
#else
#define HELD_NAME(f) f##_bf16
#endif
// FL in {8, 16, 32}; vec: the vector variant (aligned sizes), else the per-pixel ring with temporal_launch.hip's pixels per lane
void HELD_NAME(held_ingest)(int FL, bool vec, const HeldTemporalArgs& h, hipStream_t st) {
    if (vec) {
        if (FL == 8) launch_vec<8>(h, st);
        else if (FL == 16) launch_vec<16>(h, st);
        else launch_vec<32>(h, st);
    } else {
        if (FL == 8) launch_ring<8, 4>(h, st);
        else if (FL == 16) launch_ring<16, 4>(h, st);
        else launch_ring<32, 2>(h, st);
    }
}
#endif

#if HELD_PART == 5
static_assert(FVVDP_HELD_MAX_TAPS == 32, "ring lengths 8 / 16 / 32");
static_assert(FVVDP_HELD_MAX_TAPS <= TRANSPOSE_MAX_FL, "TransposeArgs::tapsT");

void held_ingest_u8(int, bool, const HeldTemporalArgs&, hipStream_t);
void held_ingest_u16(int, bool, const HeldTemporalArgs&, hipStream_t);
void held_ingest_f32(int, bool, const HeldTemporalArgs&, hipStream_t);
void held_ingest_f16(int, bool, const HeldTemporalArgs&, hipStream_t);
void held_ingest_bf16(int, bool, const HeldTemporalArgs&, hipStream_t);

static int check_fl(int fl, const char* what) {
    if (fl < 1 || fl > FVVDP_MAX_TAPS) return grad_fail(FVVDP_EINVAL, "filter length %d outside [1, %d]", fl, FVVDP_MAX_TAPS);
    if (fl > FVVDP_HELD_MAX_TAPS)
        return grad_fail(FVVDP_EUNSUPPORTED, "%s covers temporal filters of up to %d taps (128 frames per second); this one has %d",
                         what, FVVDP_HELD_MAX_TAPS, fl);
    return FVVDP_OK;
}

static int check_stream(const fvvdp_held_stream* s, const char* what, int C, size_t HW, size_t es) {
    if (!s->d_data) return grad_fail(FVVDP_EINVAL, "null data pointer (%s)", what);
    if (reinterpret_cast<uintptr_t>(s->d_data) % es != 0)
        return grad_fail(FVVDP_EINVAL, "data pointer must be aligned to its %zu-byte samples (%s)", es, what);
    if (s->n_frames < 1) return grad_fail(FVVDP_EINVAL, "a stream needs at least one frame (%s: %d)", what, s->n_frames);
    if (s->frame_stride < HW) return grad_fail(FVVDP_EINVAL, "frame_stride %zu is below the frame size %zu (%s)", s->frame_stride, HW, what);
    if (C == 3 && s->chan_stride < HW) return grad_fail(FVVDP_EINVAL, "chan_stride %zu is below the frame size %zu (%s)", s->chan_stride, HW, what);
    return FVVDP_OK;
}

extern "C" int fvvdp_temporal_channels_held(fvvdp_ctx* ctx, const fvvdp_held_stream* test, const fvvdp_held_stream* ref, int dtype,
                                            int C, const fvvdp_eotf* eotf, const float* h_rgb2y, const int32_t* h_idx_test,
                                            const int32_t* h_idx_ref, const float* h_taps, int fl, int n_out, int slot0,
                                            int32_t* d_oob_flag, void* stream) {
    if (!ctx || !test || !ref || !eotf || !h_idx_test || !h_idx_ref || !h_taps) return grad_fail(FVVDP_EINVAL, "null argument");
    if (dtype < FVVDP_U8 || dtype > FVVDP_BF16)
        return grad_fail(FVVDP_EINVAL, "Only uint8, uint16 and float32 (and float16, bfloat16 read as float32) is currently supported");
    GRAD_CHECK(grad_check_channels(C, h_rgb2y));
    GRAD_CHECK(check_fl(fl, "the held-frame ingest"));
    if (eotf->kind == FVVDP_EOTF_LUT && (dtype >= FVVDP_F32 || !eotf->d_lut))
        return grad_fail(FVVDP_EINVAL, "FVVDP_EOTF_LUT needs an integer source and a table");
    if (eotf->kind != FVVDP_EOTF_LUT && dtype == FVVDP_U8)
        return grad_fail(FVVDP_EINVAL, "uint8 sources need FVVDP_EOTF_LUT (uint16: table or closed form)");
    if (eotf->kind < FVVDP_EOTF_LUT || eotf->kind > FVVDP_EOTF_NONE) return grad_fail(FVVDP_EINVAL, "unknown display model %d", eotf->kind);
    if (n_out < 1) return grad_fail(FVVDP_EINVAL, "n_out %d: at least one output frame", n_out);
    // every index inside its stream: the kernels read frame idx * frame_stride without a further check
    for (int u = 0; u < fl - 1 + n_out; ++u) {
        if (h_idx_test[u] < 0 || h_idx_test[u] >= test->n_frames)
            return grad_fail(FVVDP_EINVAL, "list entry %d names frame %d outside the test's [0, %d)", u, h_idx_test[u], test->n_frames);
        if (h_idx_ref[u] < 0 || h_idx_ref[u] >= ref->n_frames)
            return grad_fail(FVVDP_EINVAL, "list entry %d names frame %d outside the reference's [0, %d)", u, h_idx_ref[u], ref->n_frames);
    }
    IngestBegin b;
    GRAD_CHECK(fvvdp_ctx_ingest_begin(ctx, "the held-frame ingest", false, C, eotf, h_rgb2y, h_taps, fl, n_out, slot0, &b));
    const int HW = b.W * b.H;
    const size_t es = ingest_sample_bytes(dtype);
    GRAD_CHECK(check_stream(test, "test", C, (size_t)HW, es));
    GRAD_CHECK(check_stream(ref, "reference", C, (size_t)HW, es));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    const int FL = ingest_ring_length(fl);
    for (const IngestWindow wnd : IngestWindows(fl, n_out)) {
        HeldTemporalArgs h;
        memset(&h, 0, sizeof(h));
        TemporalArgs& a = h.a;
        a.src[0] = test->d_data;
        a.src[1] = ref->d_data;
        a.chan_stride = C == 3 ? test->chan_stride : 0;
        a.frame_stride = test->frame_stride;
        h.chan_stride1 = C == 3 ? ref->chan_stride : 0;
        h.frame_stride1 = ref->frame_stride;
        a.C = C;
        a.HW = HW;
        a.e = b.e;
        ingest_fill_weights(a.w, C, h_rgb2y);
        a.out = b.out;
        a.oob = d_oob_flag;
        ingest_fill_window(a, wnd, slot0, h_taps, fl, h_idx_test, h_idx_ref);       // (both lists are checked above)
        // the vector variant needs a lane's PX consecutive samples naturally aligned, in both streams
        const size_t PXv = (size_t)k1_px(FL);
        const bool vec = !b.scalar && (size_t)HW % PXv == 0 && (size_t)HW >= PXv &&
                         (a.chan_stride | a.frame_stride | h.chan_stride1 | h.frame_stride1) % PXv == 0 &&
                         (reinterpret_cast<uintptr_t>(test->d_data) | reinterpret_cast<uintptr_t>(ref->d_data)) % (es * PXv) == 0;
        switch (dtype) {
            case FVVDP_U8: held_ingest_u8(FL, vec, h, st); break;
            case FVVDP_U16: held_ingest_u16(FL, vec, h, st); break;
            case FVVDP_F16: held_ingest_f16(FL, vec, h, st); break;
            case FVVDP_BF16: held_ingest_bf16(FL, vec, h, st); break;
            default: held_ingest_f32(FL, vec, h, st); break;
        }
        GRAD_HIP_TRY(hipGetLastError());
        if (b.debug)                                // tests: which kernel this launch ran
            fprintf(stderr, "fvvdp: held ingest: %s, FL %d, fl %d, dtype %d, C %d, eotf kind %d, n_out %d, t0 %d\n",
                    vec ? "vector" : "per-pixel", FL, fl, dtype, C, eotf->kind, wnd.nn, wnd.t0);
    }
    return FVVDP_OK;
}

template <int FL, int ST>
static void launch_input(const VideoInputHeldArgs& ia, bool vec, hipStream_t st) {
    constexpr int PXV = transpose_px(FL);
    const size_t HW = (size_t)ia.a.t.HW;
    if (vec) hipLaunchKernelGGL((video_input_held_kernel<FL, PXV, ST>), dim3((unsigned int)((HW / PXV + 255) / 256)), dim3(256), 0, st, ia);
    else hipLaunchKernelGGL((video_input_held_kernel<FL, 1, ST>), dim3((unsigned int)((HW + 255) / 256)), dim3(256), 0, st, ia);
}

extern "C" int fvvdp_video_grad_input_held(int width, int height, int n_display, int n_source, const float* d_g0, const int32_t* h_map,
                                           const int32_t* h_fold_frame, const int32_t* h_fold_pos, const float* h_taps, int fl,
                                           const void* d_src, void* d_grad, int dtype, int C, size_t chan_stride, size_t frame_stride,
                                           const fvvdp_eotf* eotf, const float* h_rgb2y, void* d_head, size_t head_bytes,
                                           void* stream) {
    if (!d_g0 || !h_map || !h_fold_frame || !h_fold_pos || !h_taps || !d_src || !d_grad || !eotf || !d_head)
        return grad_fail(FVVDP_EINVAL, "null argument");
    if (width < 1 || height < 1 || n_display < 1 || n_source < 1)
        return grad_fail(FVVDP_EINVAL, "bad shape %dx%d, %d display frames, %d source frames", width, height, n_display, n_source);
    size_t es = 4;
    GRAD_CHECK(grad_check_sample_type(dtype, &es));
    const size_t HW = (size_t)width * height;
    if (HW > 0x7FFFFFFFu) return grad_fail(FVVDP_EINVAL, "frame of %zu pixels is too large", HW);
    GRAD_CHECK(check_fl(fl, "the held-frame backward"));
    GRAD_CHECK(grad_check_channels(C, h_rgb2y));
    if (frame_stride < HW) return grad_fail(FVVDP_EINVAL, "frame_stride %zu is below the frame size %zu", frame_stride, HW);
    if (C == 3 && chan_stride < HW) return grad_fail(FVVDP_EINVAL, "chan_stride %zu is below the frame size %zu", chan_stride, HW);
    GRAD_CHECK(grad_check_closed_form(eotf));
    // the map: the kernel writes frame h_map[v] without a further check, and flushes frames in the order the map visits them
    for (int v = 0; v < n_display; ++v) {
        if (h_map[v] < 0 || h_map[v] >= n_source)
            return grad_fail(FVVDP_EINVAL, "frame map entry %d names source frame %d outside [0, %d)", v, h_map[v], n_source);
        if (v > 0 && h_map[v] < h_map[v - 1])
            return grad_fail(FVVDP_EINVAL, "frame map must be non-decreasing (entry %d: %d after %d)", v, h_map[v], h_map[v - 1]);
    }
    GRAD_CHECK(grad_verdict(transpose_check_fold(h_fold_frame, h_fold_pos, fl, n_source, "source frame")));
    if (reinterpret_cast<uintptr_t>(d_head) % 256 != 0) return grad_fail(FVVDP_EINVAL, "side buffer must be 256-byte aligned");
    const size_t mb = FVVDP_HELD_MAP_BYTES(n_display);
    GRAD_CHECK(grad_verdict(transpose_check_head_bytes(head_bytes, fl, HW, mb)));
    const uintptr_t sptrs = reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_grad);
    if (reinterpret_cast<uintptr_t>(d_g0) % 4 != 0 || sptrs % es != 0)
        return grad_fail(FVVDP_EINVAL, es == 4 ? "device pointers must be aligned to 4 bytes"
                                               : "device pointers must be aligned to 4 bytes (16-bit samples and gradient: 2 bytes)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    // the host copy of the map is the thread's own and outlives the call (fvvdp_resize_grad's tables); two of them in turn, for the
    // two calls that a backward for both streams makes back to back
    static thread_local std::vector<int32_t> maps[2];
    static thread_local int turn = 0;
    std::vector<int32_t>& map = maps[turn ^= 1];
    map.assign(h_map, h_map + n_display);
    GRAD_HIP_TRY(hipMemcpyAsync(d_head, map.data(), (size_t)n_display * sizeof(int32_t), hipMemcpyHostToDevice, st));

    VideoInputHeldArgs ha;
    memset(&ha, 0, sizeof(ha));
    VideoInputArgs& ia = ha.a;
    transpose_fill(ia.t, d_g0, reinterpret_cast<float*>(static_cast<char*>(d_head) + mb), HW, n_display, fl, h_taps, h_fold_frame,
                   h_fold_pos);
    ia.test = static_cast<const float*>(d_src);       // (16-bit samples: the kernel reads and writes them as such)
    ia.grad = static_cast<float*>(d_grad);
    ia.chan_stride = C == 3 ? chan_stride : 0;
    ia.frame_stride = frame_stride;
    ia.C = C;
    grad_fill_eotf(ia.e, ia.wgt, eotf, C, h_rgb2y);
    ha.map = static_cast<const int*>(d_head);
    ha.n_source = n_source;
    const int FL = transpose_ring_length(fl, FVVDP_HELD_MAX_TAPS);
    // (the side buffer is 256-byte aligned and the map in front of it a multiple of 256 bytes)
    const bool vec = transpose_vector_ok(FL, HW, frame_stride | ia.chan_stride, reinterpret_cast<uintptr_t>(d_g0), sptrs, es);
    transpose_dispatch<FVVDP_HELD_MAX_TAPS>(FL, [&](auto c) {
        if (dtype == FVVDP_F16) launch_input<c.value, SRC_F16>(ha, vec, st);
        else if (dtype == FVVDP_BF16) launch_input<c.value, SRC_BF16>(ha, vec, st);
        else launch_input<c.value, SRC_F32>(ha, vec, st);
    });
    GRAD_HIP_TRY(hipGetLastError());
    return FVVDP_OK;
}
#endif
