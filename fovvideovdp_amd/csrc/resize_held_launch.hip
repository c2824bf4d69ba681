// Clips whose streams have frame sizes and frame counts of their own (include/fvvdp_hip_resize_held.h): argument checks and
// launches of the hold variants of resize_clip_kernels.hpp -- resized_hold_ring_kernel and resize_adjoint_run_d_kernel.  A
// translation unit beside resize_launch.hip, built with the same flags (-ffp-contract=off: the ingest must round as that unit's
// does, and the first stage of the adjoint must decide the clip as the forward decided it).  It instantiates no kernel of another
// unit: the gather of the adjoint is launched through resize_launch_gather (resize_host.hpp), and the one function that needs a
// context asks fvvdp_hip.hip for the context's side of the call (fvvdp_ctx_ingest_begin).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "fvvdp_hip.h"
#include "fvvdp_hip_resize_held.h"
#include "device_common.hpp"
#include "temporal_launch.hpp"     // fvvdp_ctx_ingest_begin
#include "grad_common.hpp"
#include "resize_clip_kernels.hpp"
#include "grad_host.hpp"
#include "resize_host.hpp"

static_assert(FVVDP_RESIZE_MAX_TAPS == 32, "ResizedArgs::taps2");
static_assert(sizeof(ResizedHoldArgs) <= 4096, "the kernel-argument segment");

template <int FL, int MODE>
static void launch_ring_mode(const ResizedHoldArgs& h, hipStream_t st) {
    constexpr int PX = resize_ring_px(FL, MODE);              // today's rule
    const size_t HW = (size_t)h.a.Wo * h.a.Ho;
    const dim3 grid((unsigned int)((HW + 256 * PX - 1) / (256 * PX))), block(256);
    hipLaunchKernelGGL((resized_hold_ring_kernel<FL, PX, MODE>), grid, block, 0, st, h);
}
template <int FL>
static void launch_ring(int mode, const ResizedHoldArgs& h, hipStream_t st) {
    switch (mode) {
        case FVVDP_RESIZE_NEAREST: launch_ring_mode<FL, FVVDP_RESIZE_NEAREST>(h, st); break;
        case FVVDP_RESIZE_BILINEAR: launch_ring_mode<FL, FVVDP_RESIZE_BILINEAR>(h, st); break;
        case FVVDP_RESIZE_BICUBIC: launch_ring_mode<FL, FVVDP_RESIZE_BICUBIC>(h, st); break;
        default: launch_ring_mode<FL, FVVDP_RESIZE_AREA>(h, st); break;
    }
}

extern "C" int fvvdp_temporal_channels_resized_held(fvvdp_ctx* ctx, const fvvdp_resize_stream* test, const fvvdp_resize_stream* ref,
                                                    int test_frames, int ref_frames, int mode, const fvvdp_eotf* eotf,
                                                    const float* h_rgb2y, const int32_t* h_idx_test, const int32_t* h_idx_ref,
                                                    const float* h_taps, int fl, int n_out, int slot0, void* stream) {
    if (!ctx || !test || !ref || !eotf || !h_rgb2y || !h_idx_test || !h_idx_ref || !h_taps) return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(resize_check_ingest(test, ref, mode, eotf, fl));
    if (test_frames < 1 || ref_frames < 1)
        return grad_fail(FVVDP_EINVAL, "a stream needs at least one frame (test: %d, reference: %d)", test_frames, ref_frames);
    if (n_out < 1) return grad_fail(FVVDP_EINVAL, "n_out %d: at least one output frame", n_out);
    // every index inside its stream: the kernels read frame idx * frame_stride without a further check
    for (int u = 0; u < fl - 1 + n_out; ++u) {
        if (h_idx_test[u] < 0 || h_idx_test[u] >= test_frames)
            return grad_fail(FVVDP_EINVAL, "list entry %d names frame %d outside the test's [0, %d)", u, h_idx_test[u], test_frames);
        if (h_idx_ref[u] < 0 || h_idx_ref[u] >= ref_frames)
            return grad_fail(FVVDP_EINVAL, "list entry %d names frame %d outside the reference's [0, %d)", u, h_idx_ref[u], ref_frames);
    }
    // (the context's frame size is the target of the resize)
    IngestBegin b;
    GRAD_CHECK(fvvdp_ctx_ingest_begin(ctx, "the resizing ingest", false, test->channels, eotf, h_rgb2y, h_taps, fl, n_out, slot0, &b));
    const int W = b.W, H = b.H;
    GRAD_CHECK(resize_check_axes(W, H, "target"));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    const int FL = ingest_ring_length(fl);
    for (const IngestWindow wnd : IngestWindows(fl, n_out)) {
        ResizedHoldArgs h;
        memset(&h, 0, sizeof(h));
        ResizedArgs& a = h.a;
        a.src[0] = resize_dev_stream(test, W, H);
        a.src[1] = resize_dev_stream(ref, W, H);
        a.Wo = W;
        a.Ho = H;
        grad_fill_eotf(a.e, a.w, eotf, test->channels, h_rgb2y);
        a.out = b.out;
        ingest_fill_window(a, wnd, slot0, h_taps, fl, h_idx_test);              // (both lists are checked above)
        ingest_fill_indices(h.idx1, wnd, fl, h_idx_ref);
        if (FL == 8) launch_ring<8>(mode, h, st);
        else if (FL == 16) launch_ring<16>(mode, h, st);
        else launch_ring<32>(mode, h, st);
        GRAD_HIP_TRY(hipGetLastError());
    }
    return FVVDP_OK;
}

template <int MODE>
static void launch_run_d(const ResizeAdjRunArgs& r, int nf, hipStream_t st) {
    const size_t HWo = (size_t)r.a.Wo * r.a.Ho;
    hipLaunchKernelGGL((resize_adjoint_run_d_kernel<MODE>), dim3((unsigned int)((HWo + 255) / 256), nf), dim3(256), 0, st, r);
}

extern "C" int fvvdp_resize_grad_held(int out_width, int out_height, int n_display, int n_source, const float* d_gL,
                                      const int32_t* h_map, const fvvdp_resize_stream* test, float* d_grad, int mode,
                                      const fvvdp_eotf* eotf, const float* h_rgb2y, void* d_work, size_t work_bytes, void* stream) {
    if (!d_gL || !h_map || !test || !d_grad || !eotf || !h_rgb2y || !d_work) return grad_fail(FVVDP_EINVAL, "null argument");
    if (n_display < 1 || n_source < 1)
        return grad_fail(FVVDP_EINVAL, "bad shape %dx%d, %d display frames, %d source frames", out_width, out_height, n_display, n_source);
    // the map: stage 1 reads display frames [run[j], run[j + 1]) of d_gL without a further check
    for (int v = 0; v < n_display; ++v) {
        if (h_map[v] < 0 || h_map[v] >= n_source)
            return grad_fail(FVVDP_EINVAL, "frame map entry %d names source frame %d outside [0, %d)", v, h_map[v], n_source);
        if (v > 0 && h_map[v] < h_map[v - 1])
            return grad_fail(FVVDP_EINVAL, "frame map must be non-decreasing (entry %d: %d after %d)", v, h_map[v], h_map[v - 1]);
    }
    // run[j]: the first display frame that shows a source frame >= j; run[n_source] = n_display
    static thread_local std::vector<int32_t> run;
    run.assign((size_t)n_source + 1, n_display);
    for (int v = n_display - 1; v >= 0; --v) run[h_map[v]] = v;
    for (int j = n_source - 1; j >= 0; --j)
        if (run[j] > run[j + 1]) run[j] = run[j + 1];             // (a frame never shown: the empty run at its successor's start)
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ResizeAdjRunArgs r;
    memset(&r, 0, sizeof(r));
    int m = 0;
    size_t batch = 0;
    const size_t tb = test->width >= 1 && test->height >= 1 ? FVVDP_RESIZE_GRAD_HELD_TABLE_BYTES(test->width, test->height, n_source) : 0;
    GRAD_CHECK(resize_adjoint_begin(out_width, out_height, n_source, d_gL, test, d_grad, mode, eotf, h_rgb2y, d_work, work_bytes, tb,
                                    run.data(), run.size(), st, &r.a, &m, &batch));
    r.run = r.a.xhi + test->width;

    for (int f0 = 0; f0 < n_source; f0 += (int)batch) {
        const int nf = (n_source - f0) < (int)batch ? (n_source - f0) : (int)batch;
        r.a.f0 = f0;
        switch (m) {
            case FVVDP_RESIZE_NEAREST: launch_run_d<FVVDP_RESIZE_NEAREST>(r, nf, st); break;
            case FVVDP_RESIZE_BILINEAR: launch_run_d<FVVDP_RESIZE_BILINEAR>(r, nf, st); break;
            case FVVDP_RESIZE_BICUBIC: launch_run_d<FVVDP_RESIZE_BICUBIC>(r, nf, st); break;
            case FVVDP_RESIZE_AREA: launch_run_d<FVVDP_RESIZE_AREA>(r, nf, st); break;
            default: launch_run_d<RZ_IDENTITY>(r, nf, st); break;
        }
        resize_launch_gather(m, r.a, nf, st);
        GRAD_HIP_TRY(hipGetLastError());
    }
    return FVVDP_OK;
}
