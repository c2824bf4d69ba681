// Clips whose streams have frame sizes of their own (include/fvvdp_hip_resize.h): argument checks and launches of the kernels of
// resize_clip_kernels.hpp.  A translation unit of its own, as yuv_grad_launch.hip: it instantiates no kernel template of the other
// units, and the one function that needs a context asks fvvdp_hip.hip for the context's side of the call (fvvdp_ctx_ingest_begin).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "fvvdp_hip.h"
#include "fvvdp_hip_resize.h"
#include "device_common.hpp"
#include "temporal_launch.hpp"     // fvvdp_ctx_ingest_begin
#include "grad_common.hpp"
#include "resize_clip_kernels.hpp"
#include "grad_host.hpp"
#include "resize_host.hpp"

static_assert(FVVDP_RESIZE_MAX_TAPS == 32, "ResizedArgs::taps2");
static_assert(FVVDP_RESIZE_MAX_AXIS == RZ_MAX_AXIS, "resize_axis.hpp");

template <int FL, int MODE>
static void launch_ring_mode(const ResizedArgs& a, hipStream_t st) {
    constexpr int PX = resize_ring_px(FL, MODE);
    const size_t HW = (size_t)a.Wo * a.Ho;
    const dim3 grid((unsigned int)((HW + 256 * PX - 1) / (256 * PX))), block(256);
    hipLaunchKernelGGL((resized_ring_kernel<FL, PX, MODE>), grid, block, 0, st, a);
}
template <int FL>
static void launch_ring(int mode, const ResizedArgs& a, hipStream_t st) {
    switch (mode) {
        case FVVDP_RESIZE_NEAREST: launch_ring_mode<FL, FVVDP_RESIZE_NEAREST>(a, st); break;
        case FVVDP_RESIZE_BILINEAR: launch_ring_mode<FL, FVVDP_RESIZE_BILINEAR>(a, st); break;
        case FVVDP_RESIZE_BICUBIC: launch_ring_mode<FL, FVVDP_RESIZE_BICUBIC>(a, st); break;
        default: launch_ring_mode<FL, FVVDP_RESIZE_AREA>(a, st); break;
    }
}

extern "C" int fvvdp_temporal_channels_resized(fvvdp_ctx* ctx, const fvvdp_resize_stream* test, const fvvdp_resize_stream* ref, int mode,
                                               const fvvdp_eotf* eotf, const float* h_rgb2y, const int32_t* h_frame_idx,
                                               const float* h_taps, int fl, int n_out, int slot0, void* stream) {
    if (!ctx || !test || !ref || !eotf || !h_rgb2y || !h_frame_idx || !h_taps) return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(resize_check_ingest(test, ref, mode, eotf, fl));
    // (the context's frame size is the target of the resize)
    IngestBegin b;
    GRAD_CHECK(fvvdp_ctx_ingest_begin(ctx, "the resizing ingest", false, test->channels, eotf, h_rgb2y, h_taps, fl, n_out, slot0, &b));
    const int W = b.W, H = b.H;
    GRAD_CHECK(resize_check_axes(W, H, "target"));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    const int FL = ingest_ring_length(fl);
    for (const IngestWindow wnd : IngestWindows(fl, n_out)) {
        ResizedArgs a;
        memset(&a, 0, sizeof(a));
        a.src[0] = resize_dev_stream(test, W, H);
        a.src[1] = resize_dev_stream(ref, W, H);
        a.Wo = W;
        a.Ho = H;
        grad_fill_eotf(a.e, a.w, eotf, test->channels, h_rgb2y);
        a.out = b.out;
        if (const int32_t* f = ingest_fill_window(a, wnd, slot0, h_taps, fl, h_frame_idx))
            return grad_fail(FVVDP_EINVAL, "frame index %d out of range", *f);
        if (FL == 8) launch_ring<8>(mode, a, st);
        else if (FL == 16) launch_ring<16>(mode, a, st);
        else launch_ring<32>(mode, a, st);
        GRAD_HIP_TRY(hipGetLastError());
    }
    return FVVDP_OK;
}

template <int MODE>
static void launch_adjoint(const ResizeAdjArgs& a, int nf, hipStream_t st) {
    const size_t HWo = (size_t)a.Wo * a.Ho;
    hipLaunchKernelGGL((resize_adjoint_d_kernel<MODE>), dim3((unsigned int)((HWo + 255) / 256), nf), dim3(256), 0, st, a);
    hipLaunchKernelGGL((resize_adjoint_gather_kernel<MODE>), dim3((a.t.W + 63) / 64, (a.t.H + 3) / 4, nf * a.t.C), dim3(64, 4), 0, st, a);
}

template <int MODE>
static void launch_gather(const ResizeAdjArgs& a, int nf, hipStream_t st) {
    hipLaunchKernelGGL((resize_adjoint_gather_kernel<MODE>), dim3((a.t.W + 63) / 64, (a.t.H + 3) / 4, nf * a.t.C), dim3(64, 4), 0, st, a);
}

// (resize_host.hpp) stage 2 alone, for fvvdp_resize_grad_held, whose first stage is its own
void resize_launch_gather(int m, const ResizeAdjArgs& a, int nf, hipStream_t st) {
    switch (m) {
        case FVVDP_RESIZE_NEAREST: launch_gather<FVVDP_RESIZE_NEAREST>(a, nf, st); break;
        case FVVDP_RESIZE_BILINEAR: launch_gather<FVVDP_RESIZE_BILINEAR>(a, nf, st); break;
        case FVVDP_RESIZE_BICUBIC: launch_gather<FVVDP_RESIZE_BICUBIC>(a, nf, st); break;
        case FVVDP_RESIZE_AREA: launch_gather<FVVDP_RESIZE_AREA>(a, nf, st); break;
        default: launch_gather<RZ_IDENTITY>(a, nf, st); break;
    }
}

extern "C" int fvvdp_resize_grad(int out_width, int out_height, int n_frames, const float* d_gL, const fvvdp_resize_stream* test,
                                 float* d_grad, int mode, const fvvdp_eotf* eotf, const float* h_rgb2y, void* d_work,
                                 size_t work_bytes, void* stream) {
    if (!d_gL || !test || !d_grad || !eotf || !h_rgb2y || !d_work) return grad_fail(FVVDP_EINVAL, "null argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ResizeAdjArgs a;
    int m = 0;
    size_t batch = 0;
    GRAD_CHECK(resize_adjoint_begin(out_width, out_height, n_frames, d_gL, test, d_grad, mode, eotf, h_rgb2y, d_work, work_bytes,
                                    test->width >= 1 && test->height >= 1 ? FVVDP_RESIZE_GRAD_TABLE_BYTES(test->width, test->height) : 0,
                                    nullptr, 0, st, &a, &m, &batch));

    for (int f0 = 0; f0 < n_frames; f0 += (int)batch) {
        const int nf = (n_frames - f0) < (int)batch ? (n_frames - f0) : (int)batch;
        a.f0 = f0;
        switch (m) {
            case FVVDP_RESIZE_NEAREST: launch_adjoint<FVVDP_RESIZE_NEAREST>(a, nf, st); break;
            case FVVDP_RESIZE_BILINEAR: launch_adjoint<FVVDP_RESIZE_BILINEAR>(a, nf, st); break;
            case FVVDP_RESIZE_BICUBIC: launch_adjoint<FVVDP_RESIZE_BICUBIC>(a, nf, st); break;
            case FVVDP_RESIZE_AREA: launch_adjoint<FVVDP_RESIZE_AREA>(a, nf, st); break;
            default: launch_adjoint<RZ_IDENTITY>(a, nf, st); break;
        }
        GRAD_HIP_TRY(hipGetLastError());
    }
    return FVVDP_OK;
}
