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

static_assert(FVVDP_RESIZE_MAX_TAPS == 32, "ResizedArgs::taps2");
static_assert(FVVDP_RESIZE_MAX_AXIS == RZ_MAX_AXIS, "resize_axis.hpp");

static int check_mode(int mode) {
    if (mode < FVVDP_RESIZE_NEAREST || mode > FVVDP_RESIZE_AREA) return grad_fail(FVVDP_EINVAL, "unknown resize mode %d", mode);
    return FVVDP_OK;
}

// the sizes the index arithmetic of resize_axis.hpp is exact for, of a stream and of the target alike (fvvdp_yuv_frame_resized
// refuses the same sizes in the same words)
static int check_axes(int width, int height, const char* what) {
    if (width > RZ_MAX_AXIS || height > RZ_MAX_AXIS)
        return grad_fail(FVVDP_EINVAL, "frame size out of range (1..%d per axis): %dx%d (%s)", RZ_MAX_AXIS, width, height, what);
    return FVVDP_OK;
}

// pointer set and aligned to its sample, a size between 1 x 1 and RZ_MAX_AXIS per axis (every offset inside a plane fits an int,
// the rows of the gather fit its grid), strides that hold a plane
static int check_stream(const fvvdp_resize_stream* s, const char* what, bool float_only) {
    if (!s->d_data) return grad_fail(FVVDP_EINVAL, "null data pointer (%s)", what);
    if (s->dtype != FVVDP_F32 && (float_only || s->dtype != FVVDP_U8))
        return grad_fail(FVVDP_EINVAL, "the %s must be float32%s (dtype %d)", what, float_only ? "" : " or uint8", s->dtype);
    if (s->dtype == FVVDP_F32 && reinterpret_cast<uintptr_t>(s->d_data) % 4 != 0)
        return grad_fail(FVVDP_EINVAL, "data pointer must be aligned to 4 bytes (%s)", what);
    if (s->channels != 1 && s->channels != 3) return grad_fail(FVVDP_EINVAL, "The content must have either 1 or 3 colour channels.");
    if (s->width < 1 || s->height < 1) return grad_fail(FVVDP_EINVAL, "bad frame size %dx%d (%s)", s->width, s->height, what);
    GRAD_CHECK(check_axes(s->width, s->height, what));
    const size_t hw = (size_t)s->width * s->height;
    if (s->plane_stride < hw) return grad_fail(FVVDP_EINVAL, "plane_stride %zu is below the plane size %zu (%s)", s->plane_stride, hw, what);
    // (frames may lie inside a plane, [C][N][H][W], or planes inside a frame: either stride holds one plane at least)
    if (s->frame_stride < hw) return grad_fail(FVVDP_EINVAL, "frame_stride %zu is below the plane size %zu (%s)", s->frame_stride, hw, what);
    return FVVDP_OK;
}

static RzStream dev_stream(const fvvdp_resize_stream* s, int Wo, int Ho) {
    RzStream r;
    memset(&r, 0, sizeof(r));
    r.p = s->d_data;
    r.u8 = s->dtype == FVVDP_U8 ? 1 : 0;
    r.C = s->channels;
    r.W = s->width;
    r.H = s->height;
    r.identity = (s->width == Wo && s->height == Ho) ? 1 : 0;
    r.fs = s->frame_stride;
    r.ps = s->plane_stride;
    r.sx = (float)s->width / (float)Wo;
    r.sy = (float)s->height / (float)Ho;
    return r;
}

// pixels per lane: two for the short rings of the modes with few taps; the 32-slot ring, bicubic (16 indices and 8 coefficients per
// stream and pixel) and area (a loop over its window per pixel) keep one, which keeps every variant clear of register spills
template <int FL, int MODE>
static void launch_ring_mode(const ResizedArgs& a, hipStream_t st) {
    constexpr int PX = (FL <= 16 && MODE <= FVVDP_RESIZE_BILINEAR) ? 2 : 1;
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
    GRAD_CHECK(check_mode(mode));
    if (fl < 1 || fl > FVVDP_MAX_TAPS) return grad_fail(FVVDP_EINVAL, "filter length %d outside [1, %d]", fl, FVVDP_MAX_TAPS);
    if (fl > FVVDP_RESIZE_MAX_TAPS)
        return grad_fail(FVVDP_EUNSUPPORTED, "the resizing ingest covers temporal filters of up to %d taps (120 frames per second); "
                                             "this one has %d", FVVDP_RESIZE_MAX_TAPS, fl);
    if (eotf->kind < FVVDP_EOTF_SRGB || eotf->kind > FVVDP_EOTF_ABSOLUTE)
        return grad_fail(FVVDP_EINVAL, "resized sources need a closed-form display model (samples are fractional after the resize)");
    GRAD_CHECK(check_stream(test, "test", false));
    GRAD_CHECK(check_stream(ref, "reference", false));
    if (test->channels != ref->channels)
        return grad_fail(FVVDP_EINVAL, "test and reference differ in their channel counts (%d and %d)", test->channels, ref->channels);
    // (the context's frame size is the target of the resize)
    IngestBegin b;
    GRAD_CHECK(fvvdp_ctx_ingest_begin(ctx, "the resizing ingest", false, test->channels, eotf, h_rgb2y, h_taps, fl, n_out, slot0, &b));
    const int W = b.W, H = b.H;
    GRAD_CHECK(check_axes(W, H, "target"));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    const int FL = ingest_ring_length(fl);
    for (const IngestWindow wnd : IngestWindows(fl, n_out)) {
        ResizedArgs a;
        memset(&a, 0, sizeof(a));
        a.src[0] = dev_stream(test, W, H);
        a.src[1] = dev_stream(ref, W, H);
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

// Candidate ranges of the gather: per source index of one axis the targets [lo, hi) whose taps can reach it, from the same index
// functions the kernels evaluate (a target reaches every index between its lowest and its highest tap: a superset where taps are
// folded).  A source index no target reaches keeps the empty range [0, 0).
template <int MODE>
static void axis_ranges(int n, int n_out, float scale, int32_t* lo, int32_t* hi) {
    for (int i = 0; i < n; ++i) { lo[i] = 0x7FFFFFFF; hi[i] = 0; }
    for (int o = 0; o < n_out; ++o) {
        int a, b;
        rz_axis_reach<MODE>(o, n, n_out, scale, a, b);
        a = a < 0 ? 0 : a;
        b = b > n - 1 ? n - 1 : b;
        for (int i = a; i <= b; ++i) {
            if (o < lo[i]) lo[i] = o;
            if (o + 1 > hi[i]) hi[i] = o + 1;
        }
    }
    for (int i = 0; i < n; ++i)
        if (hi[i] == 0) lo[i] = 0;
}

template <int MODE>
static void launch_adjoint(const ResizeAdjArgs& a, int nf, hipStream_t st) {
    const size_t HWo = (size_t)a.Wo * a.Ho;
    hipLaunchKernelGGL((resize_adjoint_d_kernel<MODE>), dim3((unsigned int)((HWo + 255) / 256), nf), dim3(256), 0, st, a);
    hipLaunchKernelGGL((resize_adjoint_gather_kernel<MODE>), dim3((a.t.W + 63) / 64, (a.t.H + 3) / 4, nf * a.t.C), dim3(64, 4), 0, st, a);
}

extern "C" int fvvdp_resize_grad(int out_width, int out_height, int n_frames, const float* d_gL, const fvvdp_resize_stream* test,
                                 float* d_grad, int mode, const fvvdp_eotf* eotf, const float* h_rgb2y, void* d_work,
                                 size_t work_bytes, void* stream) {
    if (!d_gL || !test || !d_grad || !eotf || !h_rgb2y || !d_work) return grad_fail(FVVDP_EINVAL, "null argument");
    if (out_width < 1 || out_height < 1 || n_frames < 1)
        return grad_fail(FVVDP_EINVAL, "bad shape %dx%d, %d frames", out_width, out_height, n_frames);
    GRAD_CHECK(check_axes(out_width, out_height, "target"));
    const size_t HWo = (size_t)out_width * out_height;
    GRAD_CHECK(check_mode(mode));
    GRAD_CHECK(grad_check_closed_form(eotf));
    GRAD_CHECK(check_stream(test, "test", true));
    if ((reinterpret_cast<uintptr_t>(d_gL) | reinterpret_cast<uintptr_t>(d_grad)) % 4 != 0)
        return grad_fail(FVVDP_EINVAL, "d_gL and d_grad must be aligned to 4 bytes");
    if (reinterpret_cast<uintptr_t>(d_work) % 256 != 0) return grad_fail(FVVDP_EINVAL, "workspace must be 256-byte aligned");
    const int w = test->width, h = test->height, C = test->channels;
    const size_t tb = FVVDP_RESIZE_GRAD_TABLE_BYTES(w, h);
    const size_t per_frame = (size_t)C * HWo * sizeof(float);
    if (work_bytes < tb + per_frame)
        return grad_fail(FVVDP_EINVAL, "workspace of %zu bytes is below the %zu needed for one frame", work_bytes, tb + per_frame);
    size_t batch = (work_bytes - tb) / per_frame;
    if (batch > (size_t)(65535 / C)) batch = (size_t)(65535 / C);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    ResizeAdjArgs a;
    memset(&a, 0, sizeof(a));
    a.gL = d_gL;
    a.t = dev_stream(test, out_width, out_height);
    a.grad = d_grad;
    a.Wo = out_width;
    a.Ho = out_height;
    grad_fill_eotf(a.e, a.w, eotf, C, h_rgb2y);
    const int m = a.t.identity ? RZ_IDENTITY : mode;

    // the tables: ylo [h] | yhi [h] | xlo [w] | xhi [w].  The host copy is the thread's own and outlives the call
    static thread_local std::vector<int32_t> tab;
    tab.assign((size_t)2 * (w + h), 0);
    int32_t* ylo = tab.data();
    int32_t* yhi = ylo + h;
    int32_t* xlo = yhi + h;
    int32_t* xhi = xlo + w;
    switch (m) {
        case FVVDP_RESIZE_NEAREST:
            axis_ranges<FVVDP_RESIZE_NEAREST>(h, out_height, a.t.sy, ylo, yhi);
            axis_ranges<FVVDP_RESIZE_NEAREST>(w, out_width, a.t.sx, xlo, xhi);
            break;
        case FVVDP_RESIZE_BILINEAR:
            axis_ranges<FVVDP_RESIZE_BILINEAR>(h, out_height, a.t.sy, ylo, yhi);
            axis_ranges<FVVDP_RESIZE_BILINEAR>(w, out_width, a.t.sx, xlo, xhi);
            break;
        case FVVDP_RESIZE_BICUBIC:
            axis_ranges<FVVDP_RESIZE_BICUBIC>(h, out_height, a.t.sy, ylo, yhi);
            axis_ranges<FVVDP_RESIZE_BICUBIC>(w, out_width, a.t.sx, xlo, xhi);
            break;
        case FVVDP_RESIZE_AREA:
            axis_ranges<FVVDP_RESIZE_AREA>(h, out_height, a.t.sy, ylo, yhi);
            axis_ranges<FVVDP_RESIZE_AREA>(w, out_width, a.t.sx, xlo, xhi);
            break;
        default:
            axis_ranges<RZ_IDENTITY>(h, out_height, a.t.sy, ylo, yhi);
            axis_ranges<RZ_IDENTITY>(w, out_width, a.t.sx, xlo, xhi);
            break;
    }
    GRAD_HIP_TRY(hipMemcpyAsync(d_work, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    const int* dt = reinterpret_cast<const int*>(d_work);
    a.ylo = dt;
    a.yhi = dt + h;
    a.xlo = dt + 2 * h;
    a.xhi = dt + 2 * h + w;
    a.d = reinterpret_cast<float*>(reinterpret_cast<char*>(d_work) + tb);

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
