// Host code the two units of the resized clips share (resize_launch.hip, resize_held_launch.hip): the argument checks of a
// stream, the stream as the kernels take it, and everything of the adjoint that lies in front of its launches -- checks, the
// candidate ranges of the gather, the upload of the tables.  Include after grad_common.hpp and resize_clip_kernels.hpp.  The
// gather's kernels are instantiated by resize_launch.hip alone; resize_held_launch.hip launches them through
// resize_launch_gather.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

static inline int resize_check_mode(int mode) {
    if (mode < FVVDP_RESIZE_NEAREST || mode > FVVDP_RESIZE_AREA) return grad_fail(FVVDP_EINVAL, "unknown resize mode %d", mode);
    return FVVDP_OK;
}

// the sizes the index arithmetic of resize_axis.hpp is exact for, of a stream and of the target alike (fvvdp_yuv_frame_resized
// refuses the same sizes in the same words)
static inline int resize_check_axes(int width, int height, const char* what) {
    if (width > RZ_MAX_AXIS || height > RZ_MAX_AXIS)
        return grad_fail(FVVDP_EINVAL, "frame size out of range (1..%d per axis): %dx%d (%s)", RZ_MAX_AXIS, width, height, what);
    return FVVDP_OK;
}

// pointer set and aligned to its sample, a size between 1 x 1 and RZ_MAX_AXIS per axis (every offset inside a plane fits an int,
// the rows of the gather fit its grid), strides that hold a plane
static inline int resize_check_stream(const fvvdp_resize_stream* s, const char* what, bool float_only) {
    if (!s->d_data) return grad_fail(FVVDP_EINVAL, "null data pointer (%s)", what);
    if (s->dtype != FVVDP_F32 && (float_only || s->dtype != FVVDP_U8))
        return grad_fail(FVVDP_EINVAL, "the %s must be float32%s (dtype %d)", what, float_only ? "" : " or uint8", s->dtype);
    if (s->dtype == FVVDP_F32 && reinterpret_cast<uintptr_t>(s->d_data) % 4 != 0)
        return grad_fail(FVVDP_EINVAL, "data pointer must be aligned to 4 bytes (%s)", what);
    if (s->channels != 1 && s->channels != 3) return grad_fail(FVVDP_EINVAL, "The content must have either 1 or 3 colour channels.");
    if (s->width < 1 || s->height < 1) return grad_fail(FVVDP_EINVAL, "bad frame size %dx%d (%s)", s->width, s->height, what);
    GRAD_CHECK(resize_check_axes(s->width, s->height, what));
    const size_t hw = (size_t)s->width * s->height;
    if (s->plane_stride < hw) return grad_fail(FVVDP_EINVAL, "plane_stride %zu is below the plane size %zu (%s)", s->plane_stride, hw, what);
    // (frames may lie inside a plane, [C][N][H][W], or planes inside a frame: either stride holds one plane at least)
    if (s->frame_stride < hw) return grad_fail(FVVDP_EINVAL, "frame_stride %zu is below the plane size %zu (%s)", s->frame_stride, hw, what);
    return FVVDP_OK;
}

// what the ingests check before they look at the context
static inline int resize_check_ingest(const fvvdp_resize_stream* test, const fvvdp_resize_stream* ref, int mode, const fvvdp_eotf* eotf,
                                      int fl) {
    GRAD_CHECK(resize_check_mode(mode));
    if (fl < 1 || fl > FVVDP_MAX_TAPS) return grad_fail(FVVDP_EINVAL, "filter length %d outside [1, %d]", fl, FVVDP_MAX_TAPS);
    if (fl > FVVDP_RESIZE_MAX_TAPS)
        return grad_fail(FVVDP_EUNSUPPORTED, "the resizing ingest covers temporal filters of up to %d taps (120 frames per second); "
                                             "this one has %d", FVVDP_RESIZE_MAX_TAPS, fl);
    if (eotf->kind < FVVDP_EOTF_SRGB || eotf->kind > FVVDP_EOTF_ABSOLUTE)
        return grad_fail(FVVDP_EINVAL, "resized sources need a closed-form display model (samples are fractional after the resize)");
    GRAD_CHECK(resize_check_stream(test, "test", false));
    GRAD_CHECK(resize_check_stream(ref, "reference", false));
    if (test->channels != ref->channels)
        return grad_fail(FVVDP_EINVAL, "test and reference differ in their channel counts (%d and %d)", test->channels, ref->channels);
    return FVVDP_OK;
}

static inline RzStream resize_dev_stream(const fvvdp_resize_stream* s, int Wo, int Ho) {
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

// pixels per lane of the ring kernels: two for the short rings of the modes with few taps; the 32-slot ring, bicubic (16 indices
// and 8 coefficients per stream and pixel) and area (a loop over its window per pixel) keep one, which keeps every variant clear of
// register spills
static constexpr int resize_ring_px(int FL, int MODE) { return (FL <= 16 && MODE <= FVVDP_RESIZE_BILINEAR) ? 2 : 1; }

// Candidate ranges of the gather: per source index of one axis the targets [lo, hi) whose taps can reach it, from the same index
// functions the kernels evaluate (a target reaches every index between its lowest and its highest tap: a superset where taps are
// folded).  A source index no target reaches keeps the empty range [0, 0).
template <int MODE>
static void resize_axis_ranges(int n, int n_out, float scale, int32_t* lo, int32_t* hi) {
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

// The adjoint in front of its launches, for fvvdp_resize_grad and fvvdp_resize_grad_held: the checks, the argument block, the
// range tables ylo [h] | yhi [h] | xlo [w] | xhi [w] followed by the caller's own `n_extra` int32 (h_extra; the run table of the
// held variant) in one upload to the head of the workspace, `table_bytes` long in all.  n_frames: the frames of the test and of
// d_grad.  Returns the mode the kernels run in (RZ_IDENTITY for a test of the target's size) in *m and the frames of the first
// stage the workspace holds at once in *batch.
static inline int resize_adjoint_begin(int out_width, int out_height, int n_frames, const float* d_gL, const fvvdp_resize_stream* test,
                                       float* d_grad, int mode, const fvvdp_eotf* eotf, const float* h_rgb2y, void* d_work,
                                       size_t work_bytes, size_t table_bytes, const int32_t* h_extra, size_t n_extra, hipStream_t st,
                                       ResizeAdjArgs* out, int* m_out, size_t* batch_out) {
    if (out_width < 1 || out_height < 1 || n_frames < 1)
        return grad_fail(FVVDP_EINVAL, "bad shape %dx%d, %d frames", out_width, out_height, n_frames);
    GRAD_CHECK(resize_check_axes(out_width, out_height, "target"));
    const size_t HWo = (size_t)out_width * out_height;
    GRAD_CHECK(resize_check_mode(mode));
    GRAD_CHECK(grad_check_closed_form(eotf));
    GRAD_CHECK(resize_check_stream(test, "test", true));
    if ((reinterpret_cast<uintptr_t>(d_gL) | reinterpret_cast<uintptr_t>(d_grad)) % 4 != 0)
        return grad_fail(FVVDP_EINVAL, "d_gL and d_grad must be aligned to 4 bytes");
    if (reinterpret_cast<uintptr_t>(d_work) % 256 != 0) return grad_fail(FVVDP_EINVAL, "workspace must be 256-byte aligned");
    const int w = test->width, h = test->height, C = test->channels;
    const size_t tb = table_bytes;
    const size_t per_frame = (size_t)C * HWo * sizeof(float);
    if (work_bytes < tb + per_frame)
        return grad_fail(FVVDP_EINVAL, "workspace of %zu bytes is below the %zu needed for one frame", work_bytes, tb + per_frame);
    size_t batch = (work_bytes - tb) / per_frame;
    if (batch > (size_t)(65535 / C)) batch = (size_t)(65535 / C);

    ResizeAdjArgs& a = *out;
    memset(&a, 0, sizeof(a));
    a.gL = d_gL;
    a.t = resize_dev_stream(test, out_width, out_height);
    a.grad = d_grad;
    a.Wo = out_width;
    a.Ho = out_height;
    grad_fill_eotf(a.e, a.w, eotf, C, h_rgb2y);
    const int m = a.t.identity ? RZ_IDENTITY : mode;

    // the host copy is the thread's own and outlives the call
    static thread_local std::vector<int32_t> tab;
    tab.assign((size_t)2 * (w + h) + n_extra, 0);
    int32_t* ylo = tab.data();
    int32_t* yhi = ylo + h;
    int32_t* xlo = yhi + h;
    int32_t* xhi = xlo + w;
    switch (m) {
        case FVVDP_RESIZE_NEAREST:
            resize_axis_ranges<FVVDP_RESIZE_NEAREST>(h, out_height, a.t.sy, ylo, yhi);
            resize_axis_ranges<FVVDP_RESIZE_NEAREST>(w, out_width, a.t.sx, xlo, xhi);
            break;
        case FVVDP_RESIZE_BILINEAR:
            resize_axis_ranges<FVVDP_RESIZE_BILINEAR>(h, out_height, a.t.sy, ylo, yhi);
            resize_axis_ranges<FVVDP_RESIZE_BILINEAR>(w, out_width, a.t.sx, xlo, xhi);
            break;
        case FVVDP_RESIZE_BICUBIC:
            resize_axis_ranges<FVVDP_RESIZE_BICUBIC>(h, out_height, a.t.sy, ylo, yhi);
            resize_axis_ranges<FVVDP_RESIZE_BICUBIC>(w, out_width, a.t.sx, xlo, xhi);
            break;
        case FVVDP_RESIZE_AREA:
            resize_axis_ranges<FVVDP_RESIZE_AREA>(h, out_height, a.t.sy, ylo, yhi);
            resize_axis_ranges<FVVDP_RESIZE_AREA>(w, out_width, a.t.sx, xlo, xhi);
            break;
        default:
            resize_axis_ranges<RZ_IDENTITY>(h, out_height, a.t.sy, ylo, yhi);
            resize_axis_ranges<RZ_IDENTITY>(w, out_width, a.t.sx, xlo, xhi);
            break;
    }
    for (size_t k = 0; k < n_extra; ++k) xhi[w + k] = h_extra[k];
    GRAD_HIP_TRY(hipMemcpyAsync(d_work, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    const int* dt = reinterpret_cast<const int*>(d_work);
    a.ylo = dt;
    a.yhi = dt + h;
    a.xlo = dt + 2 * h;
    a.xhi = dt + 2 * h + w;
    a.d = reinterpret_cast<float*>(reinterpret_cast<char*>(d_work) + tb);
    *m_out = m;
    *batch_out = batch;
    return FVVDP_OK;
}

// stage 2 of the adjoint for nf frames from a.f0 on, in mode m (resize_launch.hip; not exported)
void resize_launch_gather(int m, const ResizeAdjArgs& a, int nf, hipStream_t st);
