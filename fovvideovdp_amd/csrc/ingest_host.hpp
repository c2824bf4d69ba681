// Host code the clip ingests share (array, per-frame pointers, packed YUV, float YUV planes, resized streams, held frames): what
// lies between the C ABI and a kernel launch and is the same for all of them -- the launch windows of a call, the window's part of
// an argument block, the conversion constants.  Host code only, and no HIP header: a plain C++ program can include it
// (tests/ingest_windows_check.cpp does).  The templates take any argument block that has the members they name.
#pragma once
#include <cstddef>
#include <cstdint>

#include "fvvdp_hip.h"

// History + outputs of one launch: the index lists of the argument blocks (TemporalArgs::idx and its kin) hold this many entries.
static constexpr int T_MAX_IDX = 320;

// bytes per sample of an FVVDP_* sample type
static constexpr size_t ingest_sample_bytes(int dtype) {
    return dtype == FVVDP_U8 ? 1 : ((dtype == FVVDP_U16 || dtype >= FVVDP_F16) ? 2 : 4);
}

// FL: the register ring a filter of fl taps runs in
static constexpr int ingest_ring_length(int fl) { return fl <= 8 ? 8 : (fl <= 16 ? 16 : (fl <= 32 ? 32 : 64)); }

// One launch of a call: output frames [t0, t0 + nn) of the call's n_out.
struct IngestWindow {
    int t0, nn;
};

// The launches of a call of n_out output frames with fl taps: `for (const IngestWindow wnd : IngestWindows(fl, n_out))`.  A
// launch's list holds the FL - 1 frames of history before its outputs, so it makes T_MAX_IDX - (FL - 1) outputs at the most.
class IngestWindows {
public:
    IngestWindows(int fl, int n_out) : max_out_(T_MAX_IDX - (ingest_ring_length(fl) - 1)), n_out_(n_out) {}
    struct iterator {
        int t0, n_out, max_out;
        IngestWindow operator*() const { return IngestWindow{t0, (n_out - t0) < max_out ? (n_out - t0) : max_out}; }
        iterator& operator++() { t0 += max_out; return *this; }
        bool operator!=(const iterator&) const { return t0 < n_out; }      // (against end() only: t0 may step past n_out)
    };
    iterator begin() const { return iterator{0, n_out_, max_out_}; }
    iterator end() const { return iterator{n_out_, n_out_, max_out_}; }

private:
    int max_out_, n_out_;
};

// The index list of one window from the call's list h_idx [fl - 1 + n_out].  Virtual time of h_idx: entry (fl - 1 + t) is the newest
// frame of output t.  The ring has FL >= fl slots; the FL - fl entries before the true history are padded with a valid frame (their
// taps are zero).  Returns the first negative entry among those used, or nullptr: kernels that read frame idx * stride without a
// further check have their entry point refuse such a list.
static inline const int32_t* ingest_fill_indices(int* idx, IngestWindow wnd, int fl, const int32_t* h_idx) {
    const int FL = ingest_ring_length(fl), pad = FL - fl;
    const int32_t* negative = nullptr;
    for (int u = 0; u < FL - 1 + wnd.nn; ++u) {
        const int src = wnd.t0 + u - pad;         // index into h_idx
        const int32_t* f = h_idx + (src < 0 ? 0 : src);
        if (*f < 0 && !negative) negative = f;
        idx[u] = *f;
    }
    return negative;
}

// The window's part of a zeroed argument block: n_out, fl, the slot of the window's first output, the tap pairs {sustained,
// transient} (zero beyond fl) and the index list.  Returns as ingest_fill_indices.
template <class Args>
static const int32_t* ingest_fill_window(Args& a, IngestWindow wnd, int slot0, const float* h_taps, int fl, const int32_t* h_idx) {
    a.n_out = wnd.nn;
    a.fl = fl;
    a.out.slot0 = slot0 + wnd.t0;
    for (int k = 0; k < fl; ++k) { a.taps2[k][0] = h_taps[k]; a.taps2[k][1] = h_taps[fl + k]; }
    return ingest_fill_indices(a.idx, wnd, fl, h_idx);
}

// The same for a block whose streams have a list each (idx1: the reference's); h_idx1 = nullptr: both streams take h_idx.
template <class Args>
static const int32_t* ingest_fill_window(Args& a, IngestWindow wnd, int slot0, const float* h_taps, int fl, const int32_t* h_idx,
                                         const int32_t* h_idx1) {
    const int32_t* n0 = ingest_fill_window(a, wnd, slot0, h_taps, fl, h_idx);
    const int32_t* n1 = ingest_fill_indices(a.idx1, wnd, fl, h_idx1 ? h_idx1 : h_idx);
    return n0 ? n0 : n1;
}

// the luminance weights of C channels (C == 1: the sample is the luminance), into a zeroed block
static inline void ingest_fill_weights(float (&w)[3], int C, const float* h_rgb2y) {
    if (C == 3) { w[0] = h_rgb2y[0]; w[1] = h_rgb2y[1]; w[2] = h_rgb2y[2]; } else { w[0] = 1.0f; }
}

// The display block as the kernels take it (EotfDev), member by member from the ABI's.  What a caller does with a table -- none for
// the closed-form models of the gradients, a range of its own for a table that states none -- it does after this.
template <class Dev>
static void ingest_fill_display(Dev& e, const fvvdp_eotf* eotf) {
    e.kind = eotf->kind;
    e.scale = eotf->Y_peak - eotf->Y_black;
    e.y_black = eotf->Y_black;
    e.y_peak = eotf->Y_peak;
    e.gamma = eotf->gamma;
    e.l_min = eotf->L_min;
    e.l_max = eotf->L_max;
    e.lut = eotf->d_lut;
}

// The constants of the limited-range YUV unpack of a width x height frame: the chroma planes' size, 1 / (2^(b-8) * 219) and
// 1 / (2^(b-8) * 224), the colour matrix (YuvArgs, YuvRgbArgs, YuvUnpack).
template <class Unpack>
static void ingest_fill_unpack(Unpack& k, int width, int height, const fvvdp_yuv_format* fmt) {
    k.W = width;
    k.H = height;
    k.chroma420 = fmt->chroma_420 ? 1 : 0;
    k.uvw = fmt->chroma_420 ? width / 2 : width;
    k.uvh = fmt->chroma_420 ? height / 2 : height;
    const float scale = (float)(1 << (fmt->bit_depth - 8));
    k.wy = 1.0f / (scale * 219.0f);
    k.wc = 1.0f / (scale * 224.0f);
    for (int i = 0; i < 9; ++i) k.m[i] = fmt->ycbcr2rgb[i];
}
