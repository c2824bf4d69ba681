// Launchers of the stage-1 (temporal) kernels.  The kernels are instantiated in temporal_launch.hip, which is compiled once
// per sample type (-DK1_PART=0 uint8, 1 uint16, 2 float, 3 planar YUV and the dispatcher, 4 float16, 5 bfloat16): the register-ring kernels are fully unrolled per ring
// length, channel count and display model, and one translation unit holding all of them took 4 minutes to compile.
#pragma once
#include "temporal_kernels.hpp"

// Pixels per lane (PX) of temporal_vec_kernel, per ring length; one frame of raw samples in flight (TD = 1).
// Measured at 4K (tools/gpu_fps.py): the long rings are register-bound (2*FL*PX ring registers), float samples are 4x
// wider than 8-bit ones in the prefetch registers.
static constexpr int k1_px(int FL) { return FL == 8 ? 4 : (FL == 64 ? 1 : 2); }
// what the 64-slot ring (temporal filters of 33-64 taps, 129-256 fps) is instantiated for
static inline bool k1_ring64_ok(int dtype, int C, int eotf_kind) {
    if (dtype == FVVDP_U8) return true;
    if (C == 3 && (eotf_kind == FVVDP_EOTF_SRGB || eotf_kind == FVVDP_EOTF_PQ)) return true;      // uint16 (closed form) / float, float16, bfloat16 RGB
    return dtype == FVVDP_F32 && C == 1 && eotf_kind == FVVDP_EOTF_NONE;                          // luminance frames
}

// The context's side of an ingest (fvvdp_hip.hip), for every entry point that writes a clip into level 0, in whichever translation
// unit its kernels live.  Checks the context -- planes == 4 ("<what> is for video contexts"; what = nullptr: the array ingest, whose
// still-image contexts take fl == 1), slots [slot0, slot0 + n_out) inside max_frames, even_size: the 4:2:0 rule on the frame size --
// and keeps the books of level 0's value range for `channels` weights, which is what lets the pyramid pass drop its clamps: an
// ingest that did not come through here would leave them dropped on the strength of an earlier call's range.
struct IngestBegin {
    int W, H;              // the context's frame size
    int planes;            // 4: a video context, 2: a still-image context
    L0Addr out;            // level 0 at slot0
    EotfDev e;             // the display block as the kernels take it (a table without a stated range: any value passes)
    bool scalar, debug;    // FVVDP_TEMPORAL_SCALAR, FVVDP_DEBUG_VARIANT
};
int fvvdp_ctx_ingest_begin(fvvdp_ctx* c, const char* what, bool even_size, int channels, const fvvdp_eotf* eotf, const float* h_rgb2y,
                           const float* h_taps, int fl, int n_out, int slot0, IngestBegin* b);

// FL in {8, 16, 32}; dtype FVVDP_U8 / U16 / F32 / F16 / BF16.  FL = 64: see k1_ring64_ok().
bool k1_launch_vec(int FL, int dtype, const TemporalArgs& a, hipStream_t st);     // aligned sizes (see the call site); true: blocks handed out by the ticket counter
void k1_launch_ring(int FL, int dtype, const TemporalArgs& a, hipStream_t st);    // any size
void k1_launch_generic(int planes, int dtype, const GenericArgs& a, hipStream_t st);
void k1_launch_luminance(int dtype, const LumArgs& a, hipStream_t st);     // source frames -> fp32 luminance frames (two-pass path)
void k1_launch_yuv_vec(int FL, int bytes, bool c420, bool general_matrix, const YuvArgs& a, hipStream_t st);   // FL in {8, 16}
void k1_launch_yuv(int FL, int bytes, const YuvArgs& a, hipStream_t st);
void k1_launch_yuv_luminance(int bytes, const YuvLumArgs& a, hipStream_t st);   // planar YUV frames -> fp32 luminance frames (two-pass path)
