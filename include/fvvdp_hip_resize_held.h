/*
 * fvvdp_hip_resize_held.h -- clips whose two streams have frame sizes AND frame counts of their own in libfvvdp_hip.so: the
 * full-screen resize of fvvdp_hip_resize.h behind the frame maps of fvvdp_hip_held.h, forward and backward.
 *
 * An extension beside fvvdp_hip_resize.h, whose streams, modes, limits and conventions apply unchanged (fvvdp_resize_stream,
 * FVVDP_RESIZE_*, FVVDP_RESIZE_MAX_TAPS, FVVDP_RESIZE_MAX_AXIS; d_* device and h_* host pointers, return codes,
 * fvvdp_last_error, `stream` a hipStream_t passed as void*, asynchronous).  Each stream is shown by sample-and-hold through a
 * frame map m_s: display frame v in [0, N) shows source frame m_s[v] (non-decreasing; a repeat holds the frame, a skipped frame is
 * never shown).  The pair is judged at the display's rate and at the target size, and level 0 has the bits
 * fvvdp_temporal_channels_resized gives on the two clips expanded with index_select -- neither an expanded nor a resized clip is
 * ever stored.
 *
 * The backward of a clip of N display frames whose test has F frames:
 *   per batch, as fvvdp_hip_resize.h: fvvdp_temporal_channels_resized_held, fvvdp_bands_forward with every band's maps,
 *   fvvdp_video_grad_frames into the clip-long d_g0 [N][2][Ho][Wo];
 *   then once: fvvdp_video_grad_luminance (d_g0 -> d_gL [N][Ho][Wo], at the display's rate) and fvvdp_resize_grad_held (d_gL,
 *   the map and the test clip -> the gradient of every sample of the test clip, at the clip's own size and frame count).
 * Both stages of the resize's adjoint are linear in d_gL and every display frame that shows source frame j sees the same
 * interpolated values, so the sum over a frame's display frames is taken FIRST, on d_gL, and the two stages run on F frames
 * instead of N.  Every output is a fixed sum per sample (no atomics): the result does not depend on the launch geometry and
 * repeats bit for bit.
 */
#ifndef FVVDP_HIP_RESIZE_HELD_H
#define FVVDP_HIP_RESIZE_HELD_H

#include "fvvdp_hip_resize.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fvvdp_temporal_channels_resized with one window index list per stream: level 0 of slots [slot0, slot0 + n_out) of a video
 * context, whose frame size is the target.
 *   test, ref                    the two streams: the same channel count, each its own width x height and its own frame count;
 *   test_frames, ref_frames      the frame counts (>= 1): what the lists are checked against;
 *   h_idx_test, h_idx_ref        [fl - 1 + n_out] each: the display-rate window list sent through the stream's frame map.  Every
 *                                entry is checked on the host against its stream's frame count;
 *   every other argument         as fvvdp_temporal_channels_resized.
 * A held frame is converted once: per stream and step of a launch, when the stream's entry equals its entry at the previous step
 * the luminance is taken from the previous slot of the register ring (a wave-uniform branch on two scalar loads); otherwise, and
 * at the first step of every launch, it is gathered, interpolated, clipped and sent through the display model as
 * fvvdp_temporal_channels_resized does.  The reused value is the one that arithmetic would have produced again.
 * Errors: those of fvvdp_temporal_channels_resized, and FVVDP_EINVAL for a frame count below 1, n_out below 1 or a list entry
 * outside its stream. */
int fvvdp_temporal_channels_resized_held(fvvdp_ctx* ctx, const fvvdp_resize_stream* test, const fvvdp_resize_stream* ref,
                                         int test_frames, int ref_frames, int mode, const fvvdp_eotf* eotf, const float* h_rgb2y,
                                         const int32_t* h_idx_test, const int32_t* h_idx_ref, const float* h_taps, int fl, int n_out,
                                         int slot0, void* stream);

/* Bytes at the head of the workspace of the function below that hold its int32 tables for a test of n_source frames of width x
 * height: the range tables of FVVDP_RESIZE_GRAD_TABLE_BYTES (two entries per source row and column) and behind them the run table
 * of n_source + 1 entries, rounded up to 256 bytes.  Behind them the first stage keeps channels * out_height * out_width floats
 * per SOURCE frame, for as many frames at once as the workspace holds (at least one). */
#define FVVDP_RESIZE_GRAD_HELD_TABLE_BYTES(width, height, n_source) \
    (((((size_t)2 * ((size_t)(width) + (size_t)(height)) + (size_t)(n_source) + 1) * 4) + 255) / 256 * 256)

/* fvvdp_resize_grad for a test shown through a frame map: d_gL [n_display][out_height][out_width] (dense, at the display's rate)
 * and the float32 test clip of n_source frames -> d_grad, the gradient of every sample of `test`, laid out as `test` is (its
 * strides; every sample of all n_source frames written exactly once, zeros included).
 *   h_map                        [n_display]: display frame -> source frame; non-decreasing, every entry in [0, n_source).
 *                                The host turns it into the run table r [n_source + 1] -- source frame j is shown by display
 *                                frames [r[j], r[j + 1]) -- and uploads it behind the range tables;
 *   stage 1, per source frame j and target pixel   g = the sum of d_gL[v] over the run in ascending v, starting from its first
 *                                frame (a run of one adds nothing); then d_c = g w_c EOTF'(v_c) where v_c lies in [0, 1], 0
 *                                where the clip binds, as fvvdp_resize_grad.  An empty run -- a frame no display frame shows --
 *                                writes d_c = 0;
 *   stage 2                      fvvdp_resize_grad's gather, on n_source frames.
 * With the identity map the result has fvvdp_resize_grad's bits.  d_work: 256-byte aligned; no allocation is made inside the call.
 * Errors: those of fvvdp_resize_grad (n_frames: n_source), and FVVDP_EINVAL for n_display below 1 or a map that decreases or names
 * a frame outside [0, n_source). */
int fvvdp_resize_grad_held(int out_width, int out_height, int n_display, int n_source, const float* d_gL, const int32_t* h_map,
                           const fvvdp_resize_stream* test, float* d_grad, int mode, const fvvdp_eotf* eotf, const float* h_rgb2y,
                           void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_RESIZE_HELD_H */
