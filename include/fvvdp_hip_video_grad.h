/*
 * fvvdp_hip_video_grad.h -- gradients of the video JOD in libfvvdp_hip.so: dJOD / dtest for one float clip.
 *
 * An extension, the video counterpart of fvvdp_hip_grad.h: the adjoint of what fvvdp_temporal_channels + fvvdp_bands_forward +
 * fvvdp_pool_jod compute for float32 samples behind a closed-form display model, with respect to the TEST clip only (the
 * reference clip -- background luminance L_bkg, CSF sensitivity S -- is a constant).  The conventions of fvvdp_hip.h apply
 * (d_* device and h_* host pointers, return codes, fvvdp_last_error, `stream` a hipStream_t passed as void*, asynchronous).
 * No context is needed: the functions read only what they are given, so any call on any context may run between the
 * forward and the backward.
 *
 * The backward of a clip of N frames whose forward left Q_per_ch [n_bands][2][N]:
 *   for every batch of n output frames [f0, f0 + n) (slots [0, n) of a video context):
 *     1. fvvdp_temporal_channels with the batch's slice of the window index list, exactly as the forward;
 *     2. fvvdp_bands_forward with every band's maps set (fvvdp_band_maps: d_D [n][2], d_contrast [n][4], d_lbkg [n],
 *        d_S [n][2] planes of h_b x w_b);
 *     3. fvvdp_video_grad_frames: the gradient with respect to the batch's level-0 test planes (sustained, transient)
 *        into columns [f0, f0 + n) of the clip-long buffer d_g0 [N][2][H][W];
 *   then once: fvvdp_video_grad_input -- the transpose of the sliding-window temporal filter and the display model's
 *   derivative: d_g0 -> dJOD / dtest.
 * Every output is a fixed sum per pixel (no atomics): the result does not depend on the batching and repeats bit for bit.
 */
#ifndef FVVDP_HIP_VIDEO_GRAD_H
#define FVVDP_HIP_VIDEO_GRAD_H

#include "fvvdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Longest temporal filter the transpose kernel of fvvdp_video_grad_input covers (its register ring has 8 / 16 / 32 / 64
 * slots): 64 taps, i.e. up to 256 frames per second.  Longer filters (up to FVVDP_MAX_TAPS) are REFUSED with
 * FVVDP_EUNSUPPORTED and a sentence; there is no slower generic path. */
#define FVVDP_VIDEO_GRAD_MAX_TAPS 64

/* Bytes of device workspace fvvdp_video_grad_frames needs for a batch of n frames of width x height with n_bands band-pass
 * levels.  Layout, in floats, each part 64-float (256 B) aligned, (w_b, h_b) the ceil(/2) level sizes:
 *   coef [n][2][n_bands] | GL_b [n][2][h_b][w_b] for b in [0, n_bands) | GG_L [n][2][h_L][w_L] for L in [1, n_bands]
 * Errors: FVVDP_EINVAL (null output, non-positive sizes, n_bands outside [1, FVVDP_MAX_BANDS]). */
int fvvdp_video_grad_workspace(int width, int height, int n_bands, int n, size_t* bytes);

/* d_g0[f0 + k][cc][y][x] = gamma * dJOD / d(level 0, test plane of temporal channel cc, frame f0 + k) for k in [0, n).
 *   width, height, n_bands, prm  geometry and model constants of the context the maps came from;
 *   pool                         the pooling parameters of the forward;
 *   d_Q, n_frames                Q_per_ch of the FORWARD pass of the whole clip, [n_bands][2][n_frames] (every column is
 *                                read: the pooling over frames does not drop out of the chain);
 *   f0, n                        the batch: frames [f0, f0 + n) of the clip, 0 <= f0, f0 + n <= n_frames;
 *   d_gamma                      float[1], the upstream gradient of the JOD (device);
 *   maps                         n_bands records, every pointer set, holding the n frames of step 2 above;
 *   d_g0                         the clip-long output [n_frames][2][height][width] fp32;
 *   d_work, work_bytes           workspace of at least fvvdp_video_grad_workspace bytes, 256-byte aligned.
 * Launches: coefficients, layer gradients (all bands, both channels per thread), one sweep per level, level 0. */
int fvvdp_video_grad_frames(int width, int height, int n_bands, int n, const fvvdp_params* prm, const fvvdp_pool_params* pool,
                            const float* d_Q, int n_frames, int f0, const float* d_gamma, const fvvdp_band_maps* maps,
                            float* d_g0, void* d_work, size_t work_bytes, void* stream);

/* d_grad[c][j][y][x] = w_c EOTF'(test[c][j][y][x]) * sum over the window-list positions p that show frame j of
 *                      A[p] = sum_cc sum_k taps[cc][k] g0[p - (fl - 1) + k][cc]   (terms outside [0, n_frames) dropped).
 * The forward's window index list has n_frames + fl - 1 entries: a HEAD of fl entries chosen by the temporal padding, then
 * frames 1 .. n_frames - 1 in order (position p >= fl shows frame p - fl + 1).  The streaming part is implied; the head is
 * passed as a fold list:
 *   h_fold_frame, h_fold_pos     int32[fl]: head position h_fold_pos[i] in [0, fl) shows frame h_fold_frame[i] in
 *                                [0, n_frames); every head position exactly once, sorted by frame, then by position;
 *   d_g0                         [n_frames][2][height][width] from fvvdp_video_grad_frames;
 *   h_taps, fl                   [2][fl] temporal filters as fvvdp_temporal_channels takes them; 1 <= fl <= FVVDP_MAX_TAPS,
 *                                above FVVDP_VIDEO_GRAD_MAX_TAPS: FVVDP_EUNSUPPORTED;
 *   d_test, d_grad               float32 clips, element (c, f, y, x) at c*chan_stride + f*frame_stride + y*width + x;
 *   C, eotf, h_rgb2y             as the forward's fvvdp_temporal_channels: C in {1, 3}; a closed form (SRGB, GAMMA, PQ,
 *                                LINEAR or ABSOLUTE); samples that the model clamps get a zero gradient;
 *   d_head, head_bytes           side buffer of at least fl * height * width floats for the head positions' sums.
 * One launch: a lane owns a few consecutive pixels for the whole clip and walks the list positions once with the fl partial
 * sums in registers, so every g0 value and every test sample is read once and every gradient sample written once
 * (8 + 8 C bytes per pixel and frame).  16-byte accesses when height * width and the strides are multiples of 4 and the
 * pointers 16-byte aligned (8-byte above 16 taps); a per-pixel variant of the same kernel otherwise.
 * Errors: FVVDP_EINVAL (null or misaligned pointer, bad shape, display model, fold list, small side buffer). */
int fvvdp_video_grad_input(int width, int height, int n_frames, const float* d_g0, const int32_t* h_fold_frame,
                           const int32_t* h_fold_pos, const float* h_taps, int fl, const float* d_test, float* d_grad, int C,
                           size_t chan_stride, size_t frame_stride, const fvvdp_eotf* eotf, const float* h_rgb2y,
                           float* d_head, size_t head_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_VIDEO_GRAD_H */
