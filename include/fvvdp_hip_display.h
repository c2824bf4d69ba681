/*
 * fvvdp_hip_display.h -- the sums behind the gradient of the JOD with respect to the DISPLAY's photometry in libfvvdp_hip.so:
 * what a fit or a search over Y_peak, contrast, E_ambient, k_refl and gamma of fvvdp_display_photo_eotf needs from the device.
 *
 * An extension.  The display model enters the metric only before level 0 of the pyramid.  With
 *   Y_black = E_ambient k_refl / pi + Y_peak / contrast,   scale = Y_peak - Y_black
 * the luminance of a channel sample V is  scale f(clamp01 V) + Y_black  (FVVDP_EOTF_SRGB, FVVDP_EOTF_GAMMA: f = V^gamma) or
 * clip(g(V), 0.005, Y_peak) + Y_black  (FVVDP_EOTF_PQ, FVVDP_EOTF_LINEAR), and a frame's luminance is sum_c w_c L(V_c) (w = 1
 * for C = 1).  Let s[j][x] be dJOD / d(luminance of source frame j at pixel x).  Per stream (test, reference) three sums suffice:
 *   out[0] = U0 = sum s sum_c w_c                    the derivative for Y_black;
 *   out[1] = U1 = sum s sum_c w_c a1(V_c)            SRGB / GAMMA: a1 = f(clamp01 V), the derivative for scale (not zero at a
 *                                                    clamped sample); PQ / LINEAR: a1 = 1 where the upper luminance clip binds,
 *                                                    the derivative for Y_peak at fixed Y_black;
 *   out[2] = U2 = sum s sum_c w_c scale V^gamma ln V GAMMA only (exactly 0 at V <= 0): the derivative for gamma; 0 otherwise.
 * The map from the sums of both streams to the gradient for the five parameters is host arithmetic on six numbers
 * (fovvideovdp_amd/display_grad.py).  The conventions of fvvdp_hip.h apply (d_* device and h_* host pointers, return codes,
 * fvvdp_last_error, `stream` a hipStream_t passed as void*, asynchronous).  No context is needed.
 *
 * Both entry points accumulate alike: products and sums in fp32 (fused multiply-adds) over at most 16 terms -- the pixels of one
 * lane times the channels of one frame -- then fp64 in a fixed order: per lane, shuffles inside the wave, the four waves through
 * the LDS, one partial per workgroup, a second launch that adds the partials in order.  No atomics; a result repeats bit for bit.
 */
#ifndef FVVDP_HIP_DISPLAY_H
#define FVVDP_HIP_DISPLAY_H

#include "fvvdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sums per stream. */
#define FVVDP_DISPLAY_SUMS 3

/* Bytes of device workspace of fvvdp_video_display_sums for frames of width x height:
 *   partial [ceil(height width / 256)][FVVDP_DISPLAY_SUMS] fp64.
 * Errors: FVVDP_EINVAL (null output, bad frame size). */
int fvvdp_video_display_sums_workspace(int width, int height, size_t* bytes);

/* The three sums of one stream of a clip.  s[j] = sum over the window positions that show frame j of
 * sum_cc sum_k taps[cc][k] g0[p - (fl - 1) + k][cc]: the temporal transpose of fvvdp_video_grad_input
 * (fvvdp_hip_video_grad.h), the same values in the same order.
 *   width, height, n_frames, d_g0, h_fold_frame, h_fold_pos, h_taps, fl, C, chan_stride, frame_stride, eotf, h_rgb2y, d_head,
 *   head_bytes          as fvvdp_video_grad_input takes them; d_g0 the clip-long level-0 gradient of the stream
 *                       (fvvdp_video_grad_frames for the test, fvvdp_video_ref_grad_frames for the reference, made with
 *                       gamma = 1); eotf: SRGB, GAMMA, PQ or LINEAR;
 *   d_src               the stream's float32 clip;
 *   d_out               [FVVDP_DISPLAY_SUMS] fp64, 8-byte aligned;
 *   d_work, work_bytes  workspace of at least fvvdp_video_display_sums_workspace bytes, 256-byte aligned.
 * A lane owns 4 (fl <= 16), 2 or 1 pixels as in fvvdp_video_grad_input and walks the window positions once; per pixel and frame it
 * reads 8 B of d_g0 and 4 C B of samples and writes nothing but the head (fl frames).  A frame that no window shows contributes
 * exact zeros.
 * Launches: the walk, the final add.
 * Errors: FVVDP_EINVAL (null or misaligned pointer, bad shape, fold list, side buffer or workspace too small, fl outside
 * [1, FVVDP_MAX_TAPS]); FVVDP_EUNSUPPORTED (fl above 64; a display model without the five parameters: ABSOLUTE, LUT, NONE). */
int fvvdp_video_display_sums(int width, int height, int n_frames, const float* d_g0, const int32_t* h_fold_frame,
                             const int32_t* h_fold_pos, const float* h_taps, int fl, const float* d_src, int C,
                             size_t chan_stride, size_t frame_stride, const fvvdp_eotf* eotf, const float* h_rgb2y,
                             float* d_head, size_t head_bytes, double* d_out, void* d_work, size_t work_bytes, void* stream);

/* Bytes of device workspace of fvvdp_images_display_sums for n pairs: the workspace of fvvdp_images_grad (reference == 0;
 * fvvdp_hip_grad.h) or of fvvdp_images_ref_grad (reference != 0; fvvdp_hip_ref_grad.h), rounded up to 256 bytes, followed by
 *   partial [n][ceil(height width / 256)][FVVDP_DISPLAY_SUMS] fp64.
 * Errors: FVVDP_EINVAL (null output, bad shape). */
int fvvdp_images_display_sums_workspace(int width, int height, int n_bands, int n, int reference, size_t* bytes);

/* The three sums of one stream of n image pairs, d_out[k][FVVDP_DISPLAY_SUMS] fp64: the launches of fvvdp_images_grad
 * (h_slope_ptrs == NULL: the test side) or of fvvdp_images_ref_grad (the slope planes given: the reference side) up to level 1
 * of the sweep -- coefficients, layer kernel, sweep -- and in the place of their last kernel a reduction that forms
 * g0 = GL_0 + Reduce^T(GG_1) per pixel and sums g0 w_c {1, a1, a2} over the pair.
 *   width .. maps, C, chan_stride, eotf, h_rgb2y   as fvvdp_images_grad takes them; d_gamma [n] scales pair k's sums (pass ones
 *                       for dJOD_k / dpsi itself); eotf: SRGB, GAMMA, PQ or LINEAR;
 *   h_slope_ptrs        NULL, or the slope planes fvvdp_images_ref_grad takes;
 *   h_img_ptrs          the float32 images of the stream (test or reference), one pointer per pair;
 *   d_out               [n][FVVDP_DISPLAY_SUMS] fp64, 8-byte aligned;
 *   d_work, work_bytes  workspace of at least fvvdp_images_display_sums_workspace bytes, 256-byte aligned.
 * Launches: those of the gradient entry point without its last, the reduction (128 pairs a launch), the final add.
 * Errors: FVVDP_EINVAL as fvvdp_images_grad / fvvdp_images_ref_grad, and for d_out; FVVDP_EUNSUPPORTED (ABSOLUTE, LUT, NONE). */
int fvvdp_images_display_sums(int width, int height, int n_bands, int n, const fvvdp_params* prm,
                              const fvvdp_pool_params* pool, const float* d_Q, int q_stride, int q_col0, const float* d_gamma,
                              const fvvdp_band_maps* maps, const float* const* h_slope_ptrs, const void* const* h_img_ptrs,
                              int C, size_t chan_stride, const fvvdp_eotf* eotf, const float* h_rgb2y, double* d_out,
                              void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_DISPLAY_H */
