/*
 * fvvdp_hip_ref_grad.h -- gradients of the JOD with respect to the REFERENCE in libfvvdp_hip.so: dJOD / dreference for still
 * images and for one float clip.
 *
 * An extension, the counterpart of fvvdp_hip_grad.h and fvvdp_hip_video_grad.h (gradients with respect to the test).  It is a
 * different adjoint: the reference enters a band pixel through its own band contrast, as the local adaptation luminance L_bkg
 * that divides both contrasts, and through L_bkg as the luminance argument of the CSF look-up.  The last needs the slope of the
 * CSF interpolation, kappa = d log2 S / d log2 L_bkg, which the map-writing pyramid pass writes as one more plane per band
 * (fvvdp_ctx_set_slope_maps).  The conventions of fvvdp_hip.h apply (d_* device and h_* host pointers, return codes,
 * fvvdp_last_error, `stream` a hipStream_t passed as void*, asynchronous).
 *
 * The backward of a batch, after the forward left Q_per_ch:
 *   1. the ingest of the batch, exactly as the forward (fvvdp_images_channels / fvvdp_temporal_channels);
 *   2. fvvdp_ctx_set_slope_maps(ctx, planes), the pyramid pass with every band's maps set (fvvdp_images_forward_pool /
 *      fvvdp_bands_forward), fvvdp_ctx_set_slope_maps(ctx, NULL);
 *   3. fvvdp_images_ref_grad (the gradient of the reference images), or fvvdp_video_ref_grad_frames (the gradient of the
 *      batch's level-0 reference planes into a clip-long buffer) and, once per clip, fvvdp_video_grad_input of
 *      fvvdp_hip_video_grad.h on the reference clip and that buffer.
 * The same maps serve fvvdp_images_grad / fvvdp_video_grad_frames: both gradients of a pair come from one ingest and one
 * pyramid pass.  Every output is a fixed sum per pixel (no atomics): the result does not depend on the batching and repeats bit
 * for bit.
 */
#ifndef FVVDP_HIP_REF_GRAD_H
#define FVVDP_HIP_REF_GRAD_H

#include "fvvdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One more output of the map-writing pyramid pass: h_slope_ptrs[b] (host array of n_bands device pointers) receives
 * kappa [n][2][h_b][w_b] fp32 of band b, plane cc = temporal channel (an image context writes plane 0 only), whenever a later
 * fvvdp_bands_forward* / fvvdp_images_forward_pool call on this context is given maps for that band.  kappa is the blend, over
 * the rho and eccentricity neighbours of the pixel's LUT cell, of (v[j+1] - v[j]) / (Y_log[j+1] - Y_log[j] + 1e-6); it is 0
 * where L_bkg lies outside the table's luminance range and where the query falls on the first knot.  The pointers stay set
 * until the next call; NULL (or a NULL entry) switches the output off.  Host state only: no launch, no synchronisation.
 * Errors: FVVDP_EINVAL (null context, misaligned pointer). */
int fvvdp_ctx_set_slope_maps(fvvdp_ctx* ctx, float* const* h_slope_ptrs);

/* Bytes of device workspace for a batch of n image pairs (planes = 1) or n video frames (planes = 2) of width x height with
 * n_bands band-pass levels.  Layout, in floats, each part 64-float (256 B) aligned, P = planes, (w_b, h_b) the ceil(/2) level sizes:
 *   coef [n][P][n_bands] | GLR_b [n][P][h_b][w_b] for b in [0, n_bands) | GG_L [n][P][h_L][w_L] for L in [1, n_bands]
 *   | GX_b [n][P][h_b][w_b] for b in [0, n_bands)
 * Errors: FVVDP_EINVAL (null output, non-positive sizes, n_bands outside [1, FVVDP_MAX_BANDS], planes not 1 or 2). */
int fvvdp_ref_grad_workspace(int width, int height, int n_bands, int n, int planes, size_t* bytes);

/* d_grad[k][c][y][x] = gamma[k] * dJOD_k / dreference_k[c][y][x].  The arguments of fvvdp_images_grad (fvvdp_hip_grad.h), with the
 * REFERENCE images in h_ref_ptrs, and
 *   h_slope_ptrs                 n_bands device pointers: the slope planes the pyramid pass of step 2 wrote.
 * Launches: coefficients, the reference layer gradients (all bands), one sweep per level, level 0 + display model. */
int fvvdp_images_ref_grad(int width, int height, int n_bands, int n, const fvvdp_params* prm, const fvvdp_pool_params* pool,
                          const float* d_Q, int q_stride, int q_col0, const float* d_gamma, const fvvdp_band_maps* maps,
                          const float* const* h_slope_ptrs, const void* const* h_ref_ptrs, int C, size_t chan_stride,
                          const fvvdp_eotf* eotf, const float* h_rgb2y, void* const* h_grad_ptrs, void* d_work, size_t work_bytes,
                          void* stream);

/* d_g0[f0 + k][cc][y][x] = gamma * dJOD / d(level 0, reference plane of temporal channel cc, frame f0 + k) for k in [0, n).
 * The arguments of fvvdp_video_grad_frames (fvvdp_hip_video_grad.h), and h_slope_ptrs as above.
 * Launches: coefficients, the reference layer gradients (all bands, both channels per thread), one sweep per level, level 0. */
int fvvdp_video_ref_grad_frames(int width, int height, int n_bands, int n, const fvvdp_params* prm, const fvvdp_pool_params* pool,
                                const float* d_Q, int n_frames, int f0, const float* d_gamma, const fvvdp_band_maps* maps,
                                const float* const* h_slope_ptrs, float* d_g0, void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_REF_GRAD_H */
