/*
 * fvvdp_hip_grad.h -- gradients of the still-image JOD in libfvvdp_hip.so: dJOD_k / dtest_k for a batch of float image pairs.
 *
 * An extension: the reference is plain torch, so its metric is differentiable (pyfvvdp/fvvdp.py:56, 302-304).  This is the
 * adjoint of what fvvdp_images_channels + fvvdp_images_forward_pool (fvvdp_hip_images.h) compute for float32 samples behind
 * a closed-form display model, with respect to the TEST image only: the reference image (background luminance L_bkg,
 * CSF sensitivity S) is a constant.  The conventions of fvvdp_hip.h apply (d_* device and h_* host pointers, return codes,
 * fvvdp_last_error, `stream` a hipStream_t passed as void*, asynchronous).  No context is needed: the function reads
 * only what it is given, so any call on any context may run between the forward and the backward.
 *
 * A backward batch of n pairs (slots [0, n) of a still-image context, test images on the device):
 *   1. fvvdp_images_channels, then fvvdp_images_forward_pool with every band's maps set (fvvdp_band_maps: d_D, d_contrast,
 *      d_lbkg, d_S, each [n][...][h_b][w_b] as fvvdp_hip.h describes) -- the band contrast, L_bkg, S and D of every pixel;
 *   2. fvvdp_images_grad: the gradient of every pair's JOD into the caller's buffers.
 * Per pair the arithmetic is fixed per pixel (no atomics), so a pair's gradient does not depend on its batch or slot.
 */
#ifndef FVVDP_HIP_GRAD_H
#define FVVDP_HIP_GRAD_H

#include "fvvdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device workspace fvvdp_images_grad needs for n pairs of width x height with n_bands band-pass levels (the same
 * n_bands as the context's).  Layout, in floats, each part 64-float (256 B) aligned, (w_b, h_b) the ceil(/2) level sizes:
 *   coef [n][n_bands] | GL_b [n][h_b][w_b] for b in [0, n_bands) | GG_L [n][h_L][w_L] for L in [1, n_bands]
 * (the layout of fvvdp_video_grad_workspace with one plane per batch entry).  After the call coef holds the pooling coefficient
 * of every pair and band, GL_b the gradient of the test's layer of band b and GG_L the gradient of the Gaussian level L.
 * Errors: FVVDP_EINVAL (null output, non-positive sizes, n_bands outside [1, FVVDP_MAX_BANDS]). */
int fvvdp_images_grad_workspace(int width, int height, int n_bands, int n, size_t* bytes);

/* h_grad_ptrs[k][c][y][x] = gamma[k] * dJOD_k / dtest_k[c][y][x] for pairs k in [0, n).
 *   width, height, n_bands, prm  the geometry and model constants of the context the maps came from (fvvdp_ctx_create);
 *   pool                         the pooling parameters the forward used (fvvdp_pool_params);
 *   d_Q, q_stride, q_col0        Q_per_ch of the FORWARD pass ([band][2][q_stride], pair k in column q_col0 + k): the
 *                                per-band scale factors of the chain come from it, the maps supply the per-pixel terms;
 *   d_gamma                      float[n], the upstream gradient of each JOD (device);
 *   maps                         n_bands records, every pointer set, holding the n pairs of step 1 above;
 *   h_test_ptrs, C, chan_stride  host array of n DEVICE pointers to the float32 test images [C][H][W] of step 1 (channel c
 *                                at c * chan_stride elements; C is 1 or 3);
 *   eotf, h_rgb2y                the display model and the RGB->Y weights of step 1: a closed form (SRGB, GAMMA, PQ,
 *                                LINEAR or ABSOLUTE); samples that the model clamps get a zero gradient;
 *   h_grad_ptrs                  host array of n DEVICE pointers to float32 [C][H][W] outputs (channel c at c * chan_stride);
 *   d_work, work_bytes           device workspace of at least fvvdp_images_grad_workspace bytes.
 * Launches: one per pyramid level (coefficients, layer gradients, coarse-to-fine sweep) and one input-gradient launch per
 * 128 pairs.  Errors: FVVDP_EINVAL (null or misaligned pointer, bad shape, unsupported display model, small workspace). */
int fvvdp_images_grad(int width, int height, int n_bands, int n, const fvvdp_params* prm, const fvvdp_pool_params* pool,
                      const float* d_Q, int q_stride, int q_col0, const float* d_gamma, const fvvdp_band_maps* maps,
                      const void* const* h_test_ptrs, int C, size_t chan_stride, const fvvdp_eotf* eotf,
                      const float* h_rgb2y, void* const* h_grad_ptrs, void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_GRAD_H */
