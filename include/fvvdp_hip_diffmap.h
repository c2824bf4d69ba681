/*
 * fvvdp_hip_diffmap.h -- the difference map as a differentiable quantity in libfvvdp_hip.so: the pre-power reconstruction
 * v_0 and the gradient of a per-pixel cotangent of the map with respect to the test images or the test clip.
 *
 * An extension.  The conventions of fvvdp_hip.h apply (d_* device and h_* host pointers, return codes, fvvdp_last_error,
 * `stream` a hipStream_t passed as void*, asynchronous).  The gradient functions need no context: they read only what they
 * are given.
 *
 * Forward, per pair or frame, from the difference maps D_b of a forward pass with maps (fvvdp_band_maps.d_D, [n][2][h_b][w_b]):
 *   v_b = Expand(v_{b+1}) + (D_b[0] + w_transient D_b[1]) / m_b      m_0 = 1, m_b = 2 for b >= 1; the coarsest band has no
 *                                                                     coarse term; a still image has channel 0 only
 *   units FVVDP_DIFFMAP_JOD:     map = v_0^beta_jod |jod_a|           (what fvvdp_heatmap_reconstruct writes)
 *   units FVVDP_DIFFMAP_LINEAR:  map = v_0                            (what fvvdp_heatmap_reconstruct_linear writes)
 * Backward for a cotangent G [n][H][W] of the map, one launch per level, fine to coarse:
 *   A_0 = G beta_jod |jod_a| v_0^(beta_jod - 1)  (JOD; 0 where v_0 == 0),   A_0 = G  (LINEAR)
 *   A_b = Expand^T(A_{b-1})                                           the exact transposed gather of the forward stencil
 *   GL_b[cc] = (A_b w_cc / m_b) dD/dT' S gain m_b / L_bkg             w_0 = 1, w_1 = w_transient; 0 where D == 0 and where the
 *                                                                     d_max clamp or the contrast clamp binds
 * then the coarse-to-fine sweep and level 0 of fvvdp_images_grad / fvvdp_video_grad_frames, unchanged.  Every output is a
 * fixed sum per pixel (no atomics): an entry's result does not depend on the batch it ran in and repeats bit for bit.
 */
#ifndef FVVDP_HIP_DIFFMAP_H
#define FVVDP_HIP_DIFFMAP_H

#include "fvvdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FVVDP_DIFFMAP_JOD 0
#define FVVDP_DIFFMAP_LINEAR 1

/* fvvdp_heatmap_reconstruct (fvvdp_hip.h) without its final power and scale: d_out [n][H][W] = v_0.  The same launches of the
 * same kernel on the same scratch of the context; only the last step of level 0 is left out. */
int fvvdp_heatmap_reconstruct_linear(fvvdp_ctx* ctx, int n, const float* const* h_dD, float w_transient, float* d_out,
                                     void* stream);

/* Bytes of device workspace the gradient functions below need for a batch of n entries with `channels` temporal channels
 * (1: image pairs, 2: video frames).  Layout, in floats, each part 64-float (256 B) aligned, (w_b, h_b) the ceil(/2) level sizes:
 *   the workspace of fvvdp_images_grad_workspace (channels == 1) or fvvdp_video_grad_workspace (channels == 2)
 *   | A_b [n][h_b][w_b] for b in [0, n_bands)
 * h_gl_offsets, h_a_offsets: size_t[n_bands] or NULL; they receive the offsets, in floats, of GL_b [n][channels][h_b][w_b]
 * and of A_b.  Errors: FVVDP_EINVAL (null output, bad sizes, channels not 1 or 2). */
int fvvdp_diffmap_grad_workspace(int width, int height, int n_bands, int n, int channels, size_t* h_gl_offsets,
                                 size_t* h_a_offsets, size_t* bytes);

/* The per-level launches alone: A_b and GL_b of every band into the workspace (for callers that continue on their own, and
 * for tests of the kernel).
 *   prm, pool      model constants of the context the maps came from; of `pool` w_transient, jod_a and beta_jod are read;
 *   units          FVVDP_DIFFMAP_JOD or FVVDP_DIFFMAP_LINEAR;
 *   d_G            [n][height][width] cotangent of the map;
 *   d_v0           [n][height][width] from fvvdp_heatmap_reconstruct_linear (JOD; ignored and may be NULL for LINEAR);
 *   maps           n_bands records, every pointer set: d_D [n][2], d_contrast [n][2 channels], d_lbkg [n], d_S [n][2] planes.
 * Errors: FVVDP_EINVAL (null or misaligned pointer, bad shape or units, small workspace). */
int fvvdp_diffmap_grad_levels(int width, int height, int n_bands, int n, int channels, const fvvdp_params* prm,
                              const fvvdp_pool_params* pool, int units, const float* d_G, const float* d_v0,
                              const fvvdp_band_maps* maps, void* d_work, size_t work_bytes, void* stream);

/* h_grad_ptrs[k][c][y][x] = sum over the pixels of G[k] dmap_k / dtest_k[c][y][x] for n image pairs: the per-level launches,
 * the sweep and the level-0 kernel of fvvdp_images_grad_st (test images, dtype, C, chan_stride, eotf, h_rgb2y and gradient
 * pointers as it takes them; channels = 1). */
int fvvdp_diffmap_images_grad(int width, int height, int n_bands, int n, const fvvdp_params* prm, const fvvdp_pool_params* pool,
                              int units, const float* d_G, const float* d_v0, const fvvdp_band_maps* maps,
                              const void* const* h_test_ptrs, int dtype, int C, size_t chan_stride, const fvvdp_eotf* eotf,
                              const float* h_rgb2y, void* const* h_grad_ptrs, void* d_work, size_t work_bytes, void* stream);

/* d_g0[f0 + k][cc][y][x] = the gradient with respect to level 0's test plane of temporal channel cc, frame f0 + k, for the n
 * frames of a batch: the per-level launches (channels = 2), the sweep and the level-0 kernel of fvvdp_video_grad_frames into
 * the clip-long buffer d_g0 [n_frames][2][height][width]; fvvdp_video_grad_input(_st) turns it into the clip's gradient.
 * d_G and d_v0 hold the batch's n frames. */
int fvvdp_diffmap_video_grad_frames(int width, int height, int n_bands, int n, const fvvdp_params* prm,
                                    const fvvdp_pool_params* pool, int units, const float* d_G, const float* d_v0, int n_frames,
                                    int f0, const fvvdp_band_maps* maps, float* d_g0, void* d_work, size_t work_bytes,
                                    void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_DIFFMAP_H */
