/*
 * fvvdp_hip_gaze_grad.h -- gradients of the video JOD under many gazes in libfvvdp_hip.so (foveated mode, stock display
 * geometry): sum_g gamma[g] * dJOD_g / dtest for one float clip scored under G gaze traces.
 *
 * An extension, where fvvdp_hip_gaze.h (one clip, many gazes, forward) and fvvdp_hip_video_grad.h (one gaze, backward) meet.
 * Of the backward of a clip, only two small steps depend on the gaze: the pooling coefficients (from gaze g's Q_per_ch) and
 * the pointwise layer gradient, through the CSF sensitivity of a band pixel at its eccentricity.  Everything after them is
 * linear in the layer gradient.  The functions below therefore sum the layer gradients of all gazes first and run the
 * coarse-to-fine sweep and level 0 once; the ingest, the map-writing pyramid pass before them and fvvdp_video_grad_input after
 * them are the caller's, once per batch and once per clip, whatever the number of gazes.  The conventions of fvvdp_hip.h
 * apply (d_* device and h_* host pointers, return codes, fvvdp_last_error, `stream` a hipStream_t passed as void*,
 * asynchronous).  No context is needed: the functions read only what they are given, allocate nothing and never synchronise.
 *
 * The backward of a clip of N frames whose forward (fvvdp_bands_forward_gazes_pool) left Q_per_ch [G][n_bands][2][N]:
 *   for every batch of n output frames [f0, f0 + n) (slots [0, n) of a video context):
 *     1. fvvdp_temporal_channels with the batch's slice of the window index list, exactly as the forward;
 *     2. fvvdp_bands_forward with every band's maps set, under ANY one gaze (the contrast and L_bkg maps do not depend on
 *        it; the D and S maps do and are not read here);
 *     3. fvvdp_gaze_grad_frames: columns [f0, f0 + n) of the clip-long buffer d_g0 [N][2][H][W];
 *   then once: fvvdp_video_grad_input (fvvdp_hip_video_grad.h).
 * Every output is a fixed sum per pixel, the gazes in ascending order (no atomics): the result does not depend on the
 * batching nor on how the gazes are grouped into launches, and repeats bit for bit.
 */
#ifndef FVVDP_HIP_GAZE_GRAD_H
#define FVVDP_HIP_GAZE_GRAD_H

#include "fvvdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device workspace for a batch of n frames of width x height with n_bands band-pass levels under n_gazes gazes:
 * the workspace of the single-gaze backward (fvvdp_hip_video_grad.h: one set of layer and sweep gradients, whatever n_gazes)
 * followed by the coefficients of every gaze, [n_gazes] blocks of [n][2][n_bands] floats, each rounded up to 64 floats.
 * Errors: FVVDP_EINVAL (null output, non-positive sizes, n_bands outside [1, FVVDP_MAX_BANDS], n_gazes < 1). */
int fvvdp_gaze_grad_workspace(int width, int height, int n_bands, int n, int n_gazes, size_t* bytes);

/* d_g0[f0 + k][cc][y][x] = sum_g gamma[g] * dJOD_g / d(level 0, test plane of temporal channel cc, frame f0 + k), k in [0, n).
 *   width, height, n_bands, prm  geometry and model constants of the context the maps came from;
 *   group_max                    largest group of gazes one layer launch takes: 0 (the default, 8), 1, 2, 4 or 8; the result
 *                                does not depend on it, bit for bit (smaller groups: more launches; tests and A/B runs);
 *   pool                         the pooling parameters of the forward;
 *   geom                         the stock display geometry of the forward (required);
 *   h_rho_band                   host, [n_bands] centre frequencies of the bands in cycles per degree, as fvvdp_ctx_create;
 *   d_S_log0, d_S_log1           device, the 32^3 CSF tables of the sustained and the transient channel, [Y][rho][ecc],
 *                                as fvvdp_ctx_set_csf_3d takes them on the host;
 *   d_axes, h_axes               the knots [3][32] of the tables' axes (Y_log, rho_log, ecc_sqrt), on the device and on
 *                                the host; the host copy gives the clamps and the grid.  The caller's contract: both hold
 *                                the same values -- the call cannot compare them without a synchronisation and does not;
 *   d_gaze, gaze_stride          device, gaze g of frame f0 + k at d_gaze[g * gaze_stride + 2 * k]: (x, y) in frame pixels,
 *                                as fvvdp_bands_forward_gazes (gaze_stride >= 2 n floats: a clip-long [G][N][2] array is
 *                                passed with gaze_stride = 2 N and the pointer advanced by 2 * f0);
 *   d_Q, n_frames                Q_per_ch of the FORWARD pass of the whole clip under every gaze, [n_gazes][n_bands][2][n_frames];
 *   f0, n                        the batch: frames [f0, f0 + n) of the clip, 0 <= f0, f0 + n <= n_frames;
 *   d_gamma                      float[n_gazes], the upstream gradient of every gaze's JOD (device; a gaze with gamma 0 adds
 *                                exact zeros);
 *   maps                         n_bands records, every pointer set, holding the n frames of step 2 above (d_contrast
 *                                [n][4] and d_lbkg [n] planes of h_b x w_b are read);
 *   d_g0                         the clip-long output [n_frames][2][height][width] fp32;
 *   d_work, work_bytes           workspace of at least fvvdp_gaze_grad_workspace bytes, 256-byte aligned.
 * Launches: the coefficients once per gaze, the layer gradients of all bands once per group of gazes (groups of 8, 4, 2, 1;
 * the first group stores, later groups add in order), then one sweep per level and level 0, once.
 * Errors: FVVDP_EINVAL (null pointer, bad shape, n_gazes < 1, a group_max other than 0, 1, 2, 4, 8, gaze_stride < 2 n, frames
 * outside the clip, a geometry that is not positive, maps missing, misaligned or small workspace). */
int fvvdp_gaze_grad_frames(int width, int height, int n_bands, int n, int n_gazes, int group_max, const fvvdp_params* prm,
                           const fvvdp_pool_params* pool, const fvvdp_geom* geom, const double* h_rho_band,
                           const float* d_S_log0, const float* d_S_log1, const float* d_axes, const float* h_axes,
                           const float* d_gaze, size_t gaze_stride, const float* d_Q, int n_frames, int f0,
                           const float* d_gamma, const fvvdp_band_maps* maps, float* d_g0, void* d_work, size_t work_bytes,
                           void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_GAZE_GRAD_H */
