/*
 * fvvdp_hip_params.h -- the model parameters as variables in libfvvdp_hip.so: what a calibration of the metric (a fit of
 * fvvdp_parameters.json to subjective data) needs from the device.
 *
 * An extension; the reference differentiates its torch graph with respect to its parameters (the constructor's use_checkpoints
 * "for training the model").  Here the parameters enter after the pyramid: pointwise in the masking model (mask_p, mask_q,
 * mask_c, sensitivity_correction, beta, pyfvvdp/fvvdp.py:447, 574-596, 598-607) and in the pooling stage (fvvdp.py:337-357).  The
 * map-writing pyramid pass (fvvdp_band_maps of fvvdp_hip.h) leaves every band's contrast, S and D in memory; five sums over a
 * band's pixels are all the masking parameters' derivatives need, the rest is arithmetic on [bands, 2, frames] arrays that the
 * caller does (fovvideovdp_amd/param_grad.py).  The conventions of fvvdp_hip.h apply (d_* device and h_* host pointers, return
 * codes, fvvdp_last_error, `stream` a hipStream_t passed as void*, asynchronous).
 */
#ifndef FVVDP_HIP_PARAMS_H
#define FVVDP_HIP_PARAMS_H

#include "fvvdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Replaces the model constants of a live context: every later call on it evaluates the metric under *prm.  Host state only: no
 * allocation, no launch, no synchronisation, no new choice of the level-0 ranges; everything the kernels take from the
 * constants (log2 of the gain, of mask_k and of d_max, 1 / beta) is derived when a call fills its launch arguments.  Work already
 * queued on a stream keeps the constants it was launched with.
 * Errors: FVVDP_EINVAL (null argument; a constant that is not finite; mask_p, beta, mask_k, sens_gain, contrast_max or d_max not
 * positive; lbkg_min negative): the context keeps the constants it had. */
int fvvdp_ctx_set_params(fvvdp_ctx* ctx, const fvvdp_params* prm);

#define FVVDP_PARAM_SUMS 5
/* Band pixels one workgroup of fvvdp_param_sums sums: the partial sums are indexed by (band, run of this many pixels, slot). */
#define FVVDP_PARAM_SUMS_BLOCK_PX 4096

/* Bytes of device workspace of fvvdp_param_sums for n slots of width x height with n_bands band-pass levels:
 *   partial [sum_b ceil(h_b w_b / FVVDP_PARAM_SUMS_BLOCK_PX)][n][2][FVVDP_PARAM_SUMS] fp64, (w_b, h_b) the ceil(/2) level sizes.
 * Errors: FVVDP_EINVAL (null output, non-positive sizes, n above 65535, n_bands outside [1, FVVDP_MAX_BANDS]). */
int fvvdp_param_sums_workspace(int width, int height, int n_bands, int n, size_t* bytes);

/* For every band b, temporal channel cc and slot k of a map-writing pass over n slots (fvvdp_bands_forward* /
 * fvvdp_images_forward_pool with maps; planes = 2: still images, cc = 0 only, or 4: video), five sums over the band's pixels.
 * With T, R the band contrasts (maps[b].d_contrast, planes 2cc and 2cc + 1), S the sensitivity (d_S, plane cc) and D the
 * forward's own difference value (d_D, plane cc):
 *   T' = T S sens_gain,  R' = R S sens_gain,  u = |T' - R'|,  M = mask_k min(|T'|, |R'|),  a = M^q / (1 + M^q),  q = mask_q[cc]
 *   s0 = sum_live D^beta          s1 = sum_live D^beta ln u          s2 = sum_live D^beta a ln M
 *   s3 = sum_live D^beta a        s4 = sum_{D > 0} D^beta ln D
 * A pixel is live where 0 < D < d_max, i.e. where D depends on the masking parameters: a pixel at the d_max clamp enters s4
 * only.  The maps hold the clamped value after rounding, so a value within 2^-20 of d_max counts as clamped, as in the
 * backward passes of fvvdp_hip_grad.h.  A term with D = 0, u = 0 or M = 0 is exactly 0 (never 0 x inf); values below the
 * smallest normal fp32 number count as 0.
 *   d_sums   [n_bands][2][n][FVVDP_PARAM_SUMS] fp64; plane cc = 1 is written as 0 for planes == 2
 *   d_work   workspace of fvvdp_param_sums_workspace, 256-byte aligned
 * Pixel terms in fp32 (the forward's log2 / exp2 instructions), summed per lane in fp32 over at most 16 pixels, then in fp64 in
 * a fixed order: per-workgroup partial sums indexed by the work item, one final ordered add -- no atomics.  A slot's sums do not
 * depend on n, on the slot nor on the run, bit for bit.  16-byte loads where a band's pixel count is a multiple of 4 and its maps
 * are 16-byte aligned; one pixel per load otherwise.  Reads 4 planes + 4 per temporal channel per band pixel, writes nothing per
 * pixel.  Launches: the sums (every band and slot), the final add.
 * Errors: FVVDP_EINVAL (null argument, bad shape, planes not 2 or 4, a missing D / contrast / S map, mask exponents or beta
 * not positive and finite, workspace too small or misaligned, d_sums not 8-byte aligned). */
int fvvdp_param_sums(int width, int height, int n_bands, int n, int planes, const fvvdp_params* prm,
                     const fvvdp_band_maps* maps, double* d_sums, void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_PARAMS_H */
