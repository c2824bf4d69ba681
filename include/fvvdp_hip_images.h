/*
 * fvvdp_hip_images.h -- batched still-image evaluation in libfvvdp_hip.so: many (test, reference) image pairs scored in one
 * pass on a still-image context (fvvdp_ctx_create with planes == 2, max_frames >= the pairs of one batch).
 *
 * An extension: the reference evaluates one image pair per call (pyfvvdp/fvvdp.py:248-253).  A batch of n pairs costs one
 * ingest launch, one launch per pyramid level (or level pair), one finalisation and one pooling launch, and no host
 * synchronisation.  Every pair's result is independent of the batch: of its size, of the pair's slot and of the other
 * pairs.  The conventions of fvvdp_hip.h apply (d_* device and h_* host pointers, return codes, fvvdp_last_error,
 * `stream` a hipStream_t passed as void*, asynchronous unless stated).
 *
 * A batch:  fvvdp_images_channels (level 0 of slots [0, n))  ->  fvvdp_images_forward_pool (Q_per_ch columns and one JOD
 * per pair).  Heat maps: fvvdp_heatmap_reconstruct / fvvdp_heatmap_colorize of fvvdp_hip.h with the same n, after a
 * fvvdp_images_forward_pool call that asked for difference maps.
 */
#ifndef FVVDP_HIP_IMAGES_H
#define FVVDP_HIP_IMAGES_H

#include "fvvdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pairs the pointer table of one ingest launch holds (kernel arguments, 2 KB); larger n is split into several launches. */
#define FVVDP_IMAGES_MAX_PAIRS_PER_LAUNCH 128
/* Slot count the work decomposition of fvvdp_images_forward_pool is planned for, whatever its n (batch invariance). */
#define FVVDP_IMAGES_PLAN_N 128

/* Unpack + display photometry + luminance of n separate image pairs into pyramid level 0 of slots [slot0, slot0 + n) of a
 * still-image context: what fvvdp_temporal_channels does for one image (fl == 1), with the same arithmetic, so each slot's
 * level 0 is bit-identical to that call on the same pair.
 *   h_test_ptrs, h_ref_ptrs  host arrays of n DEVICE pointers; pair k is the image [C][H][W] at h_test_ptrs[k] /
 *                            h_ref_ptrs[k] (channel c at c * chan_stride elements, chan_stride >= H*W for C == 3).  The images
 *                            are separate allocations; no staging copy is made.  Pointers must be aligned to the element size
 *                            (16-byte alignment, H*W and chan_stride multiples of 4 select the four-pixels-per-lane loads).
 *   dtype, C, eotf, h_rgb2y  as fvvdp_temporal_channels: FVVDP_U8 needs FVVDP_EOTF_LUT; FVVDP_U16 a table or a closed form;
 *                            FVVDP_F32 a closed form.  FVVDP_EOTF_NONE is refused.
 *   d_oob_flags              NULL or int32[n]: flag k is OR-ed with 1 when a sample of pair k lies outside [0, 1] for a display
 *                            model that clamps (the caller zeroes the flags; the reference's warning, video_source.py:200).
 * The pointer table travels in the kernel arguments (no upload, no synchronisation).  Errors: FVVDP_EINVAL (null or misaligned
 * pointer, planes != 2, slots beyond max_frames, unsupported type / channel count / display model). */
int fvvdp_images_channels(fvvdp_ctx* ctx, const void* const* h_test_ptrs, const void* const* h_ref_ptrs, int n, int dtype,
                          int C, size_t chan_stride, const fvvdp_eotf* eotf, const float* h_rgb2y, int slot0,
                          int32_t* d_oob_flags, void* stream);

/* fvvdp_bands_forward on slots [0, n) of a still-image context, then one JOD per pair: Q_per_ch columns q_col0 + k (layout
 * [band][2][q_stride], cc = 1 written as 0) and d_jod[k] for k in [0, n).  The chunking of the pyramid pass is chosen from the
 * level sizes alone (planned for FVVDP_IMAGES_PLAN_N slots), so pair k's Q and JOD are bit-identical whatever the batch around
 * it; they agree with a single-image fvvdp_bands_forward_pool call to fp32 rounding (that call plans for n == 1).
 * d_jod[k] is bit-identical to fvvdp_pool_jod on column q_col0 + k alone.
 *   h_fixation, geom, maps   as fvvdp_bands_forward ([n][2] gaze per pair; difference maps of the n slots).
 *   pool                     pooling parameters (fvvdp_pool_params), required.
 * Asynchronous; the fixation table is staged like fvvdp_bands_forward's.  Errors: FVVDP_EINVAL, FVVDP_ESTATE (CSF tables
 * not set). */
int fvvdp_images_forward_pool(fvvdp_ctx* ctx, int n, float* d_Q, int q_stride, int q_col0, const float* h_fixation,
                              const fvvdp_geom* geom, const fvvdp_band_maps* maps, const fvvdp_pool_params* pool,
                              float* d_jod, void* stream);

/* One JOD per column: d_jod[j] = do_pooling_and_jods (fvvdp.py:337-357) of column j of d_Q[band][2][q_stride] as a clip of
 * one frame, bit-identical to fvvdp_pool_jod(d_Q + j, n_bands, n_channels, 1, q_stride, ...).  Columns [0, n_cols);
 * offset d_Q for a later first column.  One launch, asynchronous.  Errors: FVVDP_EINVAL (shape, non-positive exponents). */
int fvvdp_pool_jod_columns(const float* d_Q, int n_bands, int n_channels, int n_cols, int q_stride,
                           const fvvdp_pool_params* prm, float* d_jod, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_IMAGES_H */
