/*
 * fvvdp_hip_gaze.h -- one clip under many gaze traces in libfvvdp_hip.so (foveated mode, stock display geometry).
 *
 * An extension.  Scoring the same (test, reference) clip under G gaze traces with G calls of fvvdp_bands_forward repeats,
 * per gaze, everything that does not depend on the gaze: the temporal channels (fvvdp_temporal_channels) and, inside the
 * pyramid pass, the row loads, reduce, expand, the write of the next level, the contrast differences and the luminance
 * axis of the CSF query.  The functions below run the pyramid pass ONCE per group of gazes: per band pixel the gaze-invariant
 * part is evaluated once, the eccentricity, the eccentricity axis of the CSF query and the masking / pooling tail once per
 * gaze.  The result of every gaze is bit-identical to fvvdp_bands_forward(_pool) called with that gaze alone on the same
 * context and batch, whatever the other gazes are.  The conventions of fvvdp_hip.h apply (d_* device and h_* host
 * pointers, return codes, fvvdp_last_error, `stream` a hipStream_t passed as void*, asynchronous).
 *
 * A clip of N frames under G gazes, in batches of n frames:
 *     1. fvvdp_temporal_channels(...)                      once per batch, as for one gaze;
 *     2. fvvdp_bands_forward_gazes(_pool)(...)             once per batch, all gazes.
 * The per-gaze partial sums live in a workspace of the caller (fvvdp_gaze_workspace bytes): per-frame calls never allocate.
 */
#ifndef FVVDP_HIP_GAZE_H
#define FVVDP_HIP_GAZE_H

#include "fvvdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Gazes evaluated by one launch of the pyramid kernel (its largest compile-time group; more gazes take several launches over
 * the same levels, fewer a smaller instantiation). */
#define FVVDP_GAZE_GROUP_MAX 8

/* Bytes of device workspace for n_gazes gazes and a batch of n frames of width x height with n_bands band-pass levels.
 * Layout, in floats: [n_gazes] rows of R floats, R = sum over bands b of n * blk_b * 2 rounded up to 64 floats (256 B), where
 * blk_b = strips(w_{b+1}) * ceil(h_{b+1} / 2) bounds the work items of band b per frame ((w_b, h_b) the ceil(/2) level sizes,
 * strips(wc) = 1 for wc <= 62, else 1 + ceil((wc - 62) / 60)); band b of a row starts at sum_{b' < b} n * blk_b' * 2.
 * Errors: FVVDP_EINVAL (null output, non-positive sizes, n_bands outside [1, FVVDP_MAX_BANDS]). */
int fvvdp_gaze_workspace(int width, int height, int n_bands, int n_gazes, int n, size_t* bytes);

/* fvvdp_bands_forward for the frames in slots [0, n) of a foveated context under n_gazes gazes at once.
 *   d_gaze        device, gaze g of frame slot s at d_gaze[g * gaze_stride + 2 * s]: (x, y) in frame pixels, converted to
 *                 a view direction exactly as fvvdp_bands_forward converts h_fixation (gaze_stride >= 2 * n floats: a
 *                 clip-long [G][N][2] array is passed with gaze_stride = 2 N and the pointer advanced by 2 * q_col0)
 *   d_Q           output [n_gazes][n_bands][2][q_stride] fp32; frame slot s of gaze g at column q_col0 + s of row block g
 *   geom          the stock display geometry (required; contexts with fvvdp_ctx_set_view_maps maps are refused)
 *   d_work        workspace of at least fvvdp_gaze_workspace(W, H, n_bands, n_gazes, n) bytes, 256-byte aligned
 * Launches: per level one pyramid launch per group of gazes (groups of 8, 4, 2, 1; the first group of a level writes the next
 * level, the others only read), then one finalisation for all gazes.  A band whose slice of the CSF table does not fit the
 * LDS (wide fields of view such as standard_hmd: every band; band 0 of a 2160-row frame on a few displays) has no grouped
 * kernel: it takes the single-gaze kernel of fvvdp_bands_forward once per gaze -- same bits, only the temporal channels shared.
 * On a new geometry the call first rebuilds the context's foveated tables, as fvvdp_bands_forward does (one synchronisation,
 * allocations, one small launch), before its remaining checks.
 * Errors: FVVDP_EINVAL (null pointer, n_gazes < 1, n outside the context's batch, columns out of range, a context without
 * the 3-D CSF tables = not foveated, view maps set, misaligned or small workspace, gaze_stride < 2 n). */
int fvvdp_bands_forward_gazes(fvvdp_ctx* ctx, int n, int n_gazes, const float* d_gaze, size_t gaze_stride, float* d_Q,
                              int q_stride, int q_col0, const fvvdp_geom* geom, void* d_work, size_t work_bytes,
                              void* stream);

/* The same and, when this batch completes the clip (q_col0 + n == q_stride), fvvdp_pool_jod over the q_stride frames of every
 * gaze (the single-gaze pooling kernel, launched once per gaze): d_jod[g] is bit-identical to fvvdp_bands_forward_pool with
 * gaze g alone. */
int fvvdp_bands_forward_gazes_pool(fvvdp_ctx* ctx, int n, int n_gazes, const float* d_gaze, size_t gaze_stride, float* d_Q,
                                   int q_stride, int q_col0, const fvvdp_geom* geom, void* d_work, size_t work_bytes,
                                   const fvvdp_pool_params* pool, float* d_jod, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_GAZE_H */
