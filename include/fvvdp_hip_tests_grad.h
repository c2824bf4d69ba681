/*
 * fvvdp_hip_tests_grad.h -- gradients of the video JOD of many tests with respect to their ONE reference in libfvvdp_hip.so:
 * sum_k gamma[k] * dJOD_k / dreference for T float test clips scored against one reference clip.
 *
 * An extension, where fvvdp_hip_tests.h (many tests, one reference, forward) and fvvdp_hip_ref_grad.h (one test, backward with
 * respect to the reference) meet.  After the pointwise layer gradient the reference's backward is linear in it, so the
 * functions below sum the layer gradients (GLR and GX of every band, ref_grad_kernels.hpp) of all tests first and run the
 * coarse-to-fine sweep and level 0 once; fvvdp_video_grad_input after them is the caller's, once per clip, whatever the number
 * of tests.  Of the 11 planes the single-test layer kernel reads per band pixel, 7 depend on the reference only (L_bkg, the two
 * S planes, the two slope planes, the reference's two contrast planes): a launch reads them once per group of up to 4 tests.
 * The conventions of fvvdp_hip.h apply (d_* device and h_* host pointers, return codes, fvvdp_last_error, `stream` a
 * hipStream_t passed as void*, asynchronous).  No context is needed: the functions read only what they are given, allocate
 * nothing and never synchronise.
 *
 * The backward of a clip of N frames whose forward (fvvdp_bands_forward_tests_pool) left Q_per_ch [T][n_bands][2][N]:
 *   for every batch of n output frames [f0, f0 + n) (slots [0, n) of a video context):
 *     for every test k, ascending:
 *       1. fvvdp_temporal_channels of (test k, reference) with the batch's slice of the window index list;
 *       2. fvvdp_bands_forward with every band's maps set and the slope planes switched on (fvvdp_ctx_set_slope_maps).  The
 *          maps that depend on the reference only (d_lbkg, d_S, the slope planes) may be the same buffers for every test;
 *     3. fvvdp_tests_ref_grad_layer, once for all tests or once per run of consecutive tests whose maps are resident
 *        (add = 0 on the batch's first call, 1 on the later ones);
 *     4. fvvdp_tests_ref_grad_finish: columns [f0, f0 + n) of the clip-long buffer d_g0 [N][2][H][W];
 *   then once: fvvdp_video_grad_input (fvvdp_hip_video_grad.h) on the reference clip.
 * Every output is a fixed sum per pixel, the tests in ascending order (no atomics): the result does not depend on the batching,
 * on how the tests are cut into calls nor on how a call groups them into launches, and repeats bit for bit.  With one test it
 * is fvvdp_video_ref_grad_frames' (fvvdp_hip_ref_grad.h), bit for bit.
 */
#ifndef FVVDP_HIP_TESTS_GRAD_H
#define FVVDP_HIP_TESTS_GRAD_H

#include "fvvdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FVVDP_TESTS_GRAD_GROUP_MAX 4 /* tests one layer launch takes */

/* Bytes of device workspace for a batch of n frames of width x height with n_bands band-pass levels and n_tests tests: the
 * workspace of fvvdp_ref_grad_workspace(planes = 2) (one set of GLR, GG and GX maps, whatever n_tests) followed by the
 * coefficients of every test, [n_tests] blocks of [n][2][n_bands] floats, each rounded up to 64 floats.
 * Errors: FVVDP_EINVAL (null output, non-positive sizes, n_bands outside [1, FVVDP_MAX_BANDS], n_tests < 1). */
int fvvdp_tests_ref_grad_workspace(int width, int height, int n_bands, int n, int n_tests, size_t* bytes);

/* The layer gradients of every band for frames [f0, f0 + n), summed over the n_group tests [test0, test0 + n_group):
 * GLR and GX in the workspace (+)= sum_k gamma[k] * (the maps ref_layer_kernel<2> writes for test k).
 *   width, height, n_bands, prm  geometry and model constants of the context the maps came from;
 *   n_tests                      T: the tests of the clip (rows of d_Q, entries of d_gamma, coefficient blocks of the workspace);
 *   test0, n_group               the tests of this call, 0 <= test0, n_group >= 1, test0 + n_group <= n_tests;
 *   group_max                    largest group of tests one layer launch takes: 0 (the default, 4), 1, 2 or 4; the result does
 *                                not depend on it, bit for bit (smaller groups: more launches; tests and A/B runs);
 *   add                          0: the call's first launch stores (the first call of a batch); 1: it adds to what the calls
 *                                before it left in the workspace;
 *   pool                         the pooling parameters of the forward;
 *   d_Q, n_frames                Q_per_ch of the FORWARD pass of the whole clip for every test, [n_tests][n_bands][2][n_frames];
 *   d_gamma                      float[n_tests], the upstream gradient of every test's JOD (device; a test with gamma 0 adds
 *                                exact zeros);
 *   maps                         n_group x n_bands records, test test0 + j in maps[j * n_bands .. ], every pointer set, holding
 *                                the n frames of step 2 above.  d_D [n][2] and d_contrast [n][4] are read from every record,
 *                                d_lbkg [n], d_S [n][2] and the reference's planes of d_contrast from the first record of a
 *                                launch's group;
 *   h_slope_ptrs                 host array of n_bands device pointers, the slope planes [n][2][h_b][w_b] of step 2;
 *   d_work, work_bytes           workspace of at least fvvdp_tests_ref_grad_workspace(..., n_tests) bytes, 256-byte aligned;
 *                                the same for every call of a batch and for fvvdp_tests_ref_grad_finish.
 * Launches: the coefficients once per test of the call, then the layer gradients of all bands once per group of tests (groups
 * of 4, 2, 1; the tests of a group are added in ascending order).
 * Errors: FVVDP_EINVAL (null pointer, bad shape, n_tests < 1, tests outside [0, n_tests), a group_max other than 0, 1, 2, 4,
 * frames outside the clip, maps or slope planes missing, misaligned or small workspace). */
int fvvdp_tests_ref_grad_layer(int width, int height, int n_bands, int n, int n_tests, int test0, int n_group, int group_max,
                               int add, const fvvdp_params* prm, const fvvdp_pool_params* pool, const float* d_Q, int n_frames,
                               int f0, const float* d_gamma, const fvvdp_band_maps* maps, const float* const* h_slope_ptrs,
                               void* d_work, size_t work_bytes, void* stream);

/* After the batch's last fvvdp_tests_ref_grad_layer: the coarse-to-fine sweep on the 2n planes and level 0, once:
 * d_g0[f0 + k][cc][y][x] = sum_k gamma[k] * dJOD_k / d(level 0, reference plane of temporal channel cc, frame f0 + k).
 *   d_g0                         the clip-long output [n_frames][2][height][width] fp32;
 *   the other arguments          as the layer calls of the batch.
 * Errors: FVVDP_EINVAL (null pointer, bad shape, n_tests < 1, frames outside the clip, misaligned or small workspace). */
int fvvdp_tests_ref_grad_finish(int width, int height, int n_bands, int n, int n_tests, int n_frames, int f0, float* d_g0,
                                void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_TESTS_GRAD_H */
