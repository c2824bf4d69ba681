/*
 * fvvdp_hip_tests.h -- many test clips against one reference in libfvvdp_hip.so (video contexts, not foveated).
 *
 * An extension.  Scoring T test clips against one reference with T calls of fvvdp_temporal_channels + fvvdp_bands_forward
 * repeats, per test, everything that depends on the reference only: its ingest, the write of its two level-0 planes, and
 * inside the pyramid pass its row loads, reduce and expand, L_bkg, log2(L_bkg) and the look-up of the CSF table.  The
 * functions below run the pyramid pass over the reference and a group of tests at once: per band pixel the reference-only part
 * is evaluated once, the contrast difference of a test and the masking / pooling tail once per test.  The result of every test
 * does not depend on the other tests nor on their number, and is bit-identical to fvvdp_bands_forward(_pool) on the pair
 * (test, reference) in a batch of the same n frames on the same context.  That includes the levels which that call walks two
 * at a time: the pass below takes them one by one, but cuts them into the two-level kernel's strips and chunks and adds the lanes
 * in its order, so the partial sums behind Q are the same.  The conventions of fvvdp_hip.h apply (d_* device and h_*
 * host pointers, return codes, fvvdp_last_error, `stream` a hipStream_t passed as void*, asynchronous).
 *
 * Streams, quads and slots.  A level plane of a video context is a float4 per pixel: components (x, z) are the sustained and
 * the transient channel of the stream fvvdp_temporal_channels got as `d_test`, (y, w) those of the stream it got as `d_ref`.
 * Number the streams 0 .. T: streams 0 .. T-1 are the tests, stream T is the reference.  Quad q, q = 0 .. NQ-1 with
 * NQ = ceil((T + 1) / 2), holds stream 2q in (x, z) and stream 2q+1 in (y, w); when T is even the last quad holds the reference
 * in both ((x, z) = (y, w) = stream T).  Frame f of a batch of n frames of quad q lives in frame slot q * n + f:
 *     for q in 0 .. NQ-1:  fvvdp_temporal_channels(ctx, d_test = stream 2q, d_ref = stream min(2q + 1, T), ..., n_out = n, slot0 = q * n, ...)
 * The context needs NQ * n frame slots (max_frames of fvvdp_ctx_create).
 *
 * A clip of N frames, T tests, in batches of n frames:
 *     1. fvvdp_temporal_channels(...)                      NQ times per batch, as above;
 *     2. fvvdp_bands_forward_tests(_pool)(...)             once per batch, all tests.
 * The per-test partial sums live in a workspace of the caller (fvvdp_tests_workspace bytes): per-frame calls never allocate
 * and never synchronise.
 */
#ifndef FVVDP_HIP_TESTS_H
#define FVVDP_HIP_TESTS_H

#include "fvvdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Quads read by one launch of the pyramid kernel (its largest compile-time group): the reference's quad and up to
 * FVVDP_TESTS_GROUP_MAX - 1 others, i.e. up to 2 * (FVVDP_TESTS_GROUP_MAX - 1) + 1 tests per launch. */
#define FVVDP_TESTS_GROUP_MAX 3

/* Bytes of device workspace for n_tests tests and a batch of n frames of width x height with n_bands band-pass levels.
 * Layout, in floats: [n_tests] rows of R floats, R = sum over bands b of n * blk_b * 2 rounded up to 64 floats (256 B), where
 * blk_b bounds the work items of band b per frame under either walk: the largest of one_b = strips(w_{b+1}) * ceil(h_{b+1} / 2)
 * (one level per launch; (w_b, h_b) the ceil(/2) level sizes, strips(wc) = 1 for wc <= 62, else 1 + ceil((wc - 62) / 60)) and,
 * for a = b - 1 and a = b with 0 <= a < n_bands - 1, two_a = ceil(w_{a+1} / 54) * h_{a+2} (levels a, a + 1 in the two-level
 * kernel's strips and chunks); band b of a row starts at sum_{b' < b} n * blk_b' * 2.
 * Touches no device.  Errors: FVVDP_EINVAL (null output, non-positive sizes, n_bands outside [1, FVVDP_MAX_BANDS]). */
int fvvdp_tests_workspace(int width, int height, int n_bands, int n_tests, int n, size_t* bytes);

/* The pyramid pass for the n frames of every quad (slots [q * n, q * n + n), see above) of a video context, n_tests tests.
 *   d_Q           output [n_tests][n_bands][2][q_stride] fp32; frame f of test k at column q_col0 + f of row block k
 *   d_work        workspace of at least fvvdp_tests_workspace(W, H, n_bands, n_tests, n) bytes, 256-byte aligned
 * The work decomposition of every level is the one fvvdp_bands_forward chooses for n frames, also where that is its two-level
 * kernel's (FVVDP_BAND_FUSE is honoured alike).
 * Launches: per level one pyramid launch per group of quads -- every group reads the reference's quad and up to
 * FVVDP_TESTS_GROUP_MAX - 1 others; a quad's next level is written by exactly one group (the reference's by the first), a test
 * is evaluated by exactly one group (the test that shares the reference's quad, T odd, by the first) -- then one finalisation
 * for all tests.
 * Errors: FVVDP_EINVAL (null pointer, n_tests < 1, n < 1, ceil((n_tests + 1) / 2) * n beyond the context's frame slots, columns
 * out of range, a still-image context (2 planes), a foveated context (fvvdp_ctx_set_csf_3d called), misaligned or small
 * workspace); FVVDP_ESTATE (fvvdp_ctx_set_csf_1d not called). */
int fvvdp_bands_forward_tests(fvvdp_ctx* ctx, int n, int n_tests, float* d_Q, int q_stride, int q_col0, void* d_work,
                              size_t work_bytes, void* stream);

/* The same and, when this batch completes the clip (q_col0 + n == q_stride), fvvdp_pool_jod over the q_stride frames of every
 * test (the pooling kernel of fvvdp_bands_forward_pool, launched once per test): d_jod[k] is that kernel's value for test k's
 * block of d_Q. */
int fvvdp_bands_forward_tests_pool(fvvdp_ctx* ctx, int n, int n_tests, float* d_Q, int q_stride, int q_col0, void* d_work,
                                   size_t work_bytes, const fvvdp_pool_params* pool, float* d_jod, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_TESTS_H */
