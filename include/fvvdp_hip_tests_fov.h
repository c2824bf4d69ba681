/*
 * fvvdp_hip_tests_fov.h -- many test clips against one reference under a gaze in libfvvdp_hip.so (foveated video contexts,
 * stock display geometry).
 *
 * An extension beside fvvdp_hip_tests.h, whose pass covers the non-foveated metric.  Scoring T foveated variants of one
 * reference under one gaze trace with T calls of fvvdp_temporal_channels + fvvdp_bands_forward repeats, per test, everything
 * that depends on the reference and the gaze only: the reference's ingest and the write of its two level-0 planes, and inside
 * the pyramid pass its row loads, reduce and expand, L_bkg and log2(L_bkg), the eccentricity of the pixel, the position of the
 * query on the Y and eccentricity axes, the four reads of the cell of the CSF table and the 3-D interpolation of both temporal
 * channels.  The functions below run the foveated pyramid pass over the reference and a group of tests at once: per band pixel
 * that part is evaluated once, the contrast difference of a test, its four logarithms and the masking / pooling tail once per
 * test.  The result of every test does not depend on the other tests nor on their number, and is bit-identical to
 * fvvdp_bands_forward(_pool) with the same h_fixation and geom on the pair (test, reference) in a batch of the same n frames on
 * the same context.  The conventions of fvvdp_hip.h apply (d_* device and h_* host pointers, return codes, fvvdp_last_error,
 * `stream` a hipStream_t passed as void*, asynchronous).
 *
 * Streams, quads and slots are those of fvvdp_hip_tests.h: streams 0 .. T-1 are the tests, stream T is the reference; quad q
 * holds stream 2q in (x, z) and stream min(2q + 1, T) in (y, w); frame f of a batch of n frames of quad q lives in frame slot
 * q * n + f, filled by fvvdp_temporal_channels(..., n_out = n, slot0 = q * n, ...).  The context needs ceil((T + 1) / 2) * n frame
 * slots.
 *
 * Coverage.  The pass covers the contexts whose every band keeps its slice of the CSF table in the LDS and takes the
 * frame-invariant rho map, i.e. the bands that fvvdp_bands_forward walks with its lean stock-geometry kernel.  A band whose slice
 * does not fit (wide fields of view; band 0 of very tall frames) has no variant here: fvvdp_tests_fov_covered tells, and
 * fvvdp_bands_forward_tests_fov refuses such a context before its first launch.
 */
#ifndef FVVDP_HIP_TESTS_FOV_H
#define FVVDP_HIP_TESTS_FOV_H

#include "fvvdp_hip.h"
#include "fvvdp_hip_tests.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Whether the pass below covers this context under this geometry: *covered = 1 if every band's slice of the CSF table fits the
 * LDS, else 0.  Host arithmetic, except that a geometry the context has not seen yet makes it build the bands' slices and rho
 * maps, as the first fvvdp_bands_forward under that geometry does (one synchronisation of `stream`, allocations, an upload and
 * one small launch per band); with the geometry of the previous call it touches no device.
 * Errors: FVVDP_EINVAL (null pointer, a context without fvvdp_ctx_set_csf_3d, a still-image context, view maps of a user
 * geometry set). */
int fvvdp_tests_fov_covered(fvvdp_ctx* ctx, const fvvdp_geom* geom, int* covered, void* stream);

/* The foveated pyramid pass for the n frames of every quad (slots [q * n, q * n + n)) of a video context, n_tests tests.
 *   d_Q           output [n_tests][n_bands][2][q_stride] fp32; frame f of test k at column q_col0 + f of row block k
 *   h_fixation    host [n][2]: the gaze of every frame of the batch in frame pixels, as fvvdp_bands_forward takes it; uploaded
 *                 stream-ordered to the context's own buffer
 *   geom          the stock display geometry (required)
 *   d_work        workspace of at least fvvdp_tests_workspace(W, H, n_bands, n_tests, n) bytes, 256-byte aligned.  The layout is
 *                 that header's; its rows bound the one-level walk of every band, the only walk of the foveated pass
 * The work decomposition of every level is the one fvvdp_bands_forward chooses for n frames under a gaze.
 * Launches: per level one pyramid launch per group of quads -- every group reads the reference's quad and up to
 * FVVDP_TESTS_GROUP_MAX - 1 others (FVVDP_TESTS_GROUP caps it); a quad's next level is written by exactly one group (the
 * reference's by the first), a test is evaluated by exactly one group (the test that shares the reference's quad, T odd, by the
 * first) -- then one finalisation for all tests.
 * Errors, all before the first launch: FVVDP_EINVAL (null pointer, n_tests < 1, n < 1, ceil((n_tests + 1) / 2) * n beyond the
 * context's frame slots, columns out of range, a still-image context (2 planes), a context that is not foveated
 * (fvvdp_ctx_set_csf_3d not called), view maps of a user geometry set, misaligned or small workspace); FVVDP_EUNSUPPORTED (a band
 * whose slice of the CSF table does not fit the LDS, see fvvdp_tests_fov_covered). */
int fvvdp_bands_forward_tests_fov(fvvdp_ctx* ctx, int n, int n_tests, float* d_Q, int q_stride, int q_col0, const float* h_fixation,
                                  const fvvdp_geom* geom, void* d_work, size_t work_bytes, void* stream);

/* The same and, when this batch completes the clip (q_col0 + n == q_stride), fvvdp_pool_jod over the q_stride frames of every
 * test (the pooling kernel of fvvdp_bands_forward_pool, launched once per test): d_jod[k] is that kernel's value for test k's
 * block of d_Q. */
int fvvdp_bands_forward_tests_fov_pool(fvvdp_ctx* ctx, int n, int n_tests, float* d_Q, int q_stride, int q_col0,
                                       const float* h_fixation, const fvvdp_geom* geom, void* d_work, size_t work_bytes,
                                       const fvvdp_pool_params* pool, float* d_jod, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_TESTS_FOV_H */
