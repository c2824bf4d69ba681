/* fvvdp_hip_half.h -- the last kernels of the backward passes on float16 / bfloat16 samples.
 *
 * The forward ingest takes FVVDP_F16 and FVVDP_BF16 through the `dtype` argument it always had (fvvdp_hip.h: fvvdp_temporal_channels,
 * fvvdp_temporal_channels_frames; fvvdp_hip_images.h: fvvdp_images_channels).  The
 * backward passes read the caller's samples and write the caller's gradient in exactly one kernel each; the three functions here
 * are fvvdp_images_grad (fvvdp_hip_grad.h), fvvdp_images_ref_grad (fvvdp_hip_ref_grad.h) and fvvdp_video_grad_input
 * (fvvdp_hip_video_grad.h) with that kernel typed:
 *   dtype    FVVDP_F32, FVVDP_F16 or FVVDP_BF16: the type of the samples AND of the gradient (anything else: FVVDP_EINVAL);
 *   strides  in elements of that type, as before; pointers aligned to the element size.
 * A 16-bit sample is widened to fp32 exactly, the arithmetic is the fp32 arithmetic of the untyped function, and the result is
 * rounded ONCE to the sample type, to nearest even, float16 subnormals kept: the gradient equals the untyped function's gradient
 * for the upcast samples, converted to the sample type, bit for bit.  Everything upstream of that kernel (g0, the side buffer, the
 * maps, the sweep, the workspace, d_gamma) is fp32 whatever dtype, so an upstream scale (the loss scaling float16 training uses)
 * multiplies before the rounding.  The untyped functions forward here with FVVDP_F32.
 */
#ifndef FVVDP_HIP_HALF_H
#define FVVDP_HIP_HALF_H

#include "fvvdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fvvdp_images_grad with typed test images and gradients (h_test_ptrs / h_grad_ptrs point at [C][H][W] samples of `dtype`). */
int fvvdp_images_grad_st(int width, int height, int n_bands, int n, const fvvdp_params* prm, const fvvdp_pool_params* pool,
                         const float* d_Q, int q_stride, int q_col0, const float* d_gamma, const fvvdp_band_maps* maps,
                         const void* const* h_test_ptrs, int dtype, int C, size_t chan_stride, const fvvdp_eotf* eotf,
                         const float* h_rgb2y, void* const* h_grad_ptrs, void* d_work, size_t work_bytes, void* stream);

/* fvvdp_images_ref_grad with typed reference images and gradients. */
int fvvdp_images_ref_grad_st(int width, int height, int n_bands, int n, const fvvdp_params* prm, const fvvdp_pool_params* pool,
                             const float* d_Q, int q_stride, int q_col0, const float* d_gamma, const fvvdp_band_maps* maps,
                             const float* const* h_slope_ptrs, const void* const* h_ref_ptrs, int dtype, int C,
                             size_t chan_stride, const fvvdp_eotf* eotf, const float* h_rgb2y, void* const* h_grad_ptrs,
                             void* d_work, size_t work_bytes, void* stream);

/* fvvdp_video_grad_input with a typed clip and gradient (d_test / d_grad: samples of `dtype`, the same layout).  The vector
 * variant needs the two pointers aligned to 4 (above 16 taps: 2) samples, next to what the untyped function asks of the rest. */
int fvvdp_video_grad_input_st(int width, int height, int n_frames, const float* d_g0, const int32_t* h_fold_frame,
                              const int32_t* h_fold_pos, const float* h_taps, int fl, const void* d_test, void* d_grad, int dtype,
                              int C, size_t chan_stride, size_t frame_stride, const fvvdp_eotf* eotf, const float* h_rgb2y,
                              float* d_head, size_t head_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_HALF_H */
