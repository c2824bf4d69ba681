/*
 * fvvdp_hip_images_resize.h -- still images whose two stacks have image sizes of their own in libfvvdp_hip.so: the full-screen
 * resize fused into the still-image ingest, and the level-0 step of the still-image backward that ends in luminance.
 *
 * An extension beside fvvdp_hip_resize.h, whose stream struct, modes, size limits and adjoint (fvvdp_resize_grad) it uses as they
 * are: image k of a stack is "frame" k of a fvvdp_resize_stream.  The context is a still-image context (planes == 2) whose frame
 * size is the target both stacks are judged at.  Per stack and target pixel: the samples of every channel are interpolated with
 * the arithmetic of torch.nn.functional.interpolate (align_corners=False, no antialiasing), clipped to [0, 1], sent through the
 * display model and weighted into luminance; a stack of the target's size is read as it is, and clipped like the other.  No image
 * at the target size is ever stored.  The conventions of fvvdp_hip.h apply (d_* device and h_* host pointers, return codes,
 * fvvdp_last_error, `stream` a hipStream_t passed as void*, asynchronous).
 *
 * The backward of a batch of n pairs:
 *   fvvdp_images_channels_resized, fvvdp_images_forward_pool with every band's maps (and the slope planes, for the reference);
 *   per differentiated side: fvvdp_images_grad_luminance (maps -> d_gL [n][H][W]) and fvvdp_resize_grad with n_frames = n (d_gL
 *   and that side's stack -> the gradient of every sample of the stack, at the stack's own size).
 * Every output is a fixed sum per sample (no atomics): the result does not depend on the launch geometry and repeats bit for bit.
 */
#ifndef FVVDP_HIP_IMAGES_RESIZE_H
#define FVVDP_HIP_IMAGES_RESIZE_H

#include "fvvdp_hip.h"
#include "fvvdp_hip_resize.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fvvdp_images_channels for two stacks of their own image sizes: level 0 of slots [slot0, slot0 + n) of a still-image context,
 * whose frame size is the target.
 *   test, ref                    the two stacks: the same channel count, each its own width x height; image k lies at
 *                                k * frame_stride, its channel c at c * plane_stride (no pointer table: n has no 128-pair split);
 *   mode                         FVVDP_RESIZE_*: how a stack whose size differs from the target is resized;
 *   eotf, h_rgb2y                as fvvdp_images_channels; the display model must have a closed form.
 * One lane owns target pixels of one pair: each stack's tap indices and weights, the interpolation in torch's order of operations,
 * the clip, the display model, the luminance weights and one store of {L_test, L_ref}.  The out-of-range flag of
 * fvvdp_images_channels does not exist here: the clip belongs to the resize.
 * Errors: FVVDP_EINVAL (null or misaligned pointer, sample type, channel counts, a stack or target size outside
 * 1 .. FVVDP_RESIZE_MAX_AXIS per axis, strides below the image, slots, unknown mode, a display model without a closed form, a
 * video context). */
int fvvdp_images_channels_resized(fvvdp_ctx* ctx, const fvvdp_resize_stream* test, const fvvdp_resize_stream* ref, int n, int mode,
                                  const fvvdp_eotf* eotf, const float* h_rgb2y, int slot0, void* stream);

/* Bytes of the workspace of the function below for n pairs of width x height (the target): fvvdp_images_grad_workspace's when
 * `reference` is 0, fvvdp_ref_grad_workspace's (planes == 1) otherwise. */
int fvvdp_images_grad_luminance_workspace(int width, int height, int n_bands, int n, int reference, size_t* bytes);

/* fvvdp_images_grad (h_slope_ptrs NULL) or fvvdp_images_ref_grad (h_slope_ptrs: one device pointer per band, the slope planes of
 * fvvdp_ctx_set_slope_maps) without the display model: their launches up to, not including, the last, then one kernel that writes
 *   d_gL[k][y][x] = d_gamma[k] * dJOD_k/dL_k[y][x] = GL_0 + Reduce^T(GG_1),
 * the gradient of the luminance of every target pixel of the differentiated side, dense [n][height][width] -- what
 * fvvdp_resize_grad takes with n_frames = n.  Every other argument as fvvdp_images_grad.  d_work: 256-byte aligned.
 * Errors: FVVDP_EINVAL (null or misaligned pointer, bad shape, Q columns, pooling exponents, a missing map or slope plane, a
 * workspace below need). */
int fvvdp_images_grad_luminance(int width, int height, int n_bands, int n, const fvvdp_params* prm, const fvvdp_pool_params* pool,
                                const float* d_Q, int q_stride, int q_col0, const float* d_gamma, const fvvdp_band_maps* maps,
                                const float* const* h_slope_ptrs, float* d_gL, void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_IMAGES_RESIZE_H */
