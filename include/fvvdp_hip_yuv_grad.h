/*
 * fvvdp_hip_yuv_grad.h -- planar YUV clips of float32 samples in libfvvdp_hip.so: their ingest, and dJOD / d(Y, U, V).
 *
 * An extension beside fvvdp_hip_video_grad.h.  The forward is fvvdp_temporal_channels_yuv (fvvdp_hip.h) for planes of float32
 * CODE VALUES: a sample stands where that function computes (float)code, on the scale of bit_depth (luma nominally in
 * [16, 235] * 2^(bit_depth - 8)), fractions allowed.  Each stream is three plane pointers and two frame strides, so a packed
 * clip (Y plane, U plane, V plane per frame) and three separate tensors are the same call.  The conventions of fvvdp_hip.h apply
 * (d_* device and h_* host pointers, return codes, fvvdp_last_error, `stream` a hipStream_t passed as void*, asynchronous).
 *
 * The backward of a clip of N frames:
 *   per batch, as fvvdp_hip_video_grad.h: fvvdp_temporal_channels_yuv_planes, fvvdp_bands_forward with every band's maps,
 *   fvvdp_video_grad_frames into the clip-long d_g0 [N][2][H][W];
 *   then once: fvvdp_video_grad_luminance (d_g0 -> the gradient of every frame's luminance, d_gL [N][H][W]) and
 *   fvvdp_yuv_grad_planes (d_gL and the test planes -> dY, dU, dV: the adjoint of the unpack).
 * Every output is a fixed sum per sample (no atomics): the result does not depend on the launch geometry and repeats bit for bit.
 */
#ifndef FVVDP_HIP_YUV_GRAD_H
#define FVVDP_HIP_YUV_GRAD_H

#include "fvvdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Longest temporal filter fvvdp_temporal_channels_yuv_planes covers (its register ring has 8 / 16 / 32 slots): 32 taps, 120 frames
 * per second have 30.  Longer filters are REFUSED with FVVDP_EUNSUPPORTED and a sentence. */
#define FVVDP_YUV_GRAD_MAX_TAPS 32

/* One stream of planar YUV, float32 code values.  Plane rows are contiguous; frame f of the luma plane starts at
 * d_y + f * luma_stride, of each chroma plane at d_u / d_v + f * chroma_stride (strides in elements).  The luma plane is
 * height x width, the chroma planes height/2 x width/2 (4:2:0) or height x width (4:4:4). */
typedef struct fvvdp_yuv_planes {
    const float* d_y;
    const float* d_u;
    const float* d_v;
    size_t luma_stride;
    size_t chroma_stride;
} fvvdp_yuv_planes;

/* fvvdp_temporal_channels_yuv for float32 planes: level 0 of slots [slot0, slot0 + n_out) of a video context.
 *   test, ref                    the two streams (frame indices of h_frame_idx address both);
 *   fmt                          bit depth (the scale of the code values), chroma format and the YCbCr -> RGB matrix;
 *   every other argument         as fvvdp_temporal_channels_yuv; 1 <= fl <= FVVDP_YUV_GRAD_MAX_TAPS.
 * Per pixel: Yf = clamp(wy y - 16/219, 0, 1), chroma clamp(wc c - 128/224, -0.5, 0.5), 4:2:0 chroma bilinear x2 (torch's
 * interpolate, align_corners=False), the matrix, clip to [0, 1], display model, luminance, then the temporal filters.
 * When width % 4 == 0 and the planes and strides keep 16-byte (chroma of 4:2:0: 8-byte) alignment and fl <= 16, a lane owns four
 * consecutive pixels of a row (one 16-byte luma load per frame and stream, one 8-byte load per chroma plane and source row plus
 * the two neighbour columns); a per-pixel kernel otherwise.
 * Errors: FVVDP_EINVAL (null or misaligned pointer, bit depth, odd 4:2:0 size, slots, strides below the plane size, a display model
 * without a closed form, a still-image context), FVVDP_EUNSUPPORTED (fl above FVVDP_YUV_GRAD_MAX_TAPS). */
int fvvdp_temporal_channels_yuv_planes(fvvdp_ctx* ctx, const fvvdp_yuv_planes* test, const fvvdp_yuv_planes* ref,
                                       const fvvdp_yuv_format* fmt, const fvvdp_eotf* eotf, const float* h_rgb2y,
                                       const int32_t* h_frame_idx, const float* h_taps, int fl, int n_out, int slot0,
                                       int32_t* d_oob_flag, void* stream);

/* d_gL[j][y][x] = sum over the window-list positions p that show frame j of
 *                 A[p] = sum_cc sum_k taps[cc][k] g0[p - (fl - 1) + k][cc]:
 * fvvdp_video_grad_input (fvvdp_hip_video_grad.h) without the display model's derivative -- the gradient with respect to each
 * frame's luminance.  The fold list, taps and side buffer are that function's, with the same checks; fl up to
 * FVVDP_VIDEO_GRAD_MAX_TAPS.  8 bytes read and 4 written per pixel and frame.
 * Errors: FVVDP_EINVAL (null or misaligned pointer, bad shape, fold list, small side buffer), FVVDP_EUNSUPPORTED (fl). */
int fvvdp_video_grad_luminance(int width, int height, int n_frames, const float* d_g0, const int32_t* h_fold_frame,
                               const int32_t* h_fold_pos, const float* h_taps, int fl, float* d_gL, float* d_head,
                               size_t head_bytes, void* stream);

/* The adjoint of the unpack: d_gL [n_frames][height][width] (dense) and the planes of the clip -> the gradient of every plane
 * sample, in planes laid out as `grad` says (its pointers are written; the same struct with the const cast away).
 *   per luma pixel     Yf, the upsampled clamped chroma and the three RGB values before their clip are recomputed;
 *                      d_c = gL w_c EOTF'(rgb_c) (zero where rgb_c is clipped), dYf = sum_c m[3c] d_c, du = sum_c m[3c+1] d_c,
 *                      dv = sum_c m[3c+2] d_c; dY = wy dYf where the luma clamp does not bind;
 *   per chroma sample  4:2:0: the transpose of the bilinear x2 upsampling -- a gather over luma rows 2i-1 .. 2i+2 and columns
 *                      2j-1 .. 2j+2 with the weights {1/4, 3/4, 3/4, 1/4} per axis, rows and columns outside the frame folded
 *                      onto the border sample; 4:4:4: pointwise; times wc where the chroma clamp does not bind.
 * A workgroup owns a tile of 64 x 32 luma pixels and its one-pixel halo, leaves du, dv of all of them in LDS and sums each chroma
 * sample's 16 terms in a fixed order: no atomics, every plane sample written exactly once.
 * Errors: FVVDP_EINVAL (null or misaligned pointer, bad shape, bit depth, odd 4:2:0 size, strides, display model). */
int fvvdp_yuv_grad_planes(int width, int height, int n_frames, const float* d_gL, const fvvdp_yuv_planes* test,
                          const fvvdp_yuv_planes* grad, const fvvdp_yuv_format* fmt, const fvvdp_eotf* eotf,
                          const float* h_rgb2y, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_YUV_GRAD_H */
