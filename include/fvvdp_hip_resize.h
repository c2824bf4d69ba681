/*
 * fvvdp_hip_resize.h -- clips whose two streams have frame sizes of their own in libfvvdp_hip.so: the full-screen resize fused
 * into the ingest, and its adjoint.
 *
 * An extension beside fvvdp_hip_yuv_grad.h.  Each stream is a clip of C planes per frame (C = 1 or 3; float32 samples, or uint8
 * codes scaled by 1/255) at its OWN width x height; the context's frame size is the target both are judged at.  A stream whose
 * size differs from the target is resized with the arithmetic of torch.nn.functional.interpolate (align_corners=False, no
 * antialiasing; FVVDP_RESIZE_NEAREST / BILINEAR / BICUBIC / AREA of fvvdp_hip.h), a stream of the target's size is read as it is.
 * Per stream and target pixel: the samples of every channel are interpolated, clipped to [0, 1], sent through the display model
 * and weighted into luminance -- what the reference's file reader does under --full-screen-resize.  No clip at the target size is
 * ever stored.  Widths and heights, of either stream and of the target, lie in 1 .. FVVDP_RESIZE_MAX_AXIS: the index arithmetic
 * runs in 32 bits (the `area` windows are ATen's integer start and end indices, whose products of an index and a size must stay
 * below 2^31); anything larger is refused with FVVDP_EINVAL.  The conventions of fvvdp_hip.h apply (d_* device and h_* host
 * pointers, return codes, fvvdp_last_error, `stream` a hipStream_t passed as void*, asynchronous).
 *
 * The backward of a clip of N frames:
 *   per batch, as fvvdp_hip_video_grad.h: fvvdp_temporal_channels_resized, fvvdp_bands_forward with every band's maps,
 *   fvvdp_video_grad_frames into the clip-long d_g0 [N][2][Ho][Wo];
 *   then once: fvvdp_video_grad_luminance (fvvdp_hip_yuv_grad.h; d_g0 -> d_gL [N][Ho][Wo]) and fvvdp_resize_grad (d_gL and the test
 *   clip -> the gradient of every sample of the test clip, at the clip's own size).
 * Every output is a fixed sum per sample (no atomics): the result does not depend on the launch geometry and repeats bit for bit.
 */
#ifndef FVVDP_HIP_RESIZE_H
#define FVVDP_HIP_RESIZE_H

#include "fvvdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Longest temporal filter fvvdp_temporal_channels_resized covers (its register ring has 8 / 16 / 32 slots): 32 taps, 120 frames
 * per second have 30.  Longer filters are REFUSED with FVVDP_EUNSUPPORTED and a sentence. */
#define FVVDP_RESIZE_MAX_TAPS 32

/* Largest width or height of a stream or of the target, as for fvvdp_yuv_frame_resized. */
#define FVVDP_RESIZE_MAX_AXIS 32768

/* One stream.  Sample (c, y, x) of frame f is element d_data[f * frame_stride + c * plane_stride + y * width + x] (strides in
 * elements; rows contiguous).  dtype: FVVDP_F32, or FVVDP_U8 (the value is code * (1/255)). */
typedef struct fvvdp_resize_stream {
    const void* d_data;
    int32_t dtype;
    int32_t channels;
    int32_t width, height;
    size_t frame_stride;
    size_t plane_stride;
} fvvdp_resize_stream;

/* fvvdp_temporal_channels for two streams of their own frame sizes: level 0 of slots [slot0, slot0 + n_out) of a video context,
 * whose frame size is the target.
 *   test, ref                    the two streams: the same channel count, each its own width x height;
 *   mode                         FVVDP_RESIZE_*: how a stream whose size differs from the target is resized;
 *   every other argument         as fvvdp_temporal_channels; 1 <= fl <= FVVDP_RESIZE_MAX_TAPS.
 * A lane owns target pixels for the whole launch: each stream's tap indices and weights are computed once, every frame is a
 * gather, the interpolation in torch's order of operations, the clip, the display model, the luminance weights and a push into
 * the register ring of the temporal filters.  The out-of-range flag of the context's other ingests does not exist here: the
 * clip belongs to the resize.
 * Errors: FVVDP_EINVAL (null or misaligned pointer, sample type, channel counts, a stream or target size outside
 * 1 .. FVVDP_RESIZE_MAX_AXIS per axis, strides below the frame, slots, unknown mode, a display model without a closed form, a
 * still-image context), FVVDP_EUNSUPPORTED (fl). */
int fvvdp_temporal_channels_resized(fvvdp_ctx* ctx, const fvvdp_resize_stream* test, const fvvdp_resize_stream* ref, int mode,
                                    const fvvdp_eotf* eotf, const float* h_rgb2y, const int32_t* h_frame_idx, const float* h_taps,
                                    int fl, int n_out, int slot0, void* stream);

/* Bytes at the head of the workspace of the function below that hold its int32 tables for a test of width x height: two
 * entries per source row and column, rounded up to 256 bytes.  Behind them the first stage keeps channels * out_height *
 * out_width floats per frame, for as many frames at once as the workspace holds (at least one). */
#define FVVDP_RESIZE_GRAD_TABLE_BYTES(width, height) ((((size_t)2 * ((size_t)(width) + (size_t)(height)) * 4) + 255) / 256 * 256)

/* The adjoint of the resize: d_gL [n_frames][out_height][out_width] (dense, the gradient of every target pixel's luminance) and
 * the float32 test clip -> d_grad, the gradient of every sample of `test`, laid out as `test` is (its strides; written exactly
 * once per sample, zeros included).
 *   stage 1, per target pixel   v_c is recomputed with the forward's own function; d_c = gL w_c EOTF'(v_c) where v_c lies in
 *                               [0, 1], 0 where the clip binds; into the workspace, [channels][out_height][out_width] per frame;
 *   stage 2, per source sample  a gather: sum over target rows oy (ascending) of wy(oy -> y) * (sum over target columns ox
 *                               (ascending) of wx(ox -> x) * d_c[oy][ox]).  The host runs the index arithmetic over the out_height
 *                               + out_width target rows and columns once and uploads, per source row and column, the range of
 *                               targets that can reach it; inside the range the device decides membership and weight with the
 *                               forward's own index function (taps that the index clamp folds onto one border sample add up).
 * A test of the target's size is the pointwise case of the same two stages.  d_work: 256-byte aligned.
 * Errors: FVVDP_EINVAL (null or misaligned pointer, bad shape, a size outside 1 .. FVVDP_RESIZE_MAX_AXIS per axis, a test that is
 * not float32, strides, unknown mode, display model, a workspace below one frame). */
int fvvdp_resize_grad(int out_width, int out_height, int n_frames, const float* d_gL, const fvvdp_resize_stream* test,
                      float* d_grad, int mode, const fvvdp_eotf* eotf, const float* h_rgb2y, void* d_work, size_t work_bytes,
                      void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_RESIZE_H */
