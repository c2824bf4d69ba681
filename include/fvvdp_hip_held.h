/*
 * fvvdp_hip_held.h -- clips whose two streams have frame COUNTS of their own in libfvvdp_hip.so: held frames in the ingest, and
 * the transpose of the hold in the last kernel of the backward.
 *
 * An extension beside fvvdp_hip_resize.h.  The pair is judged at the display's rate, N display frames.  Each stream is a clip of
 * n_frames <= N source frames of its own and is shown by sample-and-hold through a frame map m: display frame v shows source
 * frame m[v] (non-decreasing; a frame that repeats is held, a frame that is skipped is never shown).  Taps, temporal padding and
 * gaze refer to display frames; the window index list a stream's ingest reads is the display-rate list sent through its map.  The
 * result is, bit for bit, what fvvdp_temporal_channels gives on the two clips expanded to N frames each -- which never exist.
 * The conventions of fvvdp_hip.h apply (d_* device and h_* host pointers, return codes, fvvdp_last_error, `stream` a hipStream_t
 * passed as void*, asynchronous).
 *
 * The backward of a clip pair of N display frames:
 *   per batch, as fvvdp_hip_video_grad.h: fvvdp_temporal_channels_held, fvvdp_bands_forward with every band's maps,
 *   fvvdp_video_grad_frames (fvvdp_video_ref_grad_frames) into the clip-long d_g0 [N][2][H][W];
 *   then once per differentiated stream: fvvdp_video_grad_input_held (d_g0, the stream's clip and map -> the gradient of every
 *   sample of the stream's n_frames source frames).
 * Every output is a fixed sum per sample (no atomics): the result does not depend on the launch geometry and repeats bit for bit.
 */
#ifndef FVVDP_HIP_HELD_H
#define FVVDP_HIP_HELD_H

#include "fvvdp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Longest temporal filter the two functions cover (register rings of 8 / 16 / 32 slots): 32 taps, display rates of up to 128
 * frames per second.  Longer filters are REFUSED with FVVDP_EUNSUPPORTED and a sentence. */
#define FVVDP_HELD_MAX_TAPS 32

/* One stream.  Sample (c, px) of source frame f is element d_data[c * chan_stride + f * frame_stride + px] (strides in elements
 * of the sample type; a frame's H*W samples contiguous).  n_frames: the source frames behind d_data -- every index of the
 * stream's list must lie in [0, n_frames). */
typedef struct fvvdp_held_stream {
    const void* d_data;
    size_t chan_stride;
    size_t frame_stride;
    int32_t n_frames;
} fvvdp_held_stream;

/* fvvdp_temporal_channels with one stream descriptor and one window index list PER STREAM: level 0 of slots [slot0, slot0 +
 * n_out) of a video context.
 *   test, ref                    the two streams; dtype (FVVDP_U8 ... FVVDP_BF16) and C (1 or 3) are shared;
 *   h_idx_test, h_idx_ref        [fl - 1 + n_out] source frames of each stream per virtual time step: the display-rate list
 *                                (fvvdp_temporal_channels' h_frame_idx) sent through the stream's frame map;
 *   every other argument         as fvvdp_temporal_channels; 1 <= fl <= FVVDP_HELD_MAX_TAPS.
 * The kernels are the register-ring bodies of fvvdp_temporal_channels (vector variant and per-pixel fallback, every sample type)
 * instantiated with a stride pair of its own for stream 1; every arithmetic instruction is theirs.  A held frame is read again at
 * every display step it is shown in.
 * Errors: FVVDP_EINVAL (null or misaligned pointer, sample type, channel count, strides below the frame, an index outside its
 * stream, slots, display model / sample type mismatch, a still-image context), FVVDP_EUNSUPPORTED (fl). */
int fvvdp_temporal_channels_held(fvvdp_ctx* ctx, const fvvdp_held_stream* test, const fvvdp_held_stream* ref, int dtype, int C,
                                 const fvvdp_eotf* eotf, const float* h_rgb2y, const int32_t* h_idx_test,
                                 const int32_t* h_idx_ref, const float* h_taps, int fl, int n_out, int slot0,
                                 int32_t* d_oob_flag, void* stream);

/* Bytes at the head of the side buffer of the function below that hold the frame map of n_display frames: int32 entries, rounded
 * up to 256 bytes.  The fl * height * width floats of fvvdp_video_grad_input's side buffer follow. */
#define FVVDP_HELD_MAP_BYTES(n_display) ((((size_t)(n_display) * 4) + 255) / 256 * 256)

/* fvvdp_video_grad_input_st for a stream shown through a frame map: d_g0 [n_display][2][H][W] at the display's rate -> d_grad, the
 * gradient of every sample of the stream's n_source frames (laid out as d_src; every source frame written exactly once, in
 * ascending order, exact zeros in a frame that no position of the list shows).
 *   n_display, n_source          display frames (N) and source frames of this stream;
 *   h_map                        [n_display] display frame -> source frame: non-decreasing, inside [0, n_source); uploaded to the
 *                                head of the side buffer (the host copy is the library's own: the caller's may go at once);
 *   h_fold_frame, h_fold_pos     [fl] the head of the display-rate list keyed by SOURCE frame: entry i says that head position
 *                                h_fold_pos[i] shows source frame h_fold_frame[i] = h_map[list[position]]; every position of
 *                                [0, fl) exactly once, sorted by frame and then by position;
 *   d_src, d_grad, dtype         the stream's clip and its gradient (FVVDP_F32 / F16 / BF16), chan_stride / frame_stride in samples;
 *   d_head, head_bytes           256-byte aligned, at least FVVDP_HELD_MAP_BYTES(n_display) + fl * H * W * 4 bytes;
 *   every other argument         as fvvdp_video_grad_input_st; 1 <= fl <= FVVDP_HELD_MAX_TAPS.
 * One launch; a lane owns its pixels for the whole clip.  Per list position the multiply-add chain over the ring of open
 * positions is fvvdp_video_grad_input's.  A finished streaming position is added to the running sum S_j of the source frame j it
 * shows; when the map moves on (or the list ends) grad_c[j] = w_c EOTF'(V_c[j]) S_j is written, S_j = the head positions of j in
 * ascending order, then its streaming positions in ascending order.  With the identity map (n_display == n_source) the output
 * equals fvvdp_video_grad_input_st's bit for bit.
 * Errors: FVVDP_EINVAL (null or misaligned pointer, bad shape, sample type, strides, display model, a map that decreases or leaves
 * [0, n_source), a fold list that is unsorted, incomplete or out of range, a side buffer that is too small), FVVDP_EUNSUPPORTED (fl). */
int fvvdp_video_grad_input_held(int width, int height, int n_display, int n_source, const float* d_g0, const int32_t* h_map,
                                const int32_t* h_fold_frame, const int32_t* h_fold_pos, const float* h_taps, int fl,
                                const void* d_src, void* d_grad, int dtype, int C, size_t chan_stride, size_t frame_stride,
                                const fvvdp_eotf* eotf, const float* h_rgb2y, void* d_head, size_t head_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FVVDP_HIP_HELD_H */
