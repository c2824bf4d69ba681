// Batched still-image ingest: unpack + display photometry + luminance of N separate (test, reference) image pairs into pyramid
// level 0 of N slots of a still-image context (planes == 2), one launch.  Declared here for fvvdp_hip.hip,
// instantiated in still_launch.hip.
//
// The arithmetic is Sampler::lum, as in temporal_generic_kernel<SRC, 2> (the single-image path): every slot's level 0 is
// bit-identical to what that kernel writes for the same pair.  What differs is the work decomposition:
//   - the images are separate allocations: a per-slot table of (test, reference) device pointers rides in the kernel arguments
//     (no stacking copy, no upload, no stream synchronisation);
//   - a lane owns PX consecutive pixels (uint8 / float: one 4 B / 16 B load per channel and stream for PX = 4, two 16 B stores;
//     uint16: PX = 1, see still_launch.hip), and a
//     workgroup walks STILL_ITER runs of 256 * PX pixels, so the 768-entry uint8 table in LDS is built once per 4096 pixels
//     instead of once per 256;
//   - the out-of-range flag is one int32 per slot, so the caller can name the offending pair.
// Bytes per pixel: 2 * C * sizeof(sample) read, 8 written (float2 {L_test, L_ref}).
#pragma once

#define STILL_MAX_SLOTS 128     // slots per launch: 128 x 2 pointers = 2 KB of the 4 KB kernel-argument segment
#define STILL_ITER 4            // runs of 256 * PX pixels per workgroup

struct StillArgs {
    const void* test[STILL_MAX_SLOTS];
    const void* ref[STILL_MAX_SLOTS];
    size_t chan_stride;     // elements between colour channels of one image
    int C, HW;
    EotfDev e;
    float w[3];
    L0Addr out;             // slot k of the launch -> l0_frame(out, k), [HW][2] floats
    int* oob;               // [n] flags of the launch's slots (nullptr: not reported)
};

template <int SRC, int PX>
__device__ __forceinline__ void still_ingest_body(const StillArgs& a, const float* lutw) {
    const int k = blockIdx.y;
    Sampler<SRC, PX> S[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        S[s].base = s == 0 ? a.test[k] : a.ref[k];
        S[s].chan_stride = a.chan_stride;
        S[s].C = a.C;
        S[s].lutw = lutw;
        S[s].lut16 = a.e.lut;
        S[s].w0 = a.C == 3 ? a.w[0] : 1.0f;
        S[s].w1 = a.w[1];
        S[s].w2 = a.w[2];
        S[s].e = a.e;
    }
    float* dst = l0_frame(a.out, k);
    bool bad = false;
    const long long run0 = (long long)blockIdx.x * STILL_ITER * 256 * PX;
#pragma unroll 1
    for (int it = 0; it < STILL_ITER; ++it) {
        // the host picks PX = 4 only when HW % 4 == 0, so a lane's group is either wholly inside the image or wholly outside
        const long long p = run0 + ((long long)it * 256 + threadIdx.x) * PX;
        if (p + PX > a.HW) break;
        float lt[PX], lr[PX];
        S[0].lum((size_t)p, lt, bad);
        S[1].lum((size_t)p, lr, bad);
        float* q = dst + (size_t)p * 2;
        if constexpr (PX == 4) {
            reinterpret_cast<float4*>(q)[0] = make_float4(lt[0], lr[0], lt[1], lr[1]);
            reinterpret_cast<float4*>(q)[1] = make_float4(lt[2], lr[2], lt[3], lr[3]);
        } else {
#pragma unroll
            for (int i = 0; i < PX; ++i) reinterpret_cast<float2*>(q)[i] = make_float2(lt[i], lr[i]);
        }
    }
    // one atomic per wave that saw an out-of-range sample
    if (a.oob && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(a.oob + k, 1);
}

template <int SRC, int PX>
__global__ __launch_bounds__(256) void still_ingest_kernel(const StillArgs a) {
    __shared__ float lutw[SRC == SRC_U8 ? 768 : 1];
    if constexpr (SRC == SRC_U8) {
        build_lutw(lutw, a.e, a.C, a.w, threadIdx.x, 256);
        __syncthreads();
    }
    still_ingest_body<SRC, PX>(a, lutw);
}
// float16 / bfloat16 samples (widened exactly, then the float path): an entry point of its own on the same body
template <int SRC, int PX>
__global__ __launch_bounds__(256) void still_ingest_half_kernel(const StillArgs a) {
    static_assert(src_is_half(SRC), "float16 / bfloat16");
    still_ingest_body<SRC, PX>(a, nullptr);
}

// still_launch.hip: the instantiations, in a translation unit of their own (see there); px = 4 or 1
void still_launch(int dtype, int px, const StillArgs& a, int n, hipStream_t st);
