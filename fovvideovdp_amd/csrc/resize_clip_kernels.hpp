// Clips whose streams have frame sizes of their own (include/fvvdp_hip_resize.h): the full-screen resize fused with the ingest
// and the temporal filter, and the adjoint of the resize.  Instantiated and launched by resize_launch.hip, which compiles nothing
// else; the variants for streams shown through frame maps (include/fvvdp_hip_resize_held.h: resized_hold_ring_kernel,
// resize_adjoint_run_d_kernel) by resize_held_launch.hip.  The per-frame path of the integer YUV source class (resize_kernels.hpp)
// is not touched.
//
// Forward, per stream and target pixel (oy, ox):
//   v_c = Interp_mode(channel c of the frame)(oy, ox) in torch's order of operations (resize_lum_kernel of resize_kernels.hpp,
//         oracle.torch_interpolate), a stream of the target's size: the sample itself;
//   Lum = sum_c w_c EOTF(clip(v_c, 0, 1)),  then the sliding-window FIR of yuvplanes_ring_kernel.
// Backward, once per clip, after video_lum_input_kernel (yuv_grad_kernels.hpp) has made gL:
//   resize_adjoint_d_kernel       d_c[oy][ox] = gL w_c EOTF'(v_c) where v_c lies in [0, 1], 0 where the clip binds
//   resize_adjoint_gather_kernel  grad[c][y][x] = sum_oy wy(oy -> y) sum_ox wx(ox -> x) d_c[oy][ox]
// The index arithmetic of one axis (rz_*_axis, resize_axis.hpp) is host and device code: the tap setup of the forward, the weights
// of the gather and the host's candidate ranges all call the same functions.
#pragma once

#include "resize_axis.hpp"

struct RzStream {
    const void* p;
    int u8;                 // samples are uint8 codes (value = code / 255), else float32
    int C, W, H;
    int identity;           // W x H is the target: no resampling
    size_t fs, ps;          // elements between frames, between the planes of a frame
    float sx, sy;           // W / Wo, H / Ho in fp32 (torch: area_pixel_compute_scale without a scale factor)
};

// ---- what a target pixel reads: computed once, before the loop over the frames -------------------------------------------------
template <int MODE>
struct RzTaps;
template <>
struct RzTaps<FVVDP_RESIZE_NEAREST> { int off; };
template <>
struct RzTaps<RZ_IDENTITY> { int off; };
template <>
struct RzTaps<FVVDP_RESIZE_BILINEAR> { int r0, r1, x0, x1; float ly1, lx1; };       // row offsets y * W
template <>
struct RzTaps<FVVDP_RESIZE_BICUBIC> { int r[4], x[4]; float cy[4], cx[4]; };
template <>
struct RzTaps<FVVDP_RESIZE_AREA> { int y0, y1, x0, x1; float n; };

template <int MODE>
__device__ __forceinline__ void rz_setup(RzTaps<MODE>& t, const RzStream& s, int oy, int ox, int Wo, int Ho) {
    if constexpr (MODE == FVVDP_RESIZE_NEAREST) {
        t.off = rz_nearest_axis(oy, s.H, s.sy) * s.W + rz_nearest_axis(ox, s.W, s.sx);
    } else if constexpr (MODE == RZ_IDENTITY) {
        t.off = oy * s.W + ox;
    } else if constexpr (MODE == FVVDP_RESIZE_BILINEAR) {
        int y0, y1;
        rz_bilinear_axis(oy, s.H, s.sy, y0, y1, t.ly1);
        rz_bilinear_axis(ox, s.W, s.sx, t.x0, t.x1, t.lx1);
        t.r0 = y0 * s.W;
        t.r1 = y1 * s.W;
    } else if constexpr (MODE == FVVDP_RESIZE_BICUBIC) {
        int ys[4];
        rz_cubic_axis(oy, s.H, s.sy, ys, t.cy);
        rz_cubic_axis(ox, s.W, s.sx, t.x, t.cx);
#pragma unroll
        for (int k = 0; k < 4; ++k) t.r[k] = ys[k] * s.W;
    } else {
        rz_area_axis(oy, s.H, Ho, t.y0, t.y1);
        rz_area_axis(ox, s.W, Wo, t.x0, t.x1);
        t.n = (float)((t.y1 - t.y0) * (t.x1 - t.x0));
    }
}

// sample `off` of the plane at element offset `base` of the stream
__device__ __forceinline__ float rz_load(const RzStream& s, size_t base, int off) {
    if (s.u8) return (float)reinterpret_cast<const unsigned char*>(s.p)[base + off] * (1.0f / 255.0f);
    return reinterpret_cast<const float*>(s.p)[base + off];
}

// The interpolated value of one channel before its clip: the one function both streams of the ingest and the first stage of the
// adjoint evaluate.  Order of operations: resize_lum_kernel's.
template <int MODE>
__device__ __forceinline__ float rz_interp(const RzStream& s, size_t base, const RzTaps<MODE>& t) {
    if constexpr (MODE == FVVDP_RESIZE_NEAREST || MODE == RZ_IDENTITY) {
        return rz_load(s, base, t.off);
    } else if constexpr (MODE == FVVDP_RESIZE_BILINEAR) {
        const float ly0 = 1.0f - t.ly1, lx0 = 1.0f - t.lx1;
        return ly0 * (lx0 * rz_load(s, base, t.r0 + t.x0) + t.lx1 * rz_load(s, base, t.r0 + t.x1)) +
               t.ly1 * (lx0 * rz_load(s, base, t.r1 + t.x0) + t.lx1 * rz_load(s, base, t.r1 + t.x1));
    } else if constexpr (MODE == FVVDP_RESIZE_BICUBIC) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {         // x first along each of the four rows, then y (upsample_bicubic2d)
            const float row = ((rz_load(s, base, t.r[k] + t.x[0]) * t.cx[0] + rz_load(s, base, t.r[k] + t.x[1]) * t.cx[1]) +
                               rz_load(s, base, t.r[k] + t.x[2]) * t.cx[2]) + rz_load(s, base, t.r[k] + t.x[3]) * t.cx[3];
            acc = (k == 0) ? row * t.cy[0] : acc + row * t.cy[k];
        }
        return acc;
    } else {
        // the window row by row in ONE loop (lanes differ in their windows: one divergent loop costs one saved exec mask, two nested
        // ones cost scalar registers the ring kernels do not have)
        float acc = 0.0f;
        const int cnt = (t.y1 - t.y0) * (t.x1 - t.x0);
        int xx = t.x0, row = t.y0 * s.W;
        for (int k = 0; k < cnt; ++k) {
            acc += rz_load(s, base, row + xx);
            ++xx;
            const bool wrap = xx == t.x1;
            xx = wrap ? t.x0 : xx;
            row += wrap ? s.W : 0;
        }
        return acc / t.n;
    }
}

// clip, display model, luminance weights over the channels of one frame of one stream (base: the frame's first element)
template <int MODE, typename B>
__device__ __forceinline__ float rz_lum(const RzStream& s, size_t base, const RzTaps<MODE>& t, const EotfDev& e, const float (&w)[3],
                                        B& bad) {
    float L = 0.0f;
    for (int c = 0; c < s.C; ++c) {
        const float v = fminf(fmaxf(rz_interp<MODE>(s, base + (size_t)c * s.ps, t), 0.0f), 1.0f);
        const float l = __fmul_rn(eotf_f32(v, e, bad), w[c]);
        L = (c == 0) ? l : __fadd_rn(L, l);
    }
    return L;
}

// ---- ingest --------------------------------------------------------------------------------------------------------------
struct ResizedArgs {
    RzStream src[2];        // test, reference
    int Wo, Ho;
    EotfDev e;
    float w[3];
    int n_out, fl;
    L0Addr out;             // level 0 (see TemporalArgs::out)
    float taps2[32][2];     // {sustained, transient} tap k, see TemporalArgs
    int idx[T_MAX_IDX];
};

// The same block for streams that are shown through frame maps of their own (include/fvvdp_hip_resize_held.h): stream 1 reads the
// list behind the ResizedArgs, as HeldTemporalArgs' strides follow the TemporalArgs (held_kernels.hpp).
struct ResizedHoldArgs {
    ResizedArgs a;
    int idx1[T_MAX_IDX];    // the reference's list (a.idx: the test's)
};
static_assert(offsetof(ResizedHoldArgs, idx1) == sizeof(ResizedArgs), "resized_hold_ring_kernel reads stream 1's list behind the ResizedArgs");

// yuvplanes_ring_kernel (yuv_grad_kernels.hpp) with the resize in the place of the unpack.  One thread owns PX target pixels 256
// apart, sets up both streams' taps once and keeps the last FL luminance pairs in a register ring with compile-time slots.  A
// stream of the target's size takes the identity variant (a wave-uniform branch per stream).
template <int FL, int PX, int MODE>
__global__ __launch_bounds__(256) void resized_ring_kernel(const ResizedArgs a) {
    const int HW = a.Wo * a.Ho;
    int px[PX];
    bool ok[PX];
    RzTaps<MODE> tp[2][PX];
    RzTaps<RZ_IDENTITY> ti[PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) {
        const int q = blockIdx.x * (256 * PX) + i * 256 + threadIdx.x;
        ok[i] = q < HW;
        px[i] = ok[i] ? q : HW - 1;
        const int oy = px[i] / a.Wo, ox = px[i] - oy * a.Wo;
        ti[i].off = px[i];                                                  // (either stream: an identity stream has the target's size)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!a.src[s].identity) rz_setup<MODE>(tp[s][i], a.src[s], oy, ox, a.Wo, a.Ho);
            else tp[s][i] = RzTaps<MODE>{};
        }
    }
    OobMax bad;                     // never set: every value is clipped before the display model
    v2f ring[FL][PX];               // .x = test, .y = reference; every slot is written before its first read
    const int total = FL - 1 + a.n_out;
    typedef const int __attribute__((address_space(4)))* karg_int_p;
    typedef const char __attribute__((address_space(4)))* karg_p;
    const karg_p ka = (karg_p)__builtin_amdgcn_kernarg_segment_ptr();
    const karg_int_p idx0 = (karg_int_p)(ka + offsetof(ResizedArgs, idx));
    for (int v0 = 0; v0 < total; v0 += FL) {
#pragma unroll
        for (int u = 0; u < FL; ++u) {
            const int v = v0 + u;
            if (v < total) {
                const size_t fr = (size_t)idx0[v];
#pragma unroll
                for (int i = 0; i < PX; ++i) {
                    float L[2];
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const size_t base = fr * a.src[s].fs;
                        if (a.src[s].identity) L[s] = rz_lum<RZ_IDENTITY>(a.src[s], base, ti[i], a.e, a.w, bad);
                        else L[s] = rz_lum<MODE>(a.src[s], base, tp[s][i], a.e, a.w, bad);
                    }
                    ring[u][i] = v2f{L[0], L[1]};
                    asm volatile("" : "+v"(ring[u][i]));
                }
                if (v >= FL - 1) {
                    v2f accS[PX], accT[PX];
#pragma unroll
                    for (int i = 0; i < PX; ++i) accS[i] = accT[i] = v2f{0.0f, 0.0f};
                    // taps: TAPC per scalar load, laundered pointer, one chunk alive at a time (see temporal_ring_kernel)
                    karg_p tpp = ka + offsetof(ResizedArgs, taps2);
                    asm volatile("" : "+s"(tpp));
#pragma unroll
                    for (int c = FL / TAPC - 1; c >= 0; --c) {
                        const vtapf tc = *(karg_taps_p)(tpp + c * (8 * TAPC));
#pragma unroll
                        for (int kk = TAPC - 1; kk >= 0; --kk) {
                            const int k = c * TAPC + kk;
                            const int sl = (u - k + 2 * FL) % FL;
                            const v2f f = v2f{tc[2 * kk], tc[2 * kk + 1]};
#pragma unroll
                            for (int i = 0; i < PX; ++i) fir_tap(accS[i], accT[i], ring[sl][i], f);
                        }
                        if constexpr (FL > 16) __builtin_amdgcn_sched_barrier(0);
                    }
                    int t_opaque = v - (FL - 1);
                    asm volatile("" : "+s"(t_opaque));
                    float* o = l0_frame(a.out, t_opaque);
#pragma unroll
                    for (int i = 0; i < PX; ++i)
                        if (ok[i])
                            *reinterpret_cast<float4*>(o + (size_t)px[i] * 4) = make_float4(accS[i].x, accS[i].y, accT[i].x, accT[i].y);
                }
            }
        }
    }
}

// resized_ring_kernel for streams shown through frame maps of their own: each stream reads its own list, and a step whose stream
// shows the frame it showed at the previous step of the launch takes that step's luminance from the previous ring slot (a
// compile-time slot, component .x or .y) instead of converting the frame again -- the value the straight-line body would have
// produced, so level 0 keeps the bits of the expanded clips.  The comparison is on two scalar loads of the kernel-argument
// segment: a wave-uniform branch per stream and step.  The first step of a launch always converts.
// A COPY of the kernel above, not a flag on a shared body: with the body in one function that both kernels call (by reference or
// by value, the default path textually the one above) the compiler loads the argument block earlier and four of the twelve
// existing instantiations change their registers (<8, 2, 0> 86 -> 83 scalar, <16, 2, 0> 88 -> 86, <8, 1, 2> 266 + 10 -> 278 + 22
// vector, <8, 1, 3> 59 -> 72).  Whoever changes one of the two changes the other; tests/test_gpu_resize_held.py compares them bit
// for bit.
template <int FL, int PX, int MODE>
__global__ __launch_bounds__(256) void resized_hold_ring_kernel(const ResizedHoldArgs h) {
    const ResizedArgs& a = h.a;
    const int HW = a.Wo * a.Ho;
    int px[PX];
    bool ok[PX];
    RzTaps<MODE> tp[2][PX];
    RzTaps<RZ_IDENTITY> ti[PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) {
        const int q = blockIdx.x * (256 * PX) + i * 256 + threadIdx.x;
        ok[i] = q < HW;
        px[i] = ok[i] ? q : HW - 1;
        const int oy = px[i] / a.Wo, ox = px[i] - oy * a.Wo;
        ti[i].off = px[i];                                                  // (either stream: an identity stream has the target's size)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!a.src[s].identity) rz_setup<MODE>(tp[s][i], a.src[s], oy, ox, a.Wo, a.Ho);
            else tp[s][i] = RzTaps<MODE>{};
        }
    }
    OobMax bad;                     // never set: every value is clipped before the display model
    v2f ring[FL][PX];               // .x = test, .y = reference; every slot is written before its first read
    const int total = FL - 1 + a.n_out;
    typedef const int __attribute__((address_space(4)))* karg_int_p;
    typedef const char __attribute__((address_space(4)))* karg_p;
    const karg_p ka = (karg_p)__builtin_amdgcn_kernarg_segment_ptr();
    const karg_int_p idx0 = (karg_int_p)(ka + offsetof(ResizedArgs, idx));
    for (int v0 = 0; v0 < total; v0 += FL) {
#pragma unroll
        for (int u = 0; u < FL; ++u) {
            const int v = v0 + u;
            if (v < total) {
#pragma unroll
                for (int i = 0; i < PX; ++i) {
                    float L[2];
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        // (the stream's two entries are loaded where its branch stands: nothing of stream 1 is alive while stream
                        // 0 is converted.  With both flags computed in front of the pixel loop, or with the comparison written
                        // into the `if` behind the base, the 16-slot bicubic ring parked two scalar registers in vector lanes)
                        const karg_int_p idxs = s == 0 ? idx0 : (karg_int_p)(ka + offsetof(ResizedHoldArgs, idx1));
                        const int cur = idxs[v];
                        const bool same = v > 0 && idxs[v > 0 ? v - 1 : 0] == cur;      // (decided before the frame's base is made)
                        const size_t base = (size_t)cur * a.src[s].fs;
                        if (same) L[s] = s == 0 ? ring[(u - 1 + FL) % FL][i].x : ring[(u - 1 + FL) % FL][i].y;
                        else if (a.src[s].identity) L[s] = rz_lum<RZ_IDENTITY>(a.src[s], base, ti[i], a.e, a.w, bad);
                        else L[s] = rz_lum<MODE>(a.src[s], base, tp[s][i], a.e, a.w, bad);
                    }
                    ring[u][i] = v2f{L[0], L[1]};
                    asm volatile("" : "+v"(ring[u][i]));
                }
                if (v >= FL - 1) {
                    v2f accS[PX], accT[PX];
#pragma unroll
                    for (int i = 0; i < PX; ++i) accS[i] = accT[i] = v2f{0.0f, 0.0f};
                    // taps: TAPC per scalar load, laundered pointer, one chunk alive at a time (see temporal_ring_kernel)
                    karg_p tpp = ka + offsetof(ResizedArgs, taps2);
                    asm volatile("" : "+s"(tpp));
#pragma unroll
                    for (int c = FL / TAPC - 1; c >= 0; --c) {
                        const vtapf tc = *(karg_taps_p)(tpp + c * (8 * TAPC));
#pragma unroll
                        for (int kk = TAPC - 1; kk >= 0; --kk) {
                            const int k = c * TAPC + kk;
                            const int sl = (u - k + 2 * FL) % FL;
                            const v2f f = v2f{tc[2 * kk], tc[2 * kk + 1]};
#pragma unroll
                            for (int i = 0; i < PX; ++i) fir_tap(accS[i], accT[i], ring[sl][i], f);
                        }
                        if constexpr (FL > 16) __builtin_amdgcn_sched_barrier(0);
                    }
                    int t_opaque = v - (FL - 1);
                    asm volatile("" : "+s"(t_opaque));
                    float* o = l0_frame(a.out, t_opaque);
#pragma unroll
                    for (int i = 0; i < PX; ++i)
                        if (ok[i])
                            *reinterpret_cast<float4*>(o + (size_t)px[i] * 4) = make_float4(accS[i].x, accS[i].y, accT[i].x, accT[i].y);
                }
            }
        }
    }
}

// ---- adjoint ---------------------------------------------------------------------------------------------------------------
struct ResizeAdjArgs {
    const float* gL;        // [N][Ho][Wo]; the launch covers frames [f0, f0 + nf)
    RzStream t;             // the test clip (float32)
    float* grad;            // laid out as the test clip
    float* d;               // scratch [nf][C][Ho][Wo]
    const int* ylo;         // [H], [H], [W], [W]: target rows [ylo, yhi) and columns [xlo, xhi) that can reach a source row / column
    const int* yhi;
    const int* xlo;
    const int* xhi;
    int Wo, Ho, f0;
    EotfDev e;
    float w[3];
};

// Stage 1.  grid (ceil(Ho Wo / 256), nf): d_c of one target pixel of frame f0 + blockIdx.y, every channel
template <int MODE>
__global__ __launch_bounds__(256) void resize_adjoint_d_kernel(const ResizeAdjArgs a) {
    const int HWo = a.Wo * a.Ho;
    const int o = blockIdx.x * 256 + threadIdx.x, fb = blockIdx.y;
    if (o >= HWo) return;
    const int oy = o / a.Wo, ox = o - oy * a.Wo;
    RzTaps<MODE> t;
    rz_setup<MODE>(t, a.t, oy, ox, a.Wo, a.Ho);
    const size_t f = (size_t)(a.f0 + fb);
    const float g = a.gL[f * HWo + o];
    for (int c = 0; c < a.t.C; ++c) {
        const float v = rz_interp<MODE>(a.t, f * a.t.fs + (size_t)c * a.t.ps, t);
        // the clip to [0, 1] in front of every display model: open on the closed range, as torch.clamp's backward
        a.d[((size_t)fb * a.t.C + c) * HWo + o] = (v >= 0.0f && v <= 1.0f) ? g * a.w[c] * eotf_grad(v, a.e) : 0.0f;
    }
}

// Stage 1 for a test shown through a frame map (include/fvvdp_hip_resize_held.h).  a.gL is at the display's rate; the launch
// covers SOURCE frames [f0, f0 + nf), and run[j], run[j + 1] bound the display frames that show source frame j (the map is
// non-decreasing).  Every one of them has the same v_c, and both stages are linear in gL: g is the sum of gL over the run in
// ascending order, from its first frame on (a run of one gives resize_adjoint_d_kernel's bits), and d_c = g w_c EOTF'(v_c) once
// per source frame.  An empty run -- a frame no display frame shows -- writes zeros.
struct ResizeAdjRunArgs {
    ResizeAdjArgs a;
    const int* run;         // [n_source + 1] device
};

template <int MODE>
__global__ __launch_bounds__(256) void resize_adjoint_run_d_kernel(const ResizeAdjRunArgs r) {
    const ResizeAdjArgs& a = r.a;
    const int HWo = a.Wo * a.Ho;
    const int o = blockIdx.x * 256 + threadIdx.x, fb = blockIdx.y;
    if (o >= HWo) return;
    const size_t f = (size_t)(a.f0 + fb);
    const int lo = r.run[f], hi = r.run[f + 1];
    if (lo >= hi) {
        for (int c = 0; c < a.t.C; ++c) a.d[((size_t)fb * a.t.C + c) * HWo + o] = 0.0f;
        return;
    }
    float g = a.gL[(size_t)lo * HWo + o];
    for (int v = lo + 1; v < hi; ++v) g = __fadd_rn(g, a.gL[(size_t)v * HWo + o]);
    const int oy = o / a.Wo, ox = o - oy * a.Wo;
    RzTaps<MODE> t;
    rz_setup<MODE>(t, a.t, oy, ox, a.Wo, a.Ho);
    for (int c = 0; c < a.t.C; ++c) {
        const float v = rz_interp<MODE>(a.t, f * a.t.fs + (size_t)c * a.t.ps, t);
        a.d[((size_t)fb * a.t.C + c) * HWo + o] = (v >= 0.0f && v <= 1.0f) ? g * a.w[c] * eotf_grad(v, a.e) : 0.0f;
    }
}

// Stage 2.  grid (ceil(W / 64), ceil(H / 4), nf * C), block (64, 4): one source sample per thread, consecutive lanes consecutive
// columns (the d rows they read overlap or adjoin).  Fixed order of additions: rows ascending, inside a row columns ascending.
template <int MODE>
__global__ __launch_bounds__(256) void resize_adjoint_gather_kernel(const ResizeAdjArgs a) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= a.t.W || y >= a.t.H) return;
    const int fb = blockIdx.z / a.t.C, c = blockIdx.z - fb * a.t.C;
    const float* d = a.d + ((size_t)fb * a.t.C + c) * ((size_t)a.Wo * a.Ho);
    const int y0 = a.ylo[y], y1 = a.yhi[y], x0 = a.xlo[x], x1 = a.xhi[x];
    float s = 0.0f;
    for (int oy = y0; oy < y1; ++oy) {
        const float wy = rz_axis_weight<MODE>(oy, y, a.t.H, a.Ho, a.t.sy);
        if (wy == 0.0f) continue;
        const float* row = d + (size_t)oy * a.Wo;
        float r = 0.0f;
        for (int ox = x0; ox < x1; ++ox) r = fmaf(rz_axis_weight<MODE>(ox, x, a.t.W, a.Wo, a.t.sx), row[ox], r);
        s = fmaf(wy, r, s);
    }
    reinterpret_cast<float*>(a.grad)[(size_t)(a.f0 + fb) * a.t.fs + (size_t)c * a.t.ps + (size_t)y * a.t.W + x] = s;
}
