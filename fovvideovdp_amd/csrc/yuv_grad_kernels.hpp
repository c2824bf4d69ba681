// Planar YUV clips of float32 code values (include/fvvdp_hip_yuv_grad.h): their ingest fused with the temporal filter, the
// temporal transpose down to the luminance frames, and the adjoint of the unpack.  Instantiated and launched by
// yuv_grad_launch.hip, which compiles nothing else: no kernel template of the other translation units is instantiated here.
//
// Forward, per pixel (y, x) of a frame (yuv_lum of temporal_kernels.hpp with a float sample in the place of (float)code):
//   Yf = clamp(wy Y - 16/219, 0, 1),  c = clamp(wc C - 128/224, -0.5, 0.5) for both chroma planes,
//   (u, v) = 4:2:0: bilinear x2 of c (source coordinate (dst + 0.5) / 2 - 0.5 clamped at 0, upper neighbour clamped at the last
//            row / column), 4:4:4: c itself,
//   rgb_k = clip(m[3k] Yf + m[3k+1] u + m[3k+2] v, 0, 1),  Lum = sum_k w_k EOTF(rgb_k),  then the sliding-window FIR.
// Backward, once per clip:
//   video_lum_input_kernel   gL[j]  = sum_{p : idx[p] = j} sum_cc sum_k taps[cc][k] g0[p - (fl - 1) + k][cc]
//   yuv_adjoint_*_kernel     d_k = gL w_k EOTF'(rgb_k) (0 at the clip);  dYf = sum_k m[3k] d_k, du = sum_k m[3k+1] d_k, dv likewise;
//                            dY = wy dYf, dC = wc Upsample^T(du | dv), each where its clamp does not bind
#pragma once

struct YuvPlaneSet {
    const float* y;
    const float* u;
    const float* v;
    size_t ys, cs;          // elements between frames: luma plane, chroma planes
};

// what the unpack of one pixel reads besides the planes (members of both argument blocks below)
struct YuvUnpack {
    int W, H, uvw, uvh;
    int chroma420;
    float wy, wc;           // 1/(2^(b-8)*219), 1/(2^(b-8)*224)
    float m[9];             // ycbcr2rgb, row-major
    EotfDev e;
    float w[3];
};

// source index, upper neighbour and weight of the upper neighbour of destination sample d of one axis of the x2 upsampling
__device__ __forceinline__ void up_axis(int d, int n_src, int& i0, int& i1, float& f) {
    const float s = fmaxf(((float)d + 0.5f) * 0.5f - 0.5f, 0.0f);
    i0 = (int)s;
    i1 = min(i0 + 1, n_src - 1);
    f = s - (float)i0;
}

__device__ __forceinline__ float yp_chroma(float code, float wc) {
    return fminf(fmaxf(wc * code - (128.0f / 224.0f), -0.5f), 0.5f);
}

// Yf and the (upsampled, clamped) chroma of pixel (y, x) of the frame whose planes start at Y, U, V
__device__ __forceinline__ void yp_unpack(const float* __restrict__ Y, const float* __restrict__ U, const float* __restrict__ V,
                                          const YuvUnpack& a, int y, int x, float& Yf, float& u, float& v) {
    Yf = fminf(fmaxf(a.wy * Y[y * a.W + x] - (16.0f / 219.0f), 0.0f), 1.0f);
    auto cf = [&](const float* pl, int yy, int xx) { return yp_chroma(pl[yy * a.uvw + xx], a.wc); };
    if (a.chroma420) {
        int y0, y1, x0, x1;
        float fy, fx;
        up_axis(y, a.uvh, y0, y1, fy);
        up_axis(x, a.uvw, x0, x1, fx);
        const float gy = 1.0f - fy, gx = 1.0f - fx;
        u = gy * (gx * cf(U, y0, x0) + fx * cf(U, y0, x1)) + fy * (gx * cf(U, y1, x0) + fx * cf(U, y1, x1));
        v = gy * (gx * cf(V, y0, x0) + fx * cf(V, y0, x1)) + fy * (gx * cf(V, y1, x0) + fx * cf(V, y1, x1));
    } else {
        u = cf(U, y, x);
        v = cf(V, y, x);
    }
}

// the luminance of (Yf, u, v): matrix, clip, display model, RGB -> Y, with the roundings of yuv_lum
template <typename B>
__device__ __forceinline__ float yp_lum(float Yf, float u, float v, const YuvUnpack& a, B& bad) {
    float L = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float rgb = a.m[3 * c] * Yf + a.m[3 * c + 1] * u + a.m[3 * c + 2] * v;
        rgb = fminf(fmaxf(rgb, 0.0f), 1.0f);
        const float l = __fmul_rn(eotf_f32(rgb, a.e, bad), a.w[c]);
        L = (c == 0) ? l : __fadd_rn(L, l);
    }
    return L;
}

// ---- ingest --------------------------------------------------------------------------------------------------------------
struct YuvPlanesArgs {
    YuvPlaneSet src[2];     // test, reference
    YuvUnpack k;
    int n_out, fl;
    L0Addr out;             // level 0 (see TemporalArgs::out)
    int* oob;
    float taps2[32][2];     // {sustained, transient} tap k, see TemporalArgs
    int idx[T_MAX_IDX];
};

// The per-pixel kernel: temporal_yuv_kernel (temporal_kernels.hpp) on plane pointers.  One thread owns PX pixels 256 apart and
// keeps the last FL luminance pairs in a register ring with compile-time slots.
template <int FL, int PX>
__global__ __launch_bounds__(256) void yuvplanes_ring_kernel(const YuvPlanesArgs a) {
    const int HW = a.k.W * a.k.H;
    int px[PX];
    bool ok[PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) {
        const int q = blockIdx.x * (256 * PX) + i * 256 + threadIdx.x;
        ok[i] = q < HW;
        px[i] = ok[i] ? q : HW - 1;
    }
    OobMax bad;
    v2f ring[FL][PX];               // .x = test, .y = reference; every slot is written before its first read
    const int total = FL - 1 + a.n_out;
    typedef const int __attribute__((address_space(4)))* karg_int_p;
    typedef const char __attribute__((address_space(4)))* karg_p;
    const karg_p ka = (karg_p)__builtin_amdgcn_kernarg_segment_ptr();
    const karg_int_p idx0 = (karg_int_p)(ka + offsetof(YuvPlanesArgs, idx));
    for (int v0 = 0; v0 < total; v0 += FL) {
#pragma unroll
        for (int u = 0; u < FL; ++u) {
            const int v = v0 + u;
            if (v < total) {
                const size_t fr = (size_t)idx0[v];
#pragma unroll
                for (int i = 0; i < PX; ++i) {
                    const int y = px[i] / a.k.W, x = px[i] - y * a.k.W;
                    float L[2];
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        float Yf, cu, cv;
                        yp_unpack(a.src[s].y + fr * a.src[s].ys, a.src[s].u + fr * a.src[s].cs, a.src[s].v + fr * a.src[s].cs, a.k, y, x,
                                  Yf, cu, cv);
                        L[s] = yp_lum(Yf, cu, cv, a.k, bad);
                    }
                    ring[u][i] = v2f{L[0], L[1]};
                    asm volatile("" : "+v"(ring[u][i]));
                }
                if (v >= FL - 1) {
                    v2f accS[PX], accT[PX];
#pragma unroll
                    for (int i = 0; i < PX; ++i) accS[i] = accT[i] = v2f{0.0f, 0.0f};
                    // taps: TAPC per scalar load, laundered pointer, one chunk alive at a time (see temporal_ring_kernel)
                    karg_p tp = ka + offsetof(YuvPlanesArgs, taps2);
                    asm volatile("" : "+s"(tp));
#pragma unroll
                    for (int c = FL / TAPC - 1; c >= 0; --c) {
                        const vtapf tc = *(karg_taps_p)(tp + c * (8 * TAPC));
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
    if (is_oob(bad) && a.oob) atomicOr(a.oob, 1);
}

// The fast path (W % 4 == 0, aligned planes and strides): a lane owns 4 consecutive pixels of a row for the whole launch.  Per
// frame and stream it makes one 16-byte luma load and, per chroma plane, 4:2:0: one 8-byte load of its own two columns in each of
// the two source rows plus the column to the left and to the right (clamped to the plane: a second, 4-byte load each), 4:4:4:
// one 16-byte load.  What depends on the position alone (rows, weights, offsets) is computed once.  The loop over the frames is
// rolled; the window of the last FL luminance pairs stays where it is and the FIR of a frame is one of FL straight-line variants
// (yuv_window_dispatch).  The four float4 results of a lane go through LDS so that every store instruction of a wave writes 1 KiB
// of consecutive level-0 pixels (the transpose of temporal_yuv_vec_kernel).
constexpr int YP_PX = 4;
template <int FL, bool C420>
__global__ __launch_bounds__(256) void yuvplanes_vec_kernel(const YuvPlanesArgs a_byval) {
    const YuvPlanesArgs& a = *(const YuvPlanesArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    (void)a_byval;
    constexpr int PX = YP_PX;
    __shared__ float4 s_all[4][64 * (PX + 1)];
    typedef const int __attribute__((address_space(4)))* karg_int_p;
    typedef const char __attribute__((address_space(4)))* karg_p;
    const karg_p ka = (karg_p)__builtin_amdgcn_kernarg_segment_ptr();
    const karg_int_p idx = (karg_int_p)(ka + offsetof(YuvPlanesArgs, idx));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float4* s_t = s_all[wave];
    const int W = a.k.W, HW = a.k.W * a.k.H, uvw = a.k.uvw;
    const int wave_px = ((int)blockIdx.x * 256 + wave * 64) * PX;          // first pixel of the wave's run of 256
    const int p = min(wave_px / PX + lane, HW / PX - 1) * PX;              // (a lane past the frame repeats the last quad, stores nothing)
    const int y = p / W, x = p - y * W;
    // 4:2:0: the two source rows and the four source columns of the lane's pixels, with the weights of the forward's formula
    int oc[2] = {p, p}, ocl[2] = {0, 0}, ocr[2] = {0, 0};
    float fy = 0.0f, fx[PX] = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (C420) {
        int y0, y1, x0, x1;
        up_axis(y, a.k.uvh, y0, y1, fy);
        const int j2 = x >> 1;
        const int cl = max(j2 - 1, 0), cr = min(j2 + 2, uvw - 1);
        oc[0] = y0 * uvw + j2;  oc[1] = y1 * uvw + j2;
        ocl[0] = y0 * uvw + cl; ocl[1] = y1 * uvw + cl;
        ocr[0] = y0 * uvw + cr; ocr[1] = y1 * uvw + cr;
#pragma unroll
        for (int i = 0; i < PX; ++i) up_axis(x + i, uvw, x0, x1, fx[i]);
    }
    const float gy = 1.0f - fy;
    v2f win[FL][PX];
#pragma unroll
    for (int u = 0; u < FL; ++u)
#pragma unroll
        for (int i = 0; i < PX; ++i) win[u][i] = splat(0.0f);
    OobMax bad;
    const int total = FL - 1 + a.n_out;
    for (int v = 0; v < total; ++v) {
        const size_t fr = (size_t)idx[v];
        float Lm[2][PX];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const float* Yp = a.src[s].y + fr * a.src[s].ys;
            const float* Cp[2] = {a.src[s].u + fr * a.src[s].cs, a.src[s].v + fr * a.src[s].cs};
            const v4f yq = *reinterpret_cast<const v4f*>(Yp + p);
            float cu[2][PX];                                               // upsampled clamped chroma of the 4 pixels, per plane
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                if constexpr (C420) {
                    float col[2][4];                                       // [source row][column j2-1, j2, j2+1, j2+2]
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        const v2f own = *reinterpret_cast<const v2f*>(Cp[pl] + oc[r]);
                        col[r][0] = yp_chroma(Cp[pl][ocl[r]], a.k.wc);
                        col[r][1] = yp_chroma(own.x, a.k.wc);
                        col[r][2] = yp_chroma(own.y, a.k.wc);
                        col[r][3] = yp_chroma(Cp[pl][ocr[r]], a.k.wc);
                    }
                    // pixel i reads columns (0,1), (1,2), (1,2), (2,3); at x == 0 the weight of the upper neighbour is 0 and the
                    // lower one is column 0 itself, which is what slot 0 then holds
#pragma unroll
                    for (int i = 0; i < PX; ++i) {
                        const int c0 = i == 0 ? 0 : (i == 3 ? 2 : 1);
                        const float gx = 1.0f - fx[i];
                        cu[pl][i] = gy * (gx * col[0][c0] + fx[i] * col[0][c0 + 1]) + fy * (gx * col[1][c0] + fx[i] * col[1][c0 + 1]);
                    }
                } else {
                    const v4f cq = *reinterpret_cast<const v4f*>(Cp[pl] + p);
                    cu[pl][0] = yp_chroma(cq.x, a.k.wc); cu[pl][1] = yp_chroma(cq.y, a.k.wc);
                    cu[pl][2] = yp_chroma(cq.z, a.k.wc); cu[pl][3] = yp_chroma(cq.w, a.k.wc);
                }
            }
            const float yv[PX] = {yq.x, yq.y, yq.z, yq.w};
#pragma unroll
            for (int i = 0; i < PX; ++i) {
                const float Yf = fminf(fmaxf(a.k.wy * yv[i] - (16.0f / 219.0f), 0.0f), 1.0f);
                Lm[s][i] = yp_lum(Yf, cu[0][i], cu[1][i], a.k, bad);
            }
        }
        v2f lum[PX];
#pragma unroll
        for (int i = 0; i < PX; ++i) lum[i] = v2f{Lm[0][i], Lm[1][i]};
        v2f acc_s[PX], acc_t[PX];
        karg_p tp = ka + offsetof(YuvPlanesArgs, taps2);
        if constexpr (FL > 8) asm volatile("" : "+s"(tp));
        yuv_window_dispatch<FL, PX>(v & (FL - 1), win, lum, tp, acc_s, acc_t);
        if (v >= FL - 1) {                                                 // (wave-uniform)
            wave_lds_order();
#pragma unroll
            for (int i = 0; i < PX; ++i) s_t[lane * (PX + 1) + i] = make_float4(acc_s[i].x, acc_s[i].y, acc_t[i].x, acc_t[i].y);
            wave_lds_order();
            float* o = l0_frame(a.out, v - (FL - 1));
#pragma unroll
            for (int i = 0; i < PX; ++i) {
                const int q = i * 64 + lane;                               // pixel q of the wave's run: quad q / PX, its pixel q % PX
                const float4 val = s_t[(q / PX) * (PX + 1) + (q % PX)];
                if (wave_px + q < HW)
                    __builtin_nontemporal_store(v4f{val.x, val.y, val.z, val.w}, reinterpret_cast<v4f*>(o + (size_t)(wave_px + q) * 4));
            }
        }
    }
    if (is_oob(bad) && a.oob) atomicOr(a.oob, 1);
}

// ---- temporal transpose down to the luminance frames ------------------------------------------------------------------------
// The transpose of transpose_kernels.hpp with a plain store as its tail: gL[j] = s[j], the sum video_input_kernel
// (video_grad_kernels.hpp) forms before its display model, with the same order of additions.
struct LumInputArgs {
    TransposeArgs t;        // g0, head, sizes, taps and fold list
    float* gL;              // [N][HW]
};
static_assert(offsetof(LumInputArgs, t) == 0, "transpose_step and FoldCursor read the start of the kernel-argument segment");

// FL, PX: see TransposeRing
template <int FL, int PX>
__global__ __launch_bounds__(256) void video_lum_input_kernel(const LumInputArgs a) {
    const size_t px = ((size_t)blockIdx.x * 256 + threadIdx.x) * PX;
    if (px >= (size_t)a.t.HW) return;
    TransposeRing<FL, PX> ring = transpose_ring<FL, PX>();
    const size_t HW = (size_t)a.t.HW;
    FoldCursor<PX> fold(a.t.head, HW, px, a.t.fl);
    const int total = a.t.N + a.t.fl - 1;
    for (int p = 0; p < total; ++p) {
        const int j = p - (a.t.fl - 1);         // the frame that is complete after this step
        LaneVec<PX> gs, gt;
        transpose_inputs<PX>(a.t.g0, p, a.t.N, HW, px, gs, gt);
        const LaneVec<PX> done = transpose_step<FL, PX>(ring, gs, gt);
        if (p < a.t.fl) lane_store<PX>(a.t.head + (size_t)p * HW + px, done);
        if (j >= 0) lane_store<PX>(a.gL + (size_t)j * HW + px, fold.frame_sum(j, done));
    }
}

// ---- adjoint of the unpack -----------------------------------------------------------------------------------------------
struct YuvAdjArgs {
    const float* gL;        // [N][H][W]
    YuvPlaneSet t;          // the test planes
    float* gy;              // the gradient planes: frame f of luma at gy + f * gys, of chroma at gu / gv + f * gcs
    float* gu;
    float* gv;
    size_t gys, gcs;
    YuvUnpack k;
};

// dYf, du, dv of luma pixel (y, x) of the frame at Y, U, V; returns whether the luma clamp lets a gradient through
__device__ __forceinline__ bool yuv_adjoint_pixel(const float* __restrict__ Y, const float* __restrict__ U,
                                                  const float* __restrict__ V, const YuvUnpack& a, int y, int x, float g,
                                                  float& dYf, float& du, float& dv) {
    float Yf, u, v;
    yp_unpack(Y, U, V, a, y, x, Yf, u, v);
    dYf = du = dv = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float rgb = a.m[3 * c] * Yf + a.m[3 * c + 1] * u + a.m[3 * c + 2] * v;
        // the clip to [0, 1] in front of every display model (LINEAR and ABSOLUTE have no clamp of their own there)
        const float d = (rgb >= 0.0f && rgb <= 1.0f) ? g * a.w[c] * eotf_grad(rgb, a.e) : 0.0f;
        dYf = fmaf(a.m[3 * c], d, dYf);
        du = fmaf(a.m[3 * c + 1], d, du);
        dv = fmaf(a.m[3 * c + 2], d, dv);
    }
    const float yl = a.wy * Y[y * a.W + x] - (16.0f / 219.0f);
    return yl >= 0.0f && yl <= 1.0f;
}
__device__ __forceinline__ bool yp_chroma_open(float code, float wc) {
    const float c = wc * code - (128.0f / 224.0f);
    return c >= -0.5f && c <= 0.5f;
}

// weight of source sample `src` in destination sample d of one axis of the x2 upsampling (0 for d outside [0, n_dst))
__device__ __forceinline__ float up_weight(int d, int n_dst, int src, int n_src) {
    if (d < 0 || d >= n_dst) return 0.0f;
    int i0, i1;
    float f;
    up_axis(d, n_src, i0, i1, f);
    return (i0 == src ? 1.0f - f : 0.0f) + (i1 == src ? f : 0.0f);
}

// 4:2:0.  grid (ceil(W / 64), ceil(H / 32), N), 256 threads.  Phase 1: every pixel of the 66 x 34 tile-with-halo that lies in the
// frame computes (dYf, du, dv); pixels of the tile proper write dY; du and dv go to LDS, even and odd columns apart, so that the
// lanes of phase 2 -- consecutive chroma columns -- read consecutive words (YA_PAR words between the two column parities keep the
// writes of consecutive pixels on different banks as well).  Phase 2: chroma sample (I, J) sums the 4 x 4 luma pixels
// (2I - 1 .. 2I + 2) x (2J - 1 .. 2J + 2), columns first, ascending, with the weight the forward gives sample (I, J) in that pixel
// (1/4 or 3/4 per axis; at the frame's border the clamped neighbour is the sample itself, which folds the outside row or column
// onto it), a pixel outside the frame with weight 0.
constexpr int YA_TW = 64, YA_TH = 32;
constexpr int YA_PAR = 48;                      // >= (YA_TW + 2) / 2, and 16 mod 32
constexpr int YA_ROW = 2 * YA_PAR;
__global__ __launch_bounds__(256) void yuv_adjoint_420_kernel(const YuvAdjArgs a) {
    __shared__ float s_d[2][(YA_TH + 2) * YA_ROW];
    const int tid = threadIdx.x, f = blockIdx.z;
    const int tx0 = blockIdx.x * YA_TW, ty0 = blockIdx.y * YA_TH;
    const int W = a.k.W, H = a.k.H;
    const float* Y = a.t.y + (size_t)f * a.t.ys;
    const float* U = a.t.u + (size_t)f * a.t.cs;
    const float* V = a.t.v + (size_t)f * a.t.cs;
    const float* g = a.gL + (size_t)f * W * H;
    for (int e = tid; e < (YA_TH + 2) * (YA_TW + 2); e += 256) {
        const int ly = e / (YA_TW + 2), lx = e - ly * (YA_TW + 2);
        const int y = ty0 - 1 + ly, x = tx0 - 1 + lx;
        float dYf = 0.0f, du = 0.0f, dv = 0.0f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const bool open = yuv_adjoint_pixel(Y, U, V, a.k, y, x, g[y * W + x], dYf, du, dv);
            if (ly >= 1 && ly <= YA_TH && lx >= 1 && lx <= YA_TW)
                a.gy[(size_t)f * a.gys + y * W + x] = open ? a.k.wy * dYf : 0.0f;
        }
        const int o = ly * YA_ROW + (lx & 1) * YA_PAR + (lx >> 1);
        s_d[0][o] = du;
        s_d[1][o] = dv;
    }
    __syncthreads();
    const int uvw = a.k.uvw, uvh = a.k.uvh;
    for (int c = tid; c < (YA_TH / 2) * (YA_TW / 2); c += 256) {
        const int ci = c / (YA_TW / 2), cj = c - ci * (YA_TW / 2);
        const int I = ty0 / 2 + ci, J = tx0 / 2 + cj;
        if (I >= uvh || J >= uvw) continue;
        float wr[4], wk[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            wr[r] = up_weight(2 * I - 1 + r, H, I, uvh);
            wk[r] = up_weight(2 * J - 1 + r, W, J, uvw);
        }
        const size_t co = (size_t)I * uvw + J;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            float s = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ly = 2 * ci + r;                              // tile row of luma row 2I - 1 + r
                float t = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int lx = 2 * cj + k;
                    t = fmaf(wk[k], s_d[pl][ly * YA_ROW + (lx & 1) * YA_PAR + (lx >> 1)], t);
                }
                s = fmaf(wr[r], t, s);
            }
            const float code = (pl == 0 ? U : V)[co];
            (pl == 0 ? a.gu : a.gv)[(size_t)f * a.gcs + co] = yp_chroma_open(code, a.k.wc) ? a.k.wc * s : 0.0f;
        }
    }
}

// 4:4:4: pointwise.  grid (ceil(H W / 256), N)
__global__ __launch_bounds__(256) void yuv_adjoint_444_kernel(const YuvAdjArgs a) {
    const int W = a.k.W, HW = a.k.W * a.k.H;
    const int p = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (p >= HW) return;
    const float* Y = a.t.y + (size_t)f * a.t.ys;
    const float* U = a.t.u + (size_t)f * a.t.cs;
    const float* V = a.t.v + (size_t)f * a.t.cs;
    const int y = p / W, x = p - y * W;
    float dYf, du, dv;
    const bool open = yuv_adjoint_pixel(Y, U, V, a.k, y, x, a.gL[(size_t)f * HW + p], dYf, du, dv);
    a.gy[(size_t)f * a.gys + p] = open ? a.k.wy * dYf : 0.0f;
    a.gu[(size_t)f * a.gcs + p] = yp_chroma_open(U[p], a.k.wc) ? a.k.wc * du : 0.0f;
    a.gv[(size_t)f * a.gcs + p] = yp_chroma_open(V[p], a.k.wc) ? a.k.wc * dv : 0.0f;
}
