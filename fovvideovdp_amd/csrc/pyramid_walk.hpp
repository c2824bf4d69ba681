// The pyramid row walk shared by the five fused pyramid kernels (band_kernel, band2_kernel, multigaze_kernel, multitest_kernel,
// multitest_fov_kernel).
// Device only.  Included by band_kernel.hpp after its building blocks (Px, ld_px_buf, dpp_reduce_taps, dpp_expand_taps).
#pragma once
// ------------------------------------------------------------------------------------------------------------
// One copy of what every item function does the same way: the per-lane reduce and expand weights, the row loads with the
// reference's symmetric padding, the 5-tap reduce of five ring rows into a coarse row, the expand of three coarse rows into
// the four fine pixels of a step, the log-domain masking and pooling tail of the two-channel (video) pass, the four-phase step
// driver and the XCD work order.  multigaze_kernel and multitest_kernel are pinned bit for bit against band_kernel
// (tests/test_gpu_gazes.py, tests/test_gpu_multitest.py): they get the same values because they run the same code.
//
// The rule of this file: sharing a piece may not change a single instruction of any of the 34 kernel instantiations that use it
// (tests/test_pyramid_walk_cpu.py guards the registers; the comparison itself is the disassembly per kernel), nor of the five of
// multitest_fov_kernel (tests/test_tests_fov_cpu.py).  What that takes:
//   - Contraction is lexical: a function is compiled under the setting where it is WRITTEN.  band_item and band2_item
//     are compiled with floating-point contraction on, multigaze_item and multitest_item with it off.  Every function
//     here switches it off and spells each fused multiply-add as pfma / fmaf / __builtin_elementwise_fma; no a * b + c
//     is left to the compiler, in the macros neither.
//   - Scalars are passed by value and rows as references to the ring's own arrays.  Weights handed over in a struct by
//     reference cost the callers scratch memory and LDS traffic (the struct is materialised).
//   - Where a function changed the callers' code whatever its signature (a function is simplified on its own before it is
//     inlined, which reorders the caller's instructions), the piece is a statement macro: its text is compiled in the caller,
//     as the copy it replaces was.  The weights, the row loads, the reduce and the work order are functions; the expand, the
//     tail and the step driver are macros.
// ------------------------------------------------------------------------------------------------------------

// Horizontal 5-tap reduce weights of coarse column J (of wc) over a fine level of w x h, incl. the reference's edge fix-ups
// (gausspyr_reduce, fvvdp_lpyr_dec.py:198-205; the right-edge branch is selected by the parity of the ROW count, :202,
// reproduced here on purpose).  Taps: E[l-1], O[l-1], E[l], O[l], E[l+1]  (E/O = even/odd fine column of a lane); taps
// falling outside the image get weight 0 and their fix-up is folded into the in-range taps.
struct ReduceW {
    float q0, q1, q2, q3, q4;
};
__device__ __forceinline__ ReduceW lane_reduce_weights(const int J, const int wc, const int w, const int h) {
#pragma clang fp contract(off)
    const float K0 = 0.05f, K1 = 0.25f, K2 = 0.4f, K3 = 0.25f, K4 = 0.05f;
    float wq0 = K0, wq1 = K1, wq2 = K2, wq3 = K3, wq4 = K4;
    if (J == 0) {
        wq2 += K1;
        wq3 += K0;
        wq0 = 0.0f;
        wq1 = 0.0f;
    }
    if (J == wc - 1) {
        const bool hodd = (h & 1) != 0;
        if (w & 1) {   // own columns: X0 = w-1 (tap 2), X1 = w (outside)
            wq3 = 0.0f;
            wq4 = 0.0f;
            if (hodd) { wq2 += K3; wq1 += K4; } else { wq2 += K4; }
        } else {       // own columns: w-2 (tap 2), w-1 (tap 3); tap 4 = column w is outside
            wq4 = 0.0f;
            if (hodd) { wq3 += K3; wq2 += K4; } else { wq3 += K4; }
        }
    }
    return ReduceW{wq0, wq1, wq2, wq3, wq4};
}
// Horizontal expand weights of coarse column J (2K = .1 .8 .1 / .5 .5, gausspyr_expand fvvdp_lpyr_dec.py:126-142,233); a
// neighbour outside the coarse row is the clamped (own) column, so its weight moves to the centre tap.
struct ExpandW {
    float el, er, ec, orr, oc;
};
__device__ __forceinline__ ExpandW lane_expand_weights(const int J, const int wc) {
#pragma clang fp contract(off)
    const bool at_l = (J <= 0), at_r = (J >= wc - 1);
    ExpandW e;
    e.el = at_l ? 0.0f : 0.1f;
    e.er = at_r ? 0.0f : 0.1f;
    e.ec = 0.8f + (at_l ? 0.1f : 0.0f) + (at_r ? 0.1f : 0.0f);
    e.orr = at_r ? 0.0f : 0.5f;
    e.oc = at_r ? 1.0f : 0.5f;
    return e;
}

// Row r of a level of h rows under symmetric padding (fvvdp_lpyr_dec.py:190-195), clamped into the level.
__device__ __forceinline__ int reflect_row(const int r, const int h) {
    const int rr = r < 0 ? -1 - r : (r >= h ? 2 * h - 1 - r : r);
    return min(max(rr, 0), h - 1);
}
// The lane's two fine pixels of row r through a buffer resource: scalar row offset + loop-invariant lane offsets, no vector
// address arithmetic (see ld_px_buf).
template <int P>
__device__ __forceinline__ void load_row_pair(const __amdgpu_buffer_rsrc_t rsrc, const unsigned int col0_b, const unsigned int col1_b,
                                              const unsigned int row_b, const int h, const int r, Px<P>& p0, Px<P>& p1) {
    const unsigned int so = (unsigned int)reflect_row(r, h) * row_b;
    p0 = ld_px_buf<P>(rsrc, col0_b, so);
    p1 = ld_px_buf<P>(rsrc, col1_b, so);
}

// One coarse row from five fine rows (each the lane's column pair): vertical 5-tap in registers, horizontal 5-tap across lanes.
template <int P>
__device__ __forceinline__ Px<P> reduce5_rows(const Px<P> (&W0)[2], const Px<P> (&W1)[2], const Px<P> (&W2)[2], const Px<P> (&W3)[2],
                                              const Px<P> (&W4)[2], const float q0, const float q1, const float q2, const float q3,
                                              const float q4) {
#pragma clang fp contract(off)
    const float K0 = 0.05f, K1 = 0.25f, K2 = 0.4f, K3 = 0.25f, K4 = 0.05f;
    constexpr int HP = P / 2;
    Px<P> c, va, vb;
#pragma unroll
    for (int k = 0; k < HP; ++k) {
        v2f a0 = W0[0].h[k] * K0;
        a0 = pfma(W1[0].h[k], K1, a0);
        a0 = pfma(W2[0].h[k], K2, a0);
        a0 = pfma(W3[0].h[k], K3, a0);
        va.h[k] = pfma(W4[0].h[k], K4, a0);
        v2f b0 = W0[1].h[k] * K0;
        b0 = pfma(W1[1].h[k], K1, b0);
        b0 = pfma(W2[1].h[k], K2, b0);
        b0 = pfma(W3[1].h[k], K3, b0);
        vb.h[k] = pfma(W4[1].h[k], K4, b0);
    }
#pragma unroll
    for (int k = 0; k < HP; ++k) {
        v2f acc = va.h[k] * q2;
        acc = pfma(vb.h[k], q3, acc);
        c.h[k] = dpp_reduce_taps(acc, va.h[k], vb.h[k], q0, q1, q4);
    }
    return c;
}
// The window that starts in slot S0 of an 8-slot row ring.
template <int P, int S0>
__device__ __forceinline__ Px<P> reduce5_ring(const Px<P> (&R)[8][2], const float q0, const float q1, const float q2, const float q3,
                                              const float q4) {
    return reduce5_rows<P>(R[S0 & 7], R[(S0 + 1) & 7], R[(S0 + 2) & 7], R[(S0 + 3) & 7], R[(S0 + 4) & 7], q0, q1, q2, q3, q4);
}

// The expanded level at (even row | odd row, even column | odd column) of coarse row G0 from its neighbours Gm1, Gp1 (Px<2 * HP>
// each): vertical expand on the lane's coarse column (.1 .8 .1 / .5 .5), horizontal expand from lanes l-1, l, l+1 with the
// weights el .. oc of lane_expand_weights; results into x00, x01, x10, x11.
// A statement macro, not a function: as a function (outputs by reference or as a returned struct, weights as scalars or as a
// struct by value, forced inline or not) the same statements came out in another instruction order in 8 of the 12 band_kernel
// instantiations and one or two instructions longer in 4 of them; expanded in place they compile to what each copy compiled to.
#define PYRAMID_EXPAND_ROWS(HP, Gm1, G0, Gp1, el, er, ec, orr, oc, x00, x01, x10, x11)      \
    do {                                                                                    \
        Px<2 * (HP)> evE, evO;                                                              \
        _Pragma("unroll") for (int k = 0; k < (HP); ++k) {                                  \
            v2f t = (Gm1).h[k] * 0.1f;                                                      \
            t = pfma((G0).h[k], 0.8f, t);                                                   \
            evE.h[k] = pfma((Gp1).h[k], 0.1f, t);                                           \
            evO.h[k] = pfma((Gp1).h[k], 0.5f, (G0).h[k] * 0.5f);                            \
        }                                                                                   \
        _Pragma("unroll") for (int k = 0; k < (HP); ++k) {                                  \
            (x00).h[k] = evE.h[k] * (ec);                                                   \
            (x01).h[k] = evE.h[k] * (oc);                                                   \
            dpp_expand_taps(evE.h[k], el, er, orr, (x00).h[k], (x01).h[k]);                 \
            (x10).h[k] = evO.h[k] * (ec);                                                   \
            (x11).h[k] = evO.h[k] * (oc);                                                   \
            dpp_expand_taps(evO.h[k], el, er, orr, (x10).h[k], (x11).h[k]);                 \
        }                                                                                   \
    } while (0)

// ---- masking and pooling in the log2 domain ----------------------------------------------------------------
// D = |T'-R'|^p / (1 + (k*min(|T'|,|R'|))^q), T' = T*S   (fvvdp.py:585-595).  Video (two temporal channels): the channels are
// carried as one (sustained, transient) pair through packed fp32 ops, only the transcendentals are per component, and
//   beta * log2 D = beta*p*(ldiff + S') - beta*log2(1 + 2^(q*(lmin + S''))),  S' = slog + lcn + lg_base, S'' = slog + lcn + lg_mask
// with the constant factors folded into fused multiply-adds (2 packed operations fewer per pixel than the literal form; it
// differs from it by the rounding of the products only).  d0, d1: the clamped contrast differences {test, reference} of the
// two channels.
// Statement macros for the reason given at PYRAMID_EXPAND_ROWS: as functions they left multigaze_kernel as it was and changed
// band_kernel<4, false, 0>, all of band2_kernel and 4 of the 10 multitest_kernel instantiations.
//
// The core.  A = beta * p * log2(S * m / lb), lsm = log2(k * S * m / lb), ldiff = log2 |T - R|, lmin = log2 min(|T|, |R|) per
// channel (v2f variables), vm = 1.0f where the pixel counts, else 0.0f.  Adds D^beta of both channels to acc[0], acc[1] and leaves
// min(beta * log2 D, beta * log2 d_max) in the v2f variable bl.
#define PYRAMID_MASK_POOL_PAIR(A, lsm, ldiff, lmin, pb, q0, q1, beta, b_dmax, vm, acc, bl)                                  \
    do {                                                                                                                    \
        const v2f ldb_ = pfma(ldiff, pb, A);                      /* beta * p * (log2|T'-R'|) */                             \
        const v2f lm_ = ((lmin) + (lsm)) * v2f{q0, q1};                                                                     \
        const v2f one_mq_ = v2f{fast_exp2(lm_.x), fast_exp2(lm_.y)} + splat(1.0f);                                          \
        const v2f tb_ = pfma(v2f{fast_log2(one_mq_.x), fast_log2(one_mq_.y)}, -(beta), ldb_);   /* beta * log2 D */         \
        bl = v2f{fminf(tb_.x, b_dmax), fminf(tb_.y, b_dmax)};                                   /* D <= d_max */            \
        const v2f term_ = v2f{fast_exp2((bl).x), fast_exp2((bl).y)};   /* D^beta for the spatial pooling (fvvdp.py:467,607) */ \
        const v2f av_ = __builtin_elementwise_fma(term_, splat(vm), v2f{(acc)[0], (acc)[1]});                               \
        (acc)[0] = av_.x;                                                                                                   \
        (acc)[1] = av_.y;                                                                                                   \
    } while (0)
// The same from the interpolated log sensitivities sl (a v2f variable), cA = fmaf(lcn, pb, pb_base), cL = lcn + lg_mask with
// lcn = log2(m / lb), and the clamped contrast differences d0, d1 ({test, reference} of the two channels).
#define PYRAMID_MASK_POOL_VIDEO(sl, cA, cL, d0, d1, pb, q0, q1, beta, b_dmax, vm, acc, bl)                                  \
    do {                                                                                                                    \
        const v2f A_ = pfma(sl, pb, splat(cA));                                                                             \
        const v2f lsm_ = (sl) + splat(cL);                                                                                  \
        const v2f ldiff_ = v2f{fast_log2(fabsf((d0).x - (d0).y)), fast_log2(fabsf((d1).x - (d1).y))};                       \
        const v2f lmin_ = v2f{fast_log2(fminf(fabsf((d0).x), fabsf((d0).y))), fast_log2(fminf(fabsf((d1).x), fabsf((d1).y)))}; \
        PYRAMID_MASK_POOL_PAIR(A_, lsm_, ldiff_, lmin_, pb, q0, q1, beta, b_dmax, vm, acc, bl);                             \
    } while (0)
// (The still-image tail, one channel, stays a copy in band_px, fov_b, band2_item and multigaze_item: band_item and band2_item
// leave its multiply-add to contraction and form log2 |T - R| first, multigaze_item spells the fmaf and forms the masking term
// first, and either order changed P = 2 code objects of the other side.)

// ---- the walk ----------------------------------------------------------------------------------------------
// Steps c = ca .. cb-1 of a chunk, unrolled over the 4 positions the 5-row window can take in the 8-slot ring (nothing is
// moved): step(integral_constant<int, phase>(), c) with the window in slots (4 + 2 * phase) & 7 ...  Wave-uniform trip count.
// A statement macro for the reason given at PYRAMID_EXPAND_ROWS: with the loop in a function that takes the step by reference or
// by value, 7 of the 12 band_kernel instantiations changed register names and operand order.
#define PYRAMID_WALK_STEPS(step, ca, cb)                     \
    for (int c = (ca); c < (cb); c += 4) {                   \
        step(std::integral_constant<int, 0>(), c);           \
        if (c + 1 >= (cb)) break;                            \
        step(std::integral_constant<int, 1>(), c + 1);       \
        if (c + 2 >= (cb)) break;                            \
        step(std::integral_constant<int, 2>(), c + 2);       \
        if (c + 3 >= (cb)) break;                            \
        step(std::integral_constant<int, 3>(), c + 3);       \
    }

// XCD-aware work order: hardware places workgroup b of nb on XCD b % 8 (speed only, never correctness).  Give each XCD a
// contiguous range of work items so that neighbouring strips, which share their halo columns, run on the same XCD at about the
// same time and hit in its L2.
// (b in the caller's own integer type: blockIdx.x itself, or a signed index into a phase of the grid)
template <class Index>
__device__ __forceinline__ int xcd_work_order(const Index b, const int nb) {
    const int q8 = nb >> 3, r8 = nb & 7, x = b & 7;
    return x * q8 + min(x, r8) + (b >> 3);
}
