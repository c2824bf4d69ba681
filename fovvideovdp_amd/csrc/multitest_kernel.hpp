// Stage 2 for many tests per reference: one fused pass per pyramid level over a GROUP of NQ quads (include/fvvdp_hip_tests.h).
// Included by fvvdp_hip.hip after band_kernel.hpp, whose building blocks (Px, row loads, DPP taps, BandArgs, the 1-D CSF table
// and its loader) it uses unchanged.
#pragma once
// ------------------------------------------------------------------------------------------------------------
// A quad is one float4 level plane: streams (x, z) and (y, w), each with its sustained and its transient channel
// (fvvdp_temporal_channels writes stream `d_test` into (x, z) and stream `d_ref` into (y, w)).  Quad 0 of a group is the
// reference's quad: the reference is its (y, w) stream.  The other NQ - 1 quads carry two tests each; quad 0's (x, z) stream is
// a test when the number of tests is odd (RX) and a second copy of the reference otherwise.
//
// The non-foveated pass (band_kernel<4, false, 0>) does, per band pixel, work of two kinds:
//   per stream:     row loads, reduce, expand, the coarse-level store, the contrast difference g - e and its upper clamp;
//   reference only: L_bkg and its clamp, cmax * L_bkg, log2(L_bkg), the look-up of the 1-D CSF table for both temporal
//                   channels, and every term of the log-domain tail that does not involve the test.
// multitest_kernel walks the level with band_item's own walk (pyramid_walk.hpp: weights, reduce, expand, step driver, the
// two-channel tail; same strips, chunks, lanes, row ring, single-wave workgroups) over
// the NQ quads at once and evaluates the reference-only part once per pixel; per test it runs that stream's contrast difference
// and the masking / pooling tail into the test's own acc[2].
//
// Bit identity with band_kernel<4, false, 0> on the pair (test, reference) is the contract (tests/test_gpu_multitest.py).  The
// reduce and the expand are component-wise (packed fp32 multiply-adds and single-register DPP taps), so a stream's level values
// do not depend on the stream it shares a quad with.  A test's accumulators see the same adds in the same order (pixels
// (2c, X0), (2c, X1), (2c+1, X0), (2c+1, X1) of every step), so its partial sums depend neither on NQ nor on its place in a quad
// nor on the other tests.  Every value is formed by the operations band_item forms it with: the functions below switch
// floating-point contraction off, and every fused multiply-add of band_px's non-foveated video tail is already spelled as one
// there (fmaf / pfma), so the same spelling here gives the same instructions ("Many tests per reference").
// The clamps are always kept: band2_kernel's clamp-free variant is bit-identical where it is taken.
// ------------------------------------------------------------------------------------------------------------
constexpr int MT_NQ_MAX = 3;
struct MultiTestArgs {
    BandArgs b;                     // the level as band_kernel<4, false, 0> takes it, F and Gc at frame slot 0; b.partial is not used
    int qslot[MT_NQ_MAX];           // first frame slot of quad j of the group (quad j, frame f of the batch: slot qslot[j] + f)
    int store[MT_NQ_MAX];           // 1: this launch writes quad j's coarse level; 0: it only reads the quad
    long long row[2 * MT_NQ_MAX];   // stream (quad j, component s: 0 = (x, z), 1 = (y, w)): float offset of its test's row in `partial`
    float* partial;                 // a row holds band_kernel's [n][n_strips * n_chunks][2] at the band's offset (added by the caller)
    // Geometry of the walk.  Lane l of strip s owns coarse column J = s * pitch - joff + l if own_lo <= l < own_hi (strip 0:
    // own_lo0); chunk c owns the coarse rows row_mul * [ka, kb) with ka, kb counted in rows of height k_lim: the first n_big
    // chunks hold kr such rows, the others kr2.  band_kernel's walk: {60, 0, 2, 62, 0; cr, n_chunks, cr, 1, hc}.  The two
    // other settings reproduce the partial sums of band2_kernel (band2_item) for the levels predict walks with it, see below.
    int pitch, joff, own_lo, own_hi, own_lo0;
    int kr, n_big, kr2, row_mul, k_lim;
};

// Levels that predict walks with the two-level kernel.  band2_item cuts levels A = b and B = b + 1 into strips of 54 level-B
// columns (lanes 6 .. 59 of a wave own them) and chunks of level-C rows [ka, kb); a partial sum is wave_sum over the lanes' own
// sequential sums.  Its per-pixel values are band_item's, so the sums are reproduced by walking the same pixels in the same
// order and adding the lanes in the same tree:
//   level A: a lane of band2_item owns level-B column J and level-A columns 2J, 2J+1 and adds (2c, X0), (2c, X1), (2c+1, X0),
//            (2c+1, X1) for c in [2 ka, min(2 kb, hb)) -- this kernel's walk with {54, 6, 6, 60, 6; kr, n_big, kr2, 2, hc of B};
//   level B: a lane of band2_item owns ONE level-B column and adds its rows top down; lanes 2m, 2m+1 are level-C column K.  Here
//            lane m owns K = 27 s - 3 + m with both columns, keeps a sum per column (SPLIT) and adds the lanes of each parity in
//            wave_sum's order over 32 lanes, then even + odd: wave_sum's last step.  Lanes 32 .. 63 of the wave own nothing.
//
// Group sizes NQ = 1, 2, 3.  Registers are the constraint: every quad adds its own 8-slot row ring (64 registers) and two coarse
// rows.  NQ <= 2 is compiled for two waves per SIMD (256 registers), NQ = 3 for one (the ring alone holds 192).  The table per
// NQ: DESIGN.md section 4, "Many tests per reference".
template <int NQ>
constexpr int mt_minw() { return NQ <= 2 ? 2 : 1; }

template <int NQ, bool RX, bool SPLIT>
__device__ __forceinline__ void multitest_item(const MultiTestArgs& ma, const int strip, const int chunk, const int frame,
                                               const int lane, const float4* s_csf) {
#pragma clang fp contract(off)
    const BandArgs& a = ma.b;
    constexpr int P = 4, HP = 2;
    constexpr int NT = 2 * (NQ - 1) + (RX ? 1 : 0);         // tests evaluated by this launch
    const int blk = chunk * a.n_strips + strip;
    const int w = a.w, h = a.h, wc = a.wc, hc = a.hc;
    const int J = strip * ma.pitch - ma.joff + lane;
    const bool big = chunk < ma.n_big;
    const int ka = big ? chunk * ma.kr : ma.n_big * ma.kr + (chunk - ma.n_big) * ma.kr2;
    const int kb = min(ka + (big ? ma.kr : ma.kr2), ma.k_lim);
    const int ca = ma.row_mul * ka;
    const int cb = min(ma.row_mul * kb, hc);
    const bool active = (lane >= (strip == 0 ? ma.own_lo0 : ma.own_lo)) && (lane < ma.own_hi) && (J >= 0) && (J < wc);
    const int X0 = 2 * J, X1 = 2 * J + 1;
    const int xc0 = min(max(X0, 0), w - 1), xc1 = min(max(X1, 0), w - 1);
    const bool col1_ok = X1 < w;

    // reduce / expand weights of this lane's column (pyramid_walk.hpp, as every pyramid kernel)
    const ReduceW rq = lane_reduce_weights(J, wc, w, h);
    const ExpandW ex = lane_expand_weights(J, wc);

    __amdgpu_buffer_rsrc_t Gf_rsrc[NQ], Gc_rsrc[NQ];
    bool may_store[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int slot = ma.qslot[j] + frame;
        const float* Gf = l0_frame(a.F, slot);
        float* Gc = a.Gc + (size_t)slot * hc * wc * P;
        Gc_rsrc[j] = level_rsrc(Gc, (unsigned int)(hc * wc * P) * 4u);
        Gf_rsrc[j] = level_rsrc(const_cast<float*>(Gf), (unsigned int)(h * w * P) * 4u);
        may_store[j] = active && ma.store[j] != 0;
    }
    const unsigned int col0_b = (unsigned int)xc0 * (P * 4u), col1_b = (unsigned int)xc1 * (P * 4u);
    const unsigned int row_b = (unsigned int)w * (P * 4u);

    Px<P> R[NQ][8][2];              // the 8-slot row ring of band_item, one per quad
    using std::integral_constant;
    auto load_row = [&](int r, auto SLOT) {
        constexpr int s = decltype(SLOT)::value;
        const unsigned int so = (unsigned int)reflect_row(r, h) * row_b;      // one row offset for all quads
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            R[j][s][0] = ld_px_buf<P>(Gf_rsrc[j], col0_b, so);
            R[j][s][1] = ld_px_buf<P>(Gf_rsrc[j], col1_b, so);
        }
    };
    auto coarse_step = [&](const int j, auto S0) -> Px<P> {
        return reduce5_ring<P, decltype(S0)::value>(R[j], rq.q0, rq.q1, rq.q2, rq.q3, rq.q4);
    };

    // ---- prologue: coarse rows ca-1 and ca of every quad
    {
        const int r0 = 2 * (ca - 1) - 2;
        load_row(r0 + 0, integral_constant<int, 0>());
        load_row(r0 + 1, integral_constant<int, 1>());
        load_row(r0 + 2, integral_constant<int, 2>());
        load_row(r0 + 3, integral_constant<int, 3>());
        load_row(r0 + 4, integral_constant<int, 4>());
    }
    Px<P> Gm1[NQ], G0[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) Gm1[j] = coarse_step(j, integral_constant<int, 0>());
    load_row(2 * ca + 1, integral_constant<int, 5>());
    load_row(2 * ca + 2, integral_constant<int, 6>());
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const Px<P> cB = coarse_step(j, integral_constant<int, 2>());
        st_px(Gc_rsrc[j], may_store[j] ? (unsigned int)(ca * wc + J) * (P * 4u) : FVVDP_NO_STORE, cB);
        if (!(ca > 0)) Gm1[j] = cB;
        G0[j] = cB;
    }
    load_row(2 * ca + 3, integral_constant<int, 7>());
    load_row(2 * ca + 4, integral_constant<int, 0>());

    constexpr int NC = SPLIT ? 2 : 1;                       // SPLIT: one pair of sums per fine column of the lane
    float acc[NT > 0 ? NT : 1][NC][2];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            acc[t][cc][0] = 0.0f;
            acc[t][cc][1] = 0.0f;
        }
    }

    const float lg_bm = __log2f(a.band_mul);
    const float lg_base = a.lg_gain;
    const float lg_mask = a.lg_gain + a.lg_k;
    const float pb = a.p * a.beta, pb_base = lg_base * pb, b_dmax = a.beta * a.lg_dmax;
    const float y_off = -a.y_first * a.y_inv_step;

    // reference-only head of a band pixel (band_px, the part that reads component y of the reference's quad only)
    struct Head {
        float dcap;
        v2f dR;                     // the reference's clamped contrast difference per temporal channel
        v2f A, lsm;                 // beta * p * log2(S * m / lb), log2(k * S * m / lb)
    };
    auto head = [&](const Px<P>& g, const Px<P>& e) -> Head {
        Head q;
        const float lb = fmaxf(e.h[0].y, a.lbkg_min);
        q.dcap = a.cmax * lb;
        q.dR = v2f{fminf(g.h[0].y - e.h[0].y, q.dcap), fminf(g.h[1].y - e.h[1].y, q.dcap)};
        const float llb = fast_log2(lb);
        const float yq = __builtin_amdgcn_fmed3f(llb, a.ly_lo, a.ly_hi);
        const float t = fmaf(yq, a.y_inv_step, y_off);
        const float fi = __builtin_amdgcn_fmed3f(floorf(t), 0.0f, (float)(FVVDP_LUT_N - 2));
        const float4 r = s_csf[(int)fi];
        const float f = t - fi;
        const v2f sl = v2f{fmaf(f, r.z, r.x), fmaf(f, r.w, r.y)};
        const float lcn = lg_bm - llb;
        q.A = pfma(sl, pb, splat(fmaf(lcn, pb, pb_base)));
        q.lsm = sl + splat(lcn + lg_mask);
        return q;
    };
    // per test: the stream's contrast difference and the log-domain masking tail of band_px into the test's accumulators
    auto tail = [&](const Head& q, float g0, float e0, float g1, float e1, bool valid, float (&ac)[2]) {
        const v2f dT = v2f{fminf(g0 - e0, q.dcap), fminf(g1 - e1, q.dcap)};
        const v2f ldiff = v2f{fast_log2(fabsf(dT.x - q.dR.x)), fast_log2(fabsf(dT.y - q.dR.y))};
        const v2f lmin = v2f{fast_log2(fminf(fabsf(dT.x), fabsf(q.dR.x))), fast_log2(fminf(fabsf(dT.y), fabsf(q.dR.y)))};
        const float vm = valid ? 1.0f : 0.0f;
        v2f bl;
        PYRAMID_MASK_POOL_PAIR(q.A, q.lsm, ldiff, lmin, pb, a.q0, a.q1, a.beta, b_dmax, vm, ac, bl);
    };
    // one band pixel of every quad: g[j] the level value, e[j] the expanded coarse level
    auto band_px = [&](const Px<P> (&g)[NQ], const Px<P> (&e)[NQ], bool valid, auto COL) {
        constexpr int cc = SPLIT ? decltype(COL)::value : 0;
        const Head q = head(g[0], e[0]);
        if constexpr (RX) tail(q, g[0].h[0].x, e[0].h[0].x, g[0].h[1].x, e[0].h[1].x, valid, acc[0][cc]);
#pragma unroll
        for (int j = 1; j < NQ; ++j) {
            constexpr int t0 = RX ? 1 : 0;
            tail(q, g[j].h[0].x, e[j].h[0].x, g[j].h[1].x, e[j].h[1].x, valid, acc[t0 + 2 * (j - 1)][cc]);
            tail(q, g[j].h[0].y, e[j].h[0].y, g[j].h[1].y, e[j].h[1].y, valid, acc[t0 + 2 * (j - 1) + 1][cc]);
        }
    };

    // ---- main loop: band rows 2c, 2c+1 for c in [ca, cb)
    auto step = [&](auto PH, const int c) {
        constexpr int s0 = (4 + 2 * decltype(PH)::value) & 7;
        load_row(2 * c + 5, integral_constant<int, (s0 + 5) & 7>());
        load_row(2 * c + 6, integral_constant<int, (s0 + 6) & 7>());
        const bool has_next = (c + 1) <= (hc - 1);
        Px<P> x00[NQ], x01[NQ], x10[NQ], x11[NQ], Gp1[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const Px<P> cN = coarse_step(j, integral_constant<int, s0>());
            Gp1[j] = has_next ? cN : G0[j];
            st_px(Gc_rsrc[j], (has_next && (c + 1) < cb && may_store[j]) ? (unsigned int)((c + 1) * wc + J) * (P * 4u) : FVVDP_NO_STORE, cN);
            PYRAMID_EXPAND_ROWS(HP, Gm1[j], G0[j], Gp1[j], ex.el, ex.er, ex.ec, ex.orr, ex.oc, x00[j], x01[j], x10[j], x11[j]);
        }
        const bool row1_ok = (2 * c + 1) < h;
        Px<P> w00[NQ], w01[NQ], w10[NQ], w11[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            w00[j] = R[j][s0][0];
            w01[j] = R[j][s0][1];
            w10[j] = R[j][(s0 + 1) & 7][0];
            w11[j] = R[j][(s0 + 1) & 7][1];
        }
        band_px(w00, x00, active, integral_constant<int, 0>());
        band_px(w01, x01, active && col1_ok, integral_constant<int, 1>());
        band_px(w10, x10, active && row1_ok, integral_constant<int, 0>());
        band_px(w11, x11, active && row1_ok && col1_ok, integral_constant<int, 1>());
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            Gm1[j] = G0[j];
            G0[j] = Gp1[j];
        }
    };
    PYRAMID_WALK_STEPS(step, ca, cb);

    // the partial sums of every test into its own row, where band_kernel puts them
    const size_t o_blk = ((size_t)frame * (a.n_strips * a.n_chunks) + blk) * 2;
    auto half_sum = [&](float v) {                          // wave_sum's tree over lanes 0 .. 31
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        return v;
    };
    auto put = [&](const float (&ac)[NC][2], long long row) {
        float s0, s1;
        if constexpr (SPLIT) {
            s0 = half_sum(ac[0][0]) + half_sum(ac[1][0]);
            s1 = half_sum(ac[0][1]) + half_sum(ac[1][1]);
        } else {
            s0 = wave_sum(ac[0][0]);
            s1 = wave_sum(ac[0][1]);
        }
        if (lane == 0) {
            float* o = ma.partial + row + o_blk;
            o[0] = s0;
            o[1] = s1;
        }
    };
    if constexpr (RX) put(acc[0], ma.row[0]);
#pragma unroll
    for (int j = 1; j < NQ; ++j) {
        constexpr int t0 = RX ? 1 : 0;
        put(acc[t0 + 2 * (j - 1)], ma.row[2 * j]);
        put(acc[t0 + 2 * (j - 1) + 1], ma.row[2 * j + 1]);
    }
}

template <int NQ, bool RX, bool SPLIT>
__global__ __launch_bounds__(64, mt_minw<NQ>()) void multitest_kernel(const MultiTestArgs a_byval) {
    const MultiTestArgs& ma = *(const MultiTestArgs*)__builtin_amdgcn_kernarg_segment_ptr();     // see band_kernel
    (void)a_byval;
    const BandArgs& a = ma.b;
    __shared__ float4 s_csf[FVVDP_LUT_N];
    const int lane = (int)threadIdx.x;
    int bid;
    {
        bid = xcd_work_order(blockIdx.x, (int)gridDim.x);
    }
    const int strip = bid % a.n_strips;
    bid /= a.n_strips;
    const int chunk = bid % a.n_chunks;
    const int frame = bid / a.n_chunks;
    band_load_tables<0>(a, s_csf, nullptr, (int)threadIdx.x, 64);
    __syncthreads();
    multitest_item<NQ, RX, SPLIT>(ma, strip, chunk, frame, lane, s_csf);
}
