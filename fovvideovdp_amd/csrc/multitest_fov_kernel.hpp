// Stage 2 for many tests per reference under a gaze: one fused foveated pass per pyramid level over a GROUP of NQ quads
// (include/fvvdp_hip_tests_fov.h).  Included by fvvdp_hip.hip after band_kernel.hpp and multitest_kernel.hpp: the building blocks
// of the first (Px, row loads, DPP taps, BandArgs, the LDS tables, their layout and their loader) and the quad conventions of the
// second are used unchanged.
#pragma once
// ------------------------------------------------------------------------------------------------------------
// Quads as in multitest_kernel.hpp: quad 0 of a group is the reference's quad, the reference its (y, w) stream; the other NQ - 1
// quads carry two tests each; quad 0's (x, z) stream is a test when the number of tests is odd (RX).
//
// The stock-geometry foveated pass (band_kernel<4, false, 1>) does, per band pixel, work of two kinds:
//   per stream:             row loads, reduce, expand, the coarse-level store, the contrast difference g - e and its upper clamp;
//   reference and gaze only: L_bkg and its clamp, cmax * L_bkg, log2(L_bkg), the Y axis of the CSF query, the eccentricity and its
//                           axis, the rho-map record, the four cells of the LUT slice, interp3 of both temporal channels, and
//                           every term of the log-domain tail that does not involve the test.
// multitest_fov_kernel walks the level with band_item's one-level walk (pyramid_walk.hpp; same strips, chunks, lanes 2 .. 61,
// 8-slot row ring, FOV_WPB waves per workgroup, LUT slice and row table in dynamic LDS, rho-map records requested before the row
// prefetch, two pixels per phase) over the NQ quads at once and evaluates the second kind once per pixel (the head); per test it
// runs that stream's contrast difference, the four logarithms and the masking / pooling tail into the test's own acc[2].  The
// foveated pass never takes the two-level walk, so none of multitest_kernel's walk geometry is needed.
//
// Bit identity with band_kernel<4, false, 1> on the pair (test, reference) is the contract (tests/test_gpu_tests_fov.py).  The
// reduce and the expand are component-wise, so a stream's level values do not depend on the stream it shares a quad with; a
// test's accumulators see the same adds in the same order (pixels (2c, X0), (2c, X1), (2c+1, X0), (2c+1, X1) of every step).
// Every value is formed by the operations band_item forms it with: contraction is off here, and the two products that band_item's
// code fuses into a following sum are spelled as multigaze_kernel.hpp found them,
//   ecc^2 = fma(dy, dy, dx^2)            dx = fma(atan(.), 57.29..., -gx)
// everything else of fov_a / fov_b and of the two-channel tail is an explicit fmaf / pfma there already.
// ------------------------------------------------------------------------------------------------------------
struct MultiTestFovArgs {
    BandArgs b;                     // the level as band_kernel<4, false, 1> takes it (b.fix: gaze of frame f of the batch), F and Gc at
                                    // frame slot 0; b.partial is not used
    int qslot[MT_NQ_MAX];           // first frame slot of quad j of the group (quad j, frame f of the batch: slot qslot[j] + f)
    int store[MT_NQ_MAX];           // 1: this launch writes quad j's coarse level; 0: it only reads the quad
    long long row[2 * MT_NQ_MAX];   // stream (quad j, component s: 0 = (x, z), 1 = (y, w)): float offset of its test's row in `partial`
    float* partial;                 // a row holds band_kernel's [n][n_strips * n_chunks][2] at the band's offset (added by the caller)
};

// Group sizes NQ = 1 (RX only), 2, 3.  Every quad adds its own 8-slot row ring (64 registers) and two coarse rows; the head keeps
// the four cells of two pixels in flight.  NQ <= 2 is compiled for two waves per SIMD (256 registers), NQ = 3 for one.  The
// register table: DESIGN.md section 4, "Many tests per reference under a gaze".
template <int NQ>
constexpr int mtf_minw() { return NQ <= 2 ? 2 : 1; }
// pixels whose LUT cells are in flight at once: two (band_item's phases), except where that does not fit two waves per SIMD
template <int NQ, bool RX>
constexpr bool MTF_PAIRED = !(NQ == 2 && RX);

template <int NQ, bool RX>
__device__ __forceinline__ void multitest_fov_item(const MultiTestFovArgs& ma, const int strip, const int chunk, const int frame,
                                                   const int lane) {
#pragma clang fp contract(off)
    const BandArgs& a = ma.b;
    constexpr int P = 4, HP = 2;
    constexpr int NT = 2 * (NQ - 1) + (RX ? 1 : 0);         // tests evaluated by this launch
    const int blk = chunk * a.n_strips + strip;
    const int w = a.w, h = a.h, wc = a.wc, hc = a.hc;
    const int J = strip * STRIP_J + lane;
    const int ca = chunk * a.cr;
    const int cb = min(ca + a.cr, hc);
    const bool active = (lane >= 2 || strip == 0) && (lane < 62) && (J < wc);
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

    float acc[NT][2];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        acc[t][0] = 0.0f;
        acc[t][1] = 0.0f;
    }

    // ---- the gaze of this frame: its vertical view angle and the column terms of the squared eccentricity (band_item)
    float gy, dxa2, dxb2;
    {
        const float xa = ((float)X0 + 0.5f) + (-(float)w / 2.0f);
        const float xb = ((float)X1 + 0.5f) + (-(float)w / 2.0f);
        const float kx = a.size_m0 / (float)w / a.dist_m;
        const float ata = atanf(xa * kx), atb = atanf(xb * kx);
        const float fxp = a.fix[2 * frame + 0] + 0.5f, fyp = a.fix[2 * frame + 1] + 0.5f;
        const float gxm = (fxp + (-(float)a.frame_w / 2.0f)) * a.size_m0 / (float)a.frame_w;
        const float gym = -(fyp + (-(float)a.frame_h / 2.0f)) * a.size_m1 / (float)a.frame_h;
        const float gx = atanf(gxm / a.dist_m) * 57.29577951308232f;
        gy = atanf(gym / a.dist_m) * 57.29577951308232f;
        // band_item: vxa = atanf(.) * 57.29...; dxa = vxa - gx, compiled as one fused multiply-add
        const float dxa = fmaf(ata, 57.29577951308232f, -gx), dxb = fmaf(atb, 57.29577951308232f, -gx);
        dxa2 = dxa * dxa;
        dxb2 = dxb * dxb;
    }

    const float lg_bm = __log2f(a.band_mul);
    const float lg_base = a.lg_gain;
    const float lg_mask = a.lg_gain + a.lg_k;
    const float pb = a.p * a.beta, pb_base = lg_base * pb, b_dmax = a.beta * a.lg_dmax;

    // The head of a band pixel, first half (fov_a on component y of the reference's quad): the reference's contrast differences,
    // log2(L_bkg), the Y and eccentricity axes of the query and the four cells of the LUT slice, requested and not yet used.
    struct HeadA {
        float dcap;
        v2f dR;                     // the reference's clamped contrast difference per temporal channel
        float fY, fE, fR;
        float cA, cL;               // fmaf(lcn, pb, pb_base), lcn + lg_mask with lcn = log2(m / lb)
        float4 v00, v10, v01, v11;
    };
    auto head_a = [&](const Px<P>& g, const Px<P>& e, float dx2, float dy, float pre_fR, float pre_kR) -> HeadA {
        HeadA q;
        const float lb = fmaxf(e.h[0].y, a.lbkg_min);
        q.dcap = a.cmax * lb;
        q.dR = v2f{fminf(g.h[0].y - e.h[0].y, q.dcap), fminf(g.h[1].y - e.h[1].y, q.dcap)};
        const float llb = fast_log2(lb);
        const float yq = __builtin_amdgcn_fmed3f(llb, a.ly_lo, a.ly_hi);
        const float ecc = __builtin_amdgcn_sqrtf(fmaf(dy, dy, dx2));      // band_item: dx2 + dy * dy, fused
        const float eq = __builtin_amdgcn_sqrtf(__builtin_amdgcn_fmed3f(ecc, a.ecc_lo, a.ecc_hi));
        const float tY = fmaf(yq, a.inv_step[0], a.grid_off[0]);
        const float iY = __builtin_amdgcn_fmed3f(floorf(tY), 0.0f, (float)(FVVDP_LUT_N - 2));
        q.fY = (tY - iY) * a.frac_scale[0];
        const float tE = fmaf(eq, a.inv_step[2], a.grid_off[2]);
        const float iE = __builtin_amdgcn_fmed3f(floorf(tE), 0.0f, (float)(FVVDP_LUT_N - 2));
        q.fE = (tE - iE) * a.frac_scale[2];
        const int bo = (int)fmaf(iE, (float)(FOV_ROW * 16), fmaf(iY, 16.0f, pre_kR));
        q.fR = pre_fR;
        const float4* cell = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_lut_dyn) + bo);
        constexpr int sj = 1, sk = FOV_ROW;
        q.v00 = cell[0];
        q.v10 = cell[sj];
        q.v01 = cell[sk];
        q.v11 = cell[sk + sj];
        const float lcn = lg_bm - llb;
        q.cA = fmaf(lcn, pb, pb_base);
        q.cL = lcn + lg_mask;
        return q;
    };
    // The head, second half (fov_b up to the sensitivities): interp3 of both temporal channels in slope form (rho, then Y, then
    // ecc) and the two per-pixel terms the masking tail takes from them.
    struct HeadB {
        float dcap;
        v2f dR;
        v2f A, lsm;                 // beta * p * log2(S * m / lb), log2(k * S * m / lb)
    };
    auto head_b = [&](const HeadA& q) -> HeadB {
        HeadB r;
        const float fY = q.fY, fE = q.fE, fR = q.fR;
        auto rho_blend = [&](const float4& v) { return pfma(v2f{v.z, v.w}, fR, v2f{v.x, v.y}); };
        const v2f r00 = rho_blend(q.v00), r10 = rho_blend(q.v10), r01 = rho_blend(q.v01), r11 = rho_blend(q.v11);
        const v2f y0 = pfma(r10 - r00, fY, r00), y1 = pfma(r11 - r01, fY, r01);
        const v2f sl = pfma(y1 - y0, fE, y0);
        r.dcap = q.dcap;
        r.dR = q.dR;
        r.A = pfma(sl, pb, splat(q.cA));
        r.lsm = sl + splat(q.cL);
        return r;
    };
    // per test: the stream's contrast difference, the four logarithms and the log-domain masking tail into the test's accumulators
    auto tail = [&](const HeadB& q, float g0, float e0, float g1, float e1, bool valid, float (&ac)[2]) {
        const v2f dT = v2f{fminf(g0 - e0, q.dcap), fminf(g1 - e1, q.dcap)};
        const v2f ldiff = v2f{fast_log2(fabsf(dT.x - q.dR.x)), fast_log2(fabsf(dT.y - q.dR.y))};
        const v2f lmin = v2f{fast_log2(fminf(fabsf(dT.x), fabsf(q.dR.x))), fast_log2(fminf(fabsf(dT.y), fabsf(q.dR.y)))};
        const float vm = valid ? 1.0f : 0.0f;
        v2f bl;
        PYRAMID_MASK_POOL_PAIR(q.A, q.lsm, ldiff, lmin, pb, a.q0, a.q1, a.beta, b_dmax, vm, ac, bl);
    };
    // every test of the group at one band pixel: g[j] the level value, e[j] the expanded coarse level of quad j
    auto tails = [&](const HeadB& q, const Px<P> (&g)[NQ], const Px<P> (&e)[NQ], bool valid) {
        if constexpr (RX) tail(q, g[0].h[0].x, e[0].h[0].x, g[0].h[1].x, e[0].h[1].x, valid, acc[0]);
#pragma unroll
        for (int j = 1; j < NQ; ++j) {
            constexpr int t0 = RX ? 1 : 0;
            tail(q, g[j].h[0].x, e[j].h[0].x, g[j].h[1].x, e[j].h[1].x, valid, acc[t0 + 2 * (j - 1)]);
            tail(q, g[j].h[0].y, e[j].h[0].y, g[j].h[1].y, e[j].h[1].y, valid, acc[t0 + 2 * (j - 1) + 1]);
        }
    };

    // ---- main loop: band rows 2c, 2c+1 for c in [ca, cb)
    auto step = [&](auto PH, const int c) {
        constexpr int s0 = (4 + 2 * decltype(PH)::value) & 7;
        const int jj = min(max(J, 0), a.rmap_w - 1);
        const float4 ra = a.rmap[(size_t)min(2 * c, h - 1) * a.rmap_w + jj];        // rho-map records first, then the row prefetch
        const float4 rb = a.rmap[(size_t)min(2 * c + 1, h - 1) * a.rmap_w + jj];
        __builtin_amdgcn_sched_barrier(0);
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
        const float* s_vy = reinterpret_cast<const float*>(s_lut_dyn + FOV_PLANE * a.rw);
        const float vy0 = s_vy[2 * c];
        const float vy1 = s_vy[min(2 * c + 1, h - 1)];
        Px<P> w00[NQ], w01[NQ], w10[NQ], w11[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            w00[j] = R[j][s0][0];
            w01[j] = R[j][s0][1];
            w10[j] = R[j][(s0 + 1) & 7][0];
            w11[j] = R[j][(s0 + 1) & 7][1];
        }
        // Two pixels per phase, as band_item: the cells of both requested back to back, then per pixel the blends and every test.
        // <2, true> keeps one pixel's cells in flight instead: with both it needs 9 registers more than two waves per SIMD leave.
        auto phase = [&](const Px<P> (&ga)[NQ], const Px<P> (&ea)[NQ], const Px<P> (&gb)[NQ], const Px<P> (&eb)[NQ], const float vy,
                         const float4 r, const bool va, const bool vb) {
            const float dy = vy - gy;
            if constexpr (MTF_PAIRED<NQ, RX>) {
                const HeadA qa = head_a(ga[0], ea[0], dxa2, dy, r.x, r.y);
                const HeadA qb = head_a(gb[0], eb[0], dxb2, dy, r.z, r.w);
                tails(head_b(qa), ga, ea, va);
                tails(head_b(qb), gb, eb, vb);
            } else {
                tails(head_b(head_a(ga[0], ea[0], dxa2, dy, r.x, r.y)), ga, ea, va);
                __builtin_amdgcn_sched_barrier(0);
                tails(head_b(head_a(gb[0], eb[0], dxb2, dy, r.z, r.w)), gb, eb, vb);
            }
        };
        __builtin_amdgcn_sched_barrier(0);
        phase(w00, x00, w01, x01, vy0, ra, active, active && col1_ok);
        __builtin_amdgcn_sched_barrier(0);
        phase(w10, x10, w11, x11, vy1, rb, active && row1_ok, active && row1_ok && col1_ok);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            Gm1[j] = G0[j];
            G0[j] = Gp1[j];
        }
    };
    PYRAMID_WALK_STEPS(step, ca, cb);

    // the partial sums of every test into its own row, where band_kernel puts them
    const size_t o_blk = ((size_t)frame * (a.n_strips * a.n_chunks) + blk) * 2;
    auto put = [&](const float (&ac)[2], long long row) {
        const float s0 = wave_sum(ac[0]);
        const float s1 = wave_sum(ac[1]);
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

template <int NQ, bool RX>
__global__ __launch_bounds__(64 * FOV_WPB, mtf_minw<NQ>()) void multitest_fov_kernel(const MultiTestFovArgs a_byval) {
    const MultiTestFovArgs& ma = *(const MultiTestFovArgs*)__builtin_amdgcn_kernarg_segment_ptr();     // see band_kernel
    (void)a_byval;
    static_assert(NQ >= 1 && NQ <= MT_NQ_MAX && (NQ > 1 || RX), "a group evaluates at least one test");
    const BandArgs& a = ma.b;
    __shared__ float2 s_ax[3 * FVVDP_LUT_N];
    const int lane = (int)(threadIdx.x & 63);
    int bid;
    {
        bid = xcd_work_order(blockIdx.x, (int)gridDim.x);
        bid = bid * FOV_WPB + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    }
    const bool wave_has_work = bid < a.n_items;
    const int n_tiles = a.n_strips * a.n_chunks, n_frames = a.n_items / n_tiles;     // frame fastest, as band_kernel<P, DBG, 1>
    const int frame = bid % n_frames;
    bid /= n_frames;
    const int strip = bid % a.n_strips;
    const int chunk = bid / a.n_strips;
    band_load_tables<1>(a, nullptr, s_ax, (int)threadIdx.x, 64 * FOV_WPB);
    __syncthreads();
    if (!wave_has_work) return;
    multitest_fov_item<NQ, RX>(ma, strip, chunk, frame, lane);
}
