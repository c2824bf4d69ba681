// Stage 2 under many gazes: one fused pass per pyramid level for a GROUP of NG gaze traces (include/fvvdp_hip_gaze.h).
// Included by fvvdp_hip.hip after band_kernel.hpp, whose building blocks (Px, row loads, DPP taps, the LDS tables and their
// layout, BandArgs) it uses unchanged.
#pragma once
// ------------------------------------------------------------------------------------------------------------
// The stock-geometry foveated pass (band_kernel<P, false, 1>) does, per band pixel, work of two kinds:
//   gaze-invariant: row loads, reduce, expand, the coarse-level store, the contrast differences and their clamp, log2(L_bkg),
//                   the Y axis of the CSF query, the rho-map record, the logs of |T - R| and min(|T|, |R|);
//   per gaze:       eccentricity -> ecc axis of the query -> the four cells of the LUT slice -> interp3 -> the masking tail.
// multigaze_kernel walks the level with band_item's own walk (pyramid_walk.hpp: weights, row loads, reduce, expand, step driver;
// same strips, chunks, lanes, row ring, LDS tables, FOV_WPB waves per workgroup) and evaluates the first kind once, the second once per gaze g of the group into that gaze's acc[g][2].
//
// Bit identity with band_kernel<P, false, 1> run once per gaze is the contract (tests/test_gpu_gazes.py).  A gaze's
// accumulators see the same adds in the same order (pixels (2c, X0), (2c, X1), (2c+1, X0), (2c+1, X1) of every step), so its
// partial sums depend neither on NG nor on its slot nor on the other gazes.  Every value is formed by the operations band_item
// forms it with; hoisting a pure sub-expression out of the gaze loop changes no value, a different choice of the compiler
// between a multiply-add and a separate product and sum would.  The functions below therefore switch floating-point
// contraction off and spell each fused multiply-add that the existing kernel's code has as an explicit fma:
//   ecc^2 = fma(dy, dy, dx^2)            (the row term's product is fused into the sum with the column term)
//   dx    = fma(atan(.), 57.29..., -gx)  (view angle of the lane's column minus the gaze angle)
//   P = 2: fma(p, log2|T - R| + ..., -log2(1 + mq))  (the still-image tail)
// as read off the disassembly of band_kernel<4, false, 1> / band_kernel<2, false, 1> ("Many gazes per
// clip").
// ------------------------------------------------------------------------------------------------------------
struct MultiGazeArgs {
    BandArgs b;                 // the level as band_kernel<P, false, 1> takes it; b.fix and b.partial are not used
    const float* gaze;          // gaze of (group slot g, frame f of the batch) at gaze[g * gaze_stride + 2 * f]: (x, y) in frame pixels
    long long gaze_stride;
    float* partial;             // group slot g: partial + g * partial_stride, then band_kernel's [n][n_strips * n_chunks][2]
    long long partial_stride;
    int store_coarse;           // 1: this launch writes the coarse level (the first group of a level); 0: it only reads
};

// Group sizes NG = 1, 2, 4, 8 (FVVDP_GAZE_GROUP_MAX = 8; G gazes are served by the largest groups that fit, 8, 4, 2, 1).
// Registers are the constraint: every gaze adds two accumulators, its vertical view angle and two column terms, and the tails
// of a phase's two pixels are in flight per gaze.  VGPRs of the code objects (P = 4 / P = 2; no spills, no scratch):
//   NG = 1: 154 / 111   NG = 2: 168 / 125   NG = 4: 190 / 141   NG = 8: 234 / 172
// The lean single-gaze kernel holds 168 for 3 waves per SIMD; NG = 4 and 8 need more than 170, so the kernel is compiled for 2
// waves per SIMD (256 VGPRs) throughout: from NG = 4 on the occupancy is 2 whatever the group, and the larger group shares the
// gaze-invariant work among more gazes.  Measurements and the choice: DESIGN.md section 4, "Many gazes per clip".
constexpr int MG_MINW = 2;

template <int P, int NG>
__device__ __forceinline__ void multigaze_item(const MultiGazeArgs& ga, const int strip, const int chunk, const int frame,
                                               const int lane) {
#pragma clang fp contract(off)
    const BandArgs& a = ga.b;
    constexpr int HP = P / 2;
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

    const float* Gf = l0_frame(a.F, frame);
    float* Gc = a.Gc + (size_t)frame * hc * wc * P;
    const __amdgpu_buffer_rsrc_t Gc_rsrc = level_rsrc(Gc, (unsigned int)(hc * wc * P) * 4u);
    const __amdgpu_buffer_rsrc_t Gf_rsrc = level_rsrc(const_cast<float*>(Gf), (unsigned int)(h * w * P) * 4u);
    const unsigned int col0_b = (unsigned int)xc0 * (P * 4u), col1_b = (unsigned int)xc1 * (P * 4u);
    const unsigned int row_b = (unsigned int)w * (P * 4u);
    const bool may_store = active && ga.store_coarse != 0;
    auto load_row = [&](int r, Px<P>& p0, Px<P>& p1) { load_row_pair<P>(Gf_rsrc, col0_b, col1_b, row_b, h, r, p0, p1); };

    Px<P> R[8][2];                  // the 8-slot row ring (see band_item)
    using std::integral_constant;
    auto coarse_step = [&](auto S0) -> Px<P> {
        return reduce5_ring<P, decltype(S0)::value>(R, rq.q0, rq.q1, rq.q2, rq.q3, rq.q4);
    };

    // ---- prologue: coarse rows ca-1 and ca
    {
        const int r0 = 2 * (ca - 1) - 2;
#pragma unroll
        for (int k = 0; k < 5; ++k) load_row(r0 + k, R[k][0], R[k][1]);
    }
    const Px<P> cA = coarse_step(integral_constant<int, 0>());
    load_row(2 * ca + 1, R[5][0], R[5][1]);
    load_row(2 * ca + 2, R[6][0], R[6][1]);
    const Px<P> cB = coarse_step(integral_constant<int, 2>());
    st_px(Gc_rsrc, may_store ? (unsigned int)(ca * wc + J) * (P * 4u) : FVVDP_NO_STORE, cB);
    Px<P> Gm1 = (ca > 0) ? cA : cB;
    Px<P> G0 = cB;
    load_row(2 * ca + 3, R[7][0], R[7][1]);
    load_row(2 * ca + 4, R[0][0], R[0][1]);

    // ---- per gaze: accumulators, the gaze's vertical view angle and the column terms of the squared eccentricity
    float acc[NG][2];
    float gyv[NG], dxa2[NG], dxb2[NG];
    {
        const float xa = ((float)X0 + 0.5f) + (-(float)w / 2.0f);
        const float xb = ((float)X1 + 0.5f) + (-(float)w / 2.0f);
        const float kx = a.size_m0 / (float)w / a.dist_m;
        const float ata = atanf(xa * kx), atb = atanf(xb * kx);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float* fx = ga.gaze + (size_t)g * ga.gaze_stride + 2 * frame;
            const float fxp = fx[0] + 0.5f, fyp = fx[1] + 0.5f;
            const float gxm = (fxp + (-(float)a.frame_w / 2.0f)) * a.size_m0 / (float)a.frame_w;
            const float gym = -(fyp + (-(float)a.frame_h / 2.0f)) * a.size_m1 / (float)a.frame_h;
            const float gx = atanf(gxm / a.dist_m) * 57.29577951308232f;
            gyv[g] = atanf(gym / a.dist_m) * 57.29577951308232f;
            // band_item: vxa = atanf(.) * 57.29...; dxa = vxa - gx, compiled as one fused multiply-add
            const float dxa = fmaf(ata, 57.29577951308232f, -gx), dxb = fmaf(atb, 57.29577951308232f, -gx);
            dxa2[g] = dxa * dxa;
            dxb2[g] = dxb * dxb;
            acc[g][0] = 0.0f;
            acc[g][1] = 0.0f;
        }
    }

    const float lg_bm = __log2f(a.band_mul);
    const float lg_base = a.lg_gain;
    const float lg_mask = a.lg_gain + a.lg_k;
    const float pb = a.p * a.beta, pb_base = lg_base * pb, b_dmax = a.beta * a.lg_dmax;

    // gaze-invariant head of a band pixel: fov_a's contrast differences, log2(L_bkg), the Y axis of the query, and from fov_b
    // what does not involve the sensitivity
    struct Head {
        float fY, fR, boY;      // boY = byte offset of (rho plane, Y interval) in the LUT slice, as a float (fov_a's inner fmaf)
        float lcn;              // log2(m / lb)
        float cA, cL;           // HP == 2: fmaf(lcn, pb, pb_base), lcn + lg_mask
        float ldiff[HP], lmin[HP];   // log2 |T - R|, log2 min(|T|, |R|) per temporal channel
    };
    auto head = [&](const Px<P>& g, const Px<P>& e, float pre_fR, float pre_kR) -> Head {
        Head q;
        const float lb = fmaxf(e.h[0].y, a.lbkg_min);
        const float dcap = a.cmax * lb;
        v2f d[HP];
#pragma unroll
        for (int k = 0; k < HP; ++k) d[k] = v2f{fminf(g.h[k].x - e.h[k].x, dcap), fminf(g.h[k].y - e.h[k].y, dcap)};
        const float llb = fast_log2(lb);
        const float yq = __builtin_amdgcn_fmed3f(llb, a.ly_lo, a.ly_hi);
        const float tY = fmaf(yq, a.inv_step[0], a.grid_off[0]);
        const float iY = __builtin_amdgcn_fmed3f(floorf(tY), 0.0f, (float)(FVVDP_LUT_N - 2));
        q.fY = (tY - iY) * a.frac_scale[0];
        q.boY = fmaf(iY, 16.0f, pre_kR);
        q.fR = pre_fR;
        q.lcn = lg_bm - llb;
        q.cA = fmaf(q.lcn, pb, pb_base);
        q.cL = q.lcn + lg_mask;
#pragma unroll
        for (int k = 0; k < HP; ++k) {
            q.ldiff[k] = fast_log2(fabsf(d[k].x - d[k].y));
            q.lmin[k] = fast_log2(fminf(fabsf(d[k].x), fabsf(d[k].y)));
        }
        return q;
    };
    // per gaze, first half: eccentricity -> ecc axis -> the four cells (issued back to back for the pixels of a phase)
    struct Cell {
        float4 v00, v10, v01, v11;
        float fE;
    };
    auto cell_of = [&](const Head& q, float dx2, float dy) -> Cell {
        Cell cq;
        const float ecc = __builtin_amdgcn_sqrtf(fmaf(dy, dy, dx2));      // band_item: dx2 + dy * dy, fused
        const float eq = __builtin_amdgcn_sqrtf(__builtin_amdgcn_fmed3f(ecc, a.ecc_lo, a.ecc_hi));
        const float tE = fmaf(eq, a.inv_step[2], a.grid_off[2]);
        const float iE = __builtin_amdgcn_fmed3f(floorf(tE), 0.0f, (float)(FVVDP_LUT_N - 2));
        cq.fE = (tE - iE) * a.frac_scale[2];
        const int bo = (int)fmaf(iE, (float)(FOV_ROW * 16), q.boY);
        const float4* cell = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_lut_dyn) + bo);
        constexpr int sj = 1, sk = FOV_ROW;
        cq.v00 = cell[0];
        cq.v10 = cell[sj];
        cq.v01 = cell[sk];
        cq.v11 = cell[sk + sj];
        return cq;
    };
    // per gaze, second half: interp3 and the log-domain masking tail of fov_b into the gaze's accumulators
    auto tail = [&](const Head& q, const Cell& cq, bool valid, float (&ac)[2]) {
        const float fY = q.fY, fE = cq.fE, fR = q.fR;
        auto rho_blend = [&](const float4& v) { return pfma(v2f{v.z, v.w}, fR, v2f{v.x, v.y}); };
        const v2f r00 = rho_blend(cq.v00), r10 = rho_blend(cq.v10), r01 = rho_blend(cq.v01), r11 = rho_blend(cq.v11);
        const v2f y0 = pfma(r10 - r00, fY, r00), y1 = pfma(r11 - r01, fY, r01);
        const v2f sl2 = pfma(y1 - y0, fE, y0);
        const float s0 = sl2.x, s1 = sl2.y;
        const float vm = valid ? 1.0f : 0.0f;
        if constexpr (HP == 2) {
            const v2f sl = v2f{s0, s1};
            const v2f A = pfma(sl, pb, splat(q.cA));
            const v2f lsm = sl + splat(q.cL);
            const v2f ldiff = v2f{q.ldiff[0], q.ldiff[1]}, lmin = v2f{q.lmin[0], q.lmin[1]};
            v2f bl;
            PYRAMID_MASK_POOL_PAIR(A, lsm, ldiff, lmin, pb, a.q0, a.q1, a.beta, b_dmax, vm, ac, bl);
        } else {
            (void)s1;
            // one channel: a kept copy, see pyramid_walk.hpp
            const float ls = s0 + q.lcn;
            const float mq = fast_exp2(a.q0 * (q.lmin[0] + (ls + lg_mask)));
            // band_item: ld = p * (...); ldd = fminf(ld - log2(1 + mq), lg_dmax), the product fused into the difference
            const float ldd = fminf(fmaf(a.p, q.ldiff[0] + (ls + lg_base), -fast_log2(1.0f + mq)), a.lg_dmax);
            ac[0] = fmaf(fast_exp2(a.beta * ldd), vm, ac[0]);
        }
    };

    // ---- main loop: band rows 2c, 2c+1 for c in [ca, cb)
    auto step = [&](auto PH, const int c) {
        constexpr int s0 = (4 + 2 * decltype(PH)::value) & 7;
        const Px<P> (&W0)[2] = R[s0];
        const Px<P> (&W1)[2] = R[(s0 + 1) & 7];
        const int jj = min(max(J, 0), a.rmap_w - 1);
        const float4 ra = a.rmap[(size_t)min(2 * c, h - 1) * a.rmap_w + jj];        // rho-map records first, then the row prefetch
        const float4 rb = a.rmap[(size_t)min(2 * c + 1, h - 1) * a.rmap_w + jj];
        __builtin_amdgcn_sched_barrier(0);
        load_row(2 * c + 5, R[(s0 + 5) & 7][0], R[(s0 + 5) & 7][1]);
        load_row(2 * c + 6, R[(s0 + 6) & 7][0], R[(s0 + 6) & 7][1]);
        const Px<P> cN = coarse_step(integral_constant<int, s0>());
        const bool has_next = (c + 1) <= (hc - 1);
        Px<P> Gp1 = has_next ? cN : G0;
        st_px(Gc_rsrc, (has_next && (c + 1) < cb && may_store) ? (unsigned int)((c + 1) * wc + J) * (P * 4u) : FVVDP_NO_STORE, cN);
        Px<P> x00, x01, x10, x11;
        PYRAMID_EXPAND_ROWS(HP, Gm1, G0, Gp1, ex.el, ex.er, ex.ec, ex.orr, ex.oc, x00, x01, x10, x11);
        const bool row1_ok = (2 * c + 1) < h;
        const float* s_vy = reinterpret_cast<const float*>(s_lut_dyn + FOV_PLANE * a.rw);
        const float vy0 = s_vy[2 * c];
        const float vy1 = s_vy[min(2 * c + 1, h - 1)];
        // two pixels per phase, as band_item: the heads of both, then per gaze the cells of both and their tails
        __builtin_amdgcn_sched_barrier(0);
        {
            const Head q0 = head(W0[0], x00, ra.x, ra.y);
            const Head q1 = head(W0[1], x01, ra.z, ra.w);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const float dy = vy0 - gyv[g];
                const Cell c0 = cell_of(q0, dxa2[g], dy);
                const Cell c1 = cell_of(q1, dxb2[g], dy);
                tail(q0, c0, active, acc[g]);
                tail(q1, c1, active && col1_ok, acc[g]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            const Head q2 = head(W1[0], x10, rb.x, rb.y);
            const Head q3 = head(W1[1], x11, rb.z, rb.w);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const float dy = vy1 - gyv[g];
                const Cell c2 = cell_of(q2, dxa2[g], dy);
                const Cell c3 = cell_of(q3, dxb2[g], dy);
                tail(q2, c2, active && row1_ok, acc[g]);
                tail(q3, c3, active && row1_ok && col1_ok, acc[g]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        Gm1 = G0;
        G0 = Gp1;
    };
    PYRAMID_WALK_STEPS(step, ca, cb);

#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const float s0 = wave_sum(acc[g][0]);
        const float s1 = wave_sum(acc[g][1]);
        if (lane == 0) {
            float* o = ga.partial + (size_t)g * ga.partial_stride + ((size_t)frame * (a.n_strips * a.n_chunks) + blk) * 2;
            o[0] = s0;
            o[1] = s1;
        }
    }
}

template <int P, int NG>
__global__ __launch_bounds__(64 * FOV_WPB, MG_MINW) void multigaze_kernel(const MultiGazeArgs a_byval) {
    const MultiGazeArgs& ga = *(const MultiGazeArgs*)__builtin_amdgcn_kernarg_segment_ptr();     // see band_kernel
    (void)a_byval;
    const BandArgs& a = ga.b;
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
    multigaze_item<P, NG>(ga, strip, chunk, frame, lane);
}

// Finalisation of every gaze with the single-gaze arithmetic (finalize_one, aux_kernels.hpp), the gaze on a grid axis of its
// own: each gaze keeps the fixed summation order of the single-gaze call.  (The pooling is pool_jod_kernel itself, once per gaze.)
struct GazeFinalizeArgs {
    FinalizeArgs f;             // gaze 0
    long long partial_stride;   // floats between the partial sums / the Q blocks of consecutive gazes
    long long q_stride_g;
};
__global__ __launch_bounds__(64) void finalize_gazes_kernel(const GazeFinalizeArgs a) {
    FinalizeArgs f = a.f;
    f.partial += (size_t)blockIdx.y * a.partial_stride;
    f.Q += (size_t)blockIdx.y * a.q_stride_g;
    const int i = blockIdx.x;
    finalize_one(f, i / (2 * f.n), (i / f.n) % 2, i % f.n, (int)threadIdx.x);
}
