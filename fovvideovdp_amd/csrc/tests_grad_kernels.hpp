// Backward of the video JOD of many tests with respect to their one reference (include/fvvdp_hip_tests_grad.h): the layer
// gradients of a loss
//   sum_k w_k JOD_k    (w_k = the upstream gradient of test k)
// summed over the tests BEFORE the linear tail of the reference's backward (adj_sweep_kernel, video_level0_kernel,
// video_input_kernel), which then runs once instead of once per test.  Instantiated and launched by tests_grad_launch.hip.
//
// Per band pixel ref_layer_kernel<2> (ref_grad_kernels.hpp) reads 11 planes.  Seven depend on the reference only -- L_bkg, S x 2,
// kappa x 2 and the reference's contrast x 2 -- and are read here once per group of NT tests; per test the kernel reads the
// test's contrast x 2, D x 2 and its coefficients, evaluates ref_layer_one per temporal channel exactly as the single-test
// kernel does, forms GX_0 = GLR_0 - GB per test, and adds the test's GLR and GX to the running sums.
#pragma once

// What a launch takes beside the RefLayerArgs of the single-test kernel (whose band records hold the shared planes, the
// outputs and, in D and Cn, the maps of the group's first test)
struct TestsGroupArgs {
    const float* D[FVVDP_MAX_BANDS][FVVDP_TESTS_GRAD_GROUP_MAX];    // test t of the group: [n][2][h][w]
    const float* Cn[FVVDP_MAX_BANDS][FVVDP_TESTS_GRAD_GROUP_MAX];   // [n][4][h][w]; plane 2cc is read
    const float* coef;      // test t of the group: coef + t * coef_stride, then [n][2][n_bands]
    long long coef_stride;
    int accumulate;         // 0: start from +0 (the first group of a batch); 1: from the sums the groups before left
};

// grid (workgroups of all bands, n frames), 256 threads, one band pixel per thread: every plane is one coalesced stream of
// dwords, 256 B per wave instruction, as in ref_layer_kernel (the bands' odd sizes leave the planes of a batch at any 4-byte
// alignment, so wider loads would need a per-plane head and tail).  NT tests per launch: 1, 2 or 4.
// GLR = sum_k glr_k, GX = sum_k gx_k in ascending test order: the first group of a batch starts from +0, a later one from the
// value the groups before it left, so each sum is the same chain of additions whatever the group sizes.  __fadd_rn on values
// that ref_layer_one and the GX_0 line return through selects: no term's last multiply is fused into the sum.  No atomics.
template <int NT>
__global__ __launch_bounds__(256) void tests_ref_layer_kernel(const RefLayerArgs a, const TestsGroupArgs g) {
    int b = 0;
    while (b + 1 < a.n_bands && (int)blockIdx.x >= a.band[b + 1].blk0) ++b;
    const RefBand& B = a.band[b];
    const int k = blockIdx.y;
    const size_t hw = (size_t)B.w * B.h;
    const size_t px = (size_t)((int)blockIdx.x - B.blk0) * 256 + threadIdx.x;
    if (px >= hw) return;

    // ---- once per band pixel: what depends on the reference only ----------------------------------------------------------
    const float lb = B.L[(size_t)k * hw + px];
    const float rlb = fast_rcp(lb);
    const float m_lb = B.m * rlb;
    float R[2], s[2], kap[2];
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
        R[cc] = B.Cn[((size_t)k * 4 + 2 * cc + 1) * hw + px];
        s[cc] = B.S[((size_t)k * 2 + cc) * hw + px] * a.gain;
        kap[cc] = B.K[((size_t)k * 2 + cc) * hw + px];
    }
    float* gl = B.GL + (size_t)k * 2 * hw + px;
    float* gx = B.GX + (size_t)k * 2 * hw + px;
    float sl[2] = {0.0f, 0.0f}, sx[2] = {0.0f, 0.0f};
    if (g.accumulate) {
        sl[0] = gl[0];
        sl[1] = gl[hw];
        sx[0] = gx[0];
        sx[1] = gx[hw];
    }

    // ---- once per test of the group ---------------------------------------------------------------------------------------
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const float* cf = g.coef + (size_t)t * g.coef_stride + (size_t)k * 2 * a.n_bands + b;
        float glr[2], gbs = 0.0f;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const float c = cf[cc * a.n_bands];
            const float T = g.Cn[b][t][((size_t)k * 4 + 2 * cc) * hw + px];
            const float Dm = g.D[b][t][((size_t)k * 2 + cc) * hw + px];
            float gb;
            ref_layer_one(c, T, R[cc], Dm, s[cc], kap[cc], m_lb, a.q[cc], B.m, a, glr[cc], gb);
            gbs += gb;
        }
        const float GB = lb > a.lbkg_min ? gbs * rlb : 0.0f;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            sl[cc] = __fadd_rn(sl[cc], glr[cc]);
            sx[cc] = __fadd_rn(sx[cc], cc == 0 ? glr[cc] - GB : glr[cc]);
        }
    }
    gl[0] = sl[0];
    gl[hw] = sl[1];
    gx[0] = sx[0];
    gx[hw] = sx[1];
}
