// Gradients of the video JOD of many tests with respect to their one reference (include/fvvdp_hip_tests_grad.h): argument
// checks, workspace layout and launches of tests_ref_layer_kernel (tests_grad_kernels.hpp) and, through video_grad_launch.hip
// and grad_launch.hip, of video_coef_kernel, adj_sweep_kernel and video_level0_kernel.  A translation unit of its own: it reads
// only what the caller passes, never a context, and changes nothing the forward path or the other backward passes compile.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "fvvdp_hip.h"
#include "fvvdp_hip_tests_grad.h"
#include "device_common.hpp"
#include "temporal_kernels.hpp"
#include "grad_common.hpp"
#include "ref_grad_kernels.hpp"
#include "tests_grad_kernels.hpp"
#include "grad_host.hpp"

// the limits of fvvdp_video_ref_grad_frames: the 2n planes of a batch and the rows of level 0 are grid dimensions
static int check_dims(int width, int height, int n_bands, int n, int n_tests) {
    GRAD_CHECK(grad_check_dims(width, height, n_bands, n, 16384, 65535, "frames"));
    if (n_tests < 1) return grad_fail(FVVDP_EINVAL, "n_tests must be at least 1, got %d", n_tests);
    return FVVDP_OK;
}

// floats of one test's coefficients [n][2][n_bands], 256-byte aligned; they follow the single-test layout
static size_t coef_floats(int n, int n_bands) { return align64((size_t)n * 2 * n_bands); }

// the single-test layout of the reference's backward, then the coefficients of every test
static void tests_layout(int width, int height, int n_bands, int n, int n_tests, RefGradLayout& R, GradLayout& need) {
    ref_grad_layout(width, height, n_bands, n, 2, R);
    need = R.L;
    need.total = R.L.total + (size_t)n_tests * coef_floats(n, n_bands);
}

extern "C" int fvvdp_tests_ref_grad_workspace(int width, int height, int n_bands, int n, int n_tests, size_t* bytes) {
    if (!bytes) return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(check_dims(width, height, n_bands, n, n_tests));
    RefGradLayout R;
    GradLayout need;
    tests_layout(width, height, n_bands, n, n_tests, R, need);
    *bytes = need.total * sizeof(float);
    return FVVDP_OK;
}

template <int NT>
static void launch_layer(const RefLayerArgs& la, const TestsGroupArgs& ga, int blocks, int n, hipStream_t st) {
    hipLaunchKernelGGL((tests_ref_layer_kernel<NT>), dim3(blocks, n), dim3(256), 0, st, la, ga);
}

extern "C" int fvvdp_tests_ref_grad_layer(int width, int height, int n_bands, int n, int n_tests, int test0, int n_group,
                                          int group_max, int add, const fvvdp_params* prm, const fvvdp_pool_params* pool,
                                          const float* d_Q, int n_frames, int f0, const float* d_gamma,
                                          const fvvdp_band_maps* maps, const float* const* h_slope_ptrs, void* d_work,
                                          size_t work_bytes, void* stream) {
    if (!prm || !pool || !d_Q || !d_gamma || !maps || !h_slope_ptrs || !d_work) return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(check_dims(width, height, n_bands, n, n_tests));
    if (test0 < 0 || n_group < 1 || test0 > n_tests - n_group)
        return grad_fail(FVVDP_EINVAL, "tests [%d, %d) lie outside the %d tests of the clip", test0, test0 + n_group, n_tests);
    if (group_max != 0 && group_max != 1 && group_max != 2 && group_max != FVVDP_TESTS_GRAD_GROUP_MAX)
        return grad_fail(FVVDP_EINVAL, "group_max must be 0 (the default, %d), 1, 2 or %d, got %d", FVVDP_TESTS_GRAD_GROUP_MAX,
                         FVVDP_TESTS_GRAD_GROUP_MAX, group_max);
    if (add != 0 && add != 1) return grad_fail(FVVDP_EINVAL, "add must be 0 (store) or 1 (add), got %d", add);
    if (n_frames < 1 || f0 < 0 || f0 + n > n_frames)
        return grad_fail(FVVDP_EINVAL, "frames [%d, %d) lie outside the clip of %d frames", f0, f0 + n, n_frames);
    GRAD_CHECK(grad_check_exponents({pool->beta_sch, pool->beta_tch, pool->beta_t, pool->beta_jod, prm->beta}));
    for (int j = 0; j < n_group; ++j) GRAD_CHECK(grad_check_maps(maps + (size_t)j * n_bands, n_bands));
    GRAD_CHECK(check_slopes(h_slope_ptrs, n_bands));
    if ((reinterpret_cast<uintptr_t>(d_Q) | reinterpret_cast<uintptr_t>(d_gamma)) % 4 != 0)
        return grad_fail(FVVDP_EINVAL, "device pointers must be aligned to 4 bytes");
    RefGradLayout R;
    GradLayout need;
    tests_layout(width, height, n_bands, n, n_tests, R, need);
    GRAD_CHECK(grad_check_workspace(d_work, work_bytes, need));
    float* ws = static_cast<float*>(d_work);
    const size_t csz = coef_floats(n, n_bands);
    float* coef = ws + R.L.total;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    // 1. coefficients of the batch's frames, per test of the call: its Q_per_ch, its upstream gradient
    const size_t q_test = (size_t)n_bands * 2 * n_frames;
    for (int j = 0; j < n_group; ++j) {
        const int k = test0 + j;
        GRAD_HIP_TRY(video_coef_launch(d_Q + k * q_test, d_gamma + k, coef + k * csz, n, n_bands, n_frames, f0, prm, pool, R.L, st));
    }

    // 2. layer gradients of every band, summed over the tests: one launch per group of tests
    const int cap = group_max ? group_max : FVVDP_TESTS_GRAD_GROUP_MAX;      // smaller groups, more launches: same bits
    for (int j = 0; j < n_group;) {
        int nt = FVVDP_TESTS_GRAD_GROUP_MAX;         // the largest instantiation that the tests left fill: 4, 2, 1
        while (nt > cap || nt > n_group - j) nt >>= 1;
        RefLayerArgs la;
        TestsGroupArgs ga;
        memset(&la, 0, sizeof(la));
        memset(&ga, 0, sizeof(ga));
        // the shared planes, the outputs and the reference's contrast planes: from the map set of the group's first test
        const int blocks = grad_fill_layer(la, maps + (size_t)j * n_bands, ws, R.L, n_bands, prm);
        for (int b = 0; b < n_bands; ++b) {
            la.band[b].K = h_slope_ptrs[b];
            la.band[b].GX = ws + R.gx[b];
            for (int t = 0; t < nt; ++t) {
                ga.D[b][t] = maps[(size_t)(j + t) * n_bands + b].d_D;
                ga.Cn[b][t] = maps[(size_t)(j + t) * n_bands + b].d_contrast;
            }
        }
        la.q[0] = prm->mask_q[0];
        la.q[1] = prm->mask_q[1];
        la.lbkg_min = prm->lbkg_min;
        ga.coef = coef + (size_t)(test0 + j) * csz;
        ga.coef_stride = (long long)csz;
        ga.accumulate = (add || j > 0) ? 1 : 0;
        switch (nt) {
            case 4: launch_layer<4>(la, ga, blocks, n, st); break;
            case 2: launch_layer<2>(la, ga, blocks, n, st); break;
            default: launch_layer<1>(la, ga, blocks, n, st); break;
        }
        GRAD_HIP_TRY(hipGetLastError());
        j += nt;
    }
    return FVVDP_OK;
}

extern "C" int fvvdp_tests_ref_grad_finish(int width, int height, int n_bands, int n, int n_tests, int n_frames, int f0,
                                           float* d_g0, void* d_work, size_t work_bytes, void* stream) {
    if (!d_g0 || !d_work) return grad_fail(FVVDP_EINVAL, "null argument");
    GRAD_CHECK(check_dims(width, height, n_bands, n, n_tests));
    if (n_frames < 1 || f0 < 0 || f0 + n > n_frames)
        return grad_fail(FVVDP_EINVAL, "frames [%d, %d) lie outside the clip of %d frames", f0, f0 + n, n_frames);
    if (reinterpret_cast<uintptr_t>(d_g0) % 4 != 0) return grad_fail(FVVDP_EINVAL, "d_g0 must be aligned to 4 bytes");
    RefGradLayout R;
    GradLayout need;
    tests_layout(width, height, n_bands, n, n_tests, R, need);
    GRAD_CHECK(grad_check_workspace(d_work, work_bytes, need));
    float* ws = static_cast<float*>(d_work);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t HW = (size_t)width * height;

    // coarse to fine on the 2n planes, then level 0 into the clip-long buffer (video_level0_kernel reads L.gl[0], GLR_0 here,
    // and L.gg[1]): once, whatever the number of tests
    GRAD_HIP_TRY(grad_sweep_levels(ws, R.L, n_bands, 2 * n, st, R.gx));
    GRAD_HIP_TRY(video_level0_launch(ws, R.L, d_g0 + (size_t)f0 * 2 * HW, n, st));
    return FVVDP_OK;
}
