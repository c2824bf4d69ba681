// The sums behind the gradients with respect to the model parameters (include/fvvdp_hip_params.h): argument checks, workspace
// layout and launches of param_sums_kernel / param_finalize_kernel (param_kernels.hpp).  A translation unit of its own: it reads
// only what the caller passes, never a context (fvvdp_ctx_set_params lives with the context, in fvvdp_hip.hip).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "fvvdp_hip.h"
#include "fvvdp_hip_params.h"
#include "device_common.hpp"
#include "param_kernels.hpp"

int fvvdp_fail_from(int code, const char* msg);      // fvvdp_hip.hip: sets the message of fvvdp_last_error

static int param_fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static int param_fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return fvvdp_fail_from(FVVDP_EINVAL, buf);
}

// workgroups per band (blk0[b] .. blk0[b + 1]) and pixels per band
struct ParamLayout {
    int blk0[FVVDP_MAX_BANDS + 1];
    unsigned int hw[FVVDP_MAX_BANDS];
};

static int param_layout(int width, int height, int n_bands, int n, ParamLayout& L) {
    if (width < 1 || height < 1 || n < 1 || n > 65535 || n_bands < 1 || n_bands > FVVDP_MAX_BANDS ||
        (size_t)width * height > (size_t)1 << 30)
        return param_fail("bad shape %dx%d, %d bands, %d slots", width, height, n_bands, n);
    int w = width, h = height, blocks = 0;
    for (int b = 0; b < n_bands; ++b) {              // ceil(/2), as the context's levels (fvvdp_lpyr_dec.py:198)
        L.blk0[b] = blocks;
        L.hw[b] = (unsigned int)w * (unsigned int)h;
        blocks += (int)((L.hw[b] + PS_BLOCK_PX - 1) / PS_BLOCK_PX);
        w = (w + 1) / 2;
        h = (h + 1) / 2;
    }
    L.blk0[n_bands] = blocks;
    return FVVDP_OK;
}

extern "C" int fvvdp_param_sums_workspace(int width, int height, int n_bands, int n, size_t* bytes) {
    if (!bytes) return param_fail("null argument");
    ParamLayout L;
    const int rc = param_layout(width, height, n_bands, n, L);
    if (rc != FVVDP_OK) return rc;
    *bytes = (size_t)L.blk0[n_bands] * n * 2 * PS_SUMS * sizeof(double);
    return FVVDP_OK;
}

extern "C" int fvvdp_param_sums(int width, int height, int n_bands, int n, int planes, const fvvdp_params* prm,
                                const fvvdp_band_maps* maps, double* d_sums, void* d_work, size_t work_bytes, void* stream) {
    if (!prm || !maps || !d_sums || !d_work) return param_fail("null argument");
    if (planes != 2 && planes != 4) return param_fail("planes must be 2 (image) or 4 (video), got %d", planes);
    ParamLayout L;
    const int rc = param_layout(width, height, n_bands, n, L);
    if (rc != FVVDP_OK) return rc;
    for (float x : {prm->mask_p, prm->mask_q[0], prm->mask_q[1], prm->beta, prm->mask_k, prm->sens_gain, prm->d_max})
        if (!(x > 0.0f) || !std::isfinite(x))
            return param_fail("mask_p, mask_q, beta, mask_k, sens_gain and d_max must be positive and finite");
    for (int b = 0; b < n_bands; ++b)
        if (!maps[b].d_D || !maps[b].d_contrast || !maps[b].d_S)
            return param_fail("band %d: the maps D, contrast and S are required", b);
    if (reinterpret_cast<uintptr_t>(d_sums) % 8 != 0) return param_fail("d_sums must be aligned to 8 bytes");
    if (reinterpret_cast<uintptr_t>(d_work) % 256 != 0) return param_fail("workspace must be 256-byte aligned");
    const size_t need = (size_t)L.blk0[n_bands] * n * 2 * PS_SUMS * sizeof(double);
    if (work_bytes < need) return param_fail("workspace of %zu bytes is below the %zu needed", work_bytes, need);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    ParamSumsArgs a;
    memset(&a, 0, sizeof(a));
    for (int b = 0; b < n_bands; ++b) {
        ParamBand& B = a.band[b];
        B.D = maps[b].d_D;
        B.Cn = maps[b].d_contrast;
        B.S = maps[b].d_S;
        B.hw = L.hw[b];
        B.blk0 = L.blk0[b];
        const uintptr_t bits = reinterpret_cast<uintptr_t>(B.D) | reinterpret_cast<uintptr_t>(B.Cn) | reinterpret_cast<uintptr_t>(B.S);
        if (bits % 4 != 0) return param_fail("band %d: the maps must be aligned to 4 bytes", b);
        B.vec = (L.hw[b] % 4 == 0 && bits % 16 == 0) ? 1 : 0;
    }
    a.partial = static_cast<double*>(d_work);
    a.n_bands = n_bands;
    a.n = n;
    a.p = prm->mask_p;
    a.q[0] = prm->mask_q[0];
    a.q[1] = prm->mask_q[1];
    a.k_mask = prm->mask_k;
    a.beta = prm->beta;
    a.gain = prm->sens_gain;
    a.dmax_hi = prm->d_max * (1.0f - 0x1p-20f);      // the maps hold the clamped value, rounded (grad_host.hpp)
    if (planes == 4) hipLaunchKernelGGL((param_sums_kernel<4>), dim3(L.blk0[n_bands], n), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((param_sums_kernel<2>), dim3(L.blk0[n_bands], n), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fvvdp_fail_from(FVVDP_EHIP, hipGetErrorString(e));

    ParamFinalizeArgs f;
    memset(&f, 0, sizeof(f));
    f.partial = a.partial;
    f.sums = d_sums;
    for (int b = 0; b <= n_bands; ++b) f.blk0[b] = L.blk0[b];
    f.n = n;
    f.channels = planes / 2;
    hipLaunchKernelGGL(param_finalize_kernel, dim3(n_bands, n), dim3(256), 0, st, f);
    e = hipGetLastError();
    if (e != hipSuccess) return fvvdp_fail_from(FVVDP_EHIP, hipGetErrorString(e));
    return FVVDP_OK;
}
