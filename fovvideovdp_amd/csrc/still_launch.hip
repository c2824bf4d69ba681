// Instantiations + launcher of the batched still-image ingest (still_kernels.hpp).
// A translation unit of its own because it is compiled with -fno-slp-vectorize (fovvideovdp_amd/_native.py): with four pixels per
// lane the SLP vectorizer packs the display models' multiplies and adds of neighbouring pixels into v_pk_mul / v_pk_add, and some of
// the multiply-adds that the one-pixel kernels contract into v_fma no longer are -- level 0 then differs from the single-image path
// (temporal_generic_kernel) in the last bit.  Without it every pixel is evaluated with the same instructions as there.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstddef>
#include <cstdint>

#include "fvvdp_hip.h"
#include "device_common.hpp"
#include "temporal_kernels.hpp"
#include "still_kernels.hpp"

template <int SRC, int PX>
static void launch(const StillArgs& a, int n, hipStream_t st) {
    const long long per_block = (long long)STILL_ITER * 256 * PX;
    const dim3 grid((unsigned int)((a.HW + per_block - 1) / per_block), (unsigned int)n), block(256);
    if constexpr (src_is_half(SRC)) hipLaunchKernelGGL((still_ingest_half_kernel<SRC, PX>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((still_ingest_kernel<SRC, PX>), grid, block, 0, st, a);
}

// uint16 always runs one pixel per lane: with four, the closed-form display models of RGB input still contract differently from
// temporal_generic_kernel (measured on MI355X: ~5200 of 7680 level-0 values of a 64x120 RGB pair off by an ulp; gray and every
// uint8 / float case bit-identical), and level 0 must be bit-identical to the single-image path
void still_launch(int dtype, int px, const StillArgs& a, int n, hipStream_t st) {
    if (dtype == FVVDP_U8) {
        if (px == 4) launch<SRC_U8, 4>(a, n, st);
        else launch<SRC_U8, 1>(a, n, st);
    } else if (dtype == FVVDP_U16) {
        launch<SRC_U16, 1>(a, n, st);
    } else if (dtype == FVVDP_F16) {
        if (px == 4) launch<SRC_F16, 4>(a, n, st);
        else launch<SRC_F16, 1>(a, n, st);
    } else if (dtype == FVVDP_BF16) {
        if (px == 4) launch<SRC_BF16, 4>(a, n, st);
        else launch<SRC_BF16, 1>(a, n, st);
    } else {
        if (px == 4) launch<SRC_F32, 4>(a, n, st);
        else launch<SRC_F32, 1>(a, n, st);
    }
}
