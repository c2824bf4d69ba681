// Host code the three pyramid forward passes share (plain and foveated, many gazes, many tests; fvvdp_hip.hip) and, for the axis
// constants, the many-gaze backward (gaze_grad_launch.hip): the level sizes, the work decomposition of a launch as a function of
// plain integers, the most work items any such plan can have -- which is what sizes the partial sums -- and the constants of the
// foveated tables' axes.  Host code only, no HIP header and no context: a plain C++ program can include it
// (tests/pyramid_plan_check.cpp does, and proves there that no plan exceeds its bound).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "fvvdp_hip.h"
#include "pyramid_constants.hpp"

// sizes of pyramid levels 0 .. n_levels - 1: ceil(/2) per level (fvvdp_lpyr_dec.py:198)
static inline void pyramid_level_sizes(int width, int height, int n_levels, int* lw, int* lh) {
    for (int i = 0; i < n_levels; ++i) {
        lw[i] = width;
        lh[i] = height;
        width = (width + 1) / 2;
        height = (height + 1) / 2;
    }
}

// ---- plans ---------------------------------------------------------------------------------------------------------------------
struct BandPlan {               // one-level launch (band_kernel): strips of coarse columns, chunks of cr coarse rows
    int n_strips, n_chunks, cr;
};
struct Band2Plan {              // two-level launch (band2_kernel): strips of level-B columns, chunks of level-C rows -- the first
    int n_strips, n_chunks, kr, n_big, kr2;      // n_big of kr rows, the others of kr2
};

// strips cover coarse columns [0,62), [62,122), ... (see band_kernel)
static inline int band_strips(int wc) {
    return wc <= 62 ? 1 : 1 + (wc - 62 + STRIP_J - 1) / STRIP_J;
}

static inline int band2_strips(int wb) { return (wb + F2_PITCH - 1) / F2_PITCH; }

// cr_override >= 2 (FVVDP_BAND_CR): that chunk height instead of the cheapest one -- taller chunks, so fewer, never more
static inline BandPlan chunking(int hc, int n_strips, int n, long long capacity, int cr_override) {
    // Every single-wave workgroup does the same amount of work (cr steps + the prologue for the two halo coarse
    // rows, whose 7 extra fine rows are re-read from HBM: weighted as 8 steps), so the launch proceeds in "rounds"
    // of `capacity` resident waves.  Pick the chunk height that minimises rounds x per-wave cost.
    double best = 1e300;
    int cr = hc;
    for (int cand = 2; cand <= hc || cand == 2; ++cand) {
        const int c = cand > hc ? hc : cand;
        const long long chunks = (hc + c - 1) / c;
        const long long waves = (long long)n * n_strips * chunks;
        const long long rounds = (waves + capacity - 1) / capacity;
        const double cost = (double)rounds * ((double)c + 8.0) * (1.0 + 1e-4 * (double)chunks);
        if (cost < best) { best = cost; cr = c; }
        if (cand >= hc) break;
    }
    if (cr_override >= 2) cr = cr_override > hc ? hc : cr_override;
    return BandPlan{n_strips, (hc + cr - 1) / cr, cr};
}

// two-level kernel: a chunk of kr level-C rows costs 2*kr steps of level A plus 7 halo steps and the prologue; uniform chunks
static inline Band2Plan chunking2(int hc, int n_strips, int n, long long capacity, int kr_override) {
    double best = 1e300;
    int kr = hc;
    for (int cand = 1; cand <= hc; ++cand) {
        const long long chunks = (hc + cand - 1) / cand;
        const long long waves = (long long)n * n_strips * chunks;
        const long long rounds = (waves + capacity - 1) / capacity;
        const double cost = (double)rounds * (2.0 * cand + 9.0) * (1.0 + 1e-4 * (double)chunks);
        if (cost < best) { best = cost; kr = cand; }
    }
    if (kr_override >= 1) kr = kr_override > hc ? hc : kr_override;      // tuning override (FVVDP_BAND2_KR)
    const int n_chunks = (hc + kr - 1) / kr;
    return Band2Plan{n_strips, n_chunks, kr, n_chunks, kr};
}

// Does the plain pass walk levels b and b + 1 (of lw / lh [n_bands + 1]) in one two-level launch?  Where it pays -- large levels,
// see bands_forward_core -- and where the two-level border logic holds; fuse_mode (FVVDP_BAND_FUSE) 1 forces it wherever valid,
// 0 (the caller's check) never.
static inline bool band2_takes(const int* lw, const int* lh, int n_bands, int b, int fuse_mode) {
    const bool big = (long long)lw[b] * lh[b] >= 500000;      // (4K: levels 0+1 and 2+3; 2+3 in one launch: 3.06 -> 2.67 us per frame)
    return (big || fuse_mode == 1) && b + 1 < n_bands && lw[b + 1] >= 4 && lh[b + 1] >= 4 && lw[b + 2] >= 2 && lh[b + 2] >= 2;
}

// Work decomposition of the two-level launch over a level B of wb columns and a level C of hc rows for plan_n frames; capacity =
// resident waves of band2_kernel on the chip, kr_override / kr2_override = FVVDP_BAND2_KR (>= 1) / FVVDP_BAND2_KR2 (>= 0).
static inline Band2Plan band2_plan(int wb, int hc, int plan_n, long long capacity, int kr_override, int kr2_override) {
    Band2Plan p = chunking2(hc, band2_strips(wb), plan_n, capacity, kr_override);
    // a launch of several rounds of tall chunks: the last chunk of every frame is cut into four and dispatched after
    // all tall ones (band2_kernel's two phases)
    const long long waves = (long long)plan_n * p.n_strips * p.n_chunks;
    int kr2 = (waves >= 2 * capacity && p.n_chunks >= 3 && p.kr >= 16) ? (p.kr + 3) / 4 : 0;
    if (kr2_override >= 0) kr2 = kr2_override;                          // tuning override; 0 = uniform chunks
    if (kr2 >= 1 && kr2 < p.kr && p.n_chunks >= 2) {
        p.n_big = p.n_chunks - 1;
        p.kr2 = kr2;
        p.n_chunks = p.n_big + (hc - p.n_big * p.kr + kr2 - 1) / kr2;
    }
    return p;
}

// ---- bounds --------------------------------------------------------------------------------------------------------------------
// Per band, the most work items per frame that any plan above can have.  One level: chunks are at least two coarse rows.  Two
// levels (bands b, b + 1 share one work decomposition): a chunk is at least one level-C row; a band takes the larger bound.
// two_level = false: the passes that never take the two-level walk (many gazes).
static inline void pyramid_item_bounds(const int* lw, const int* lh, int n_bands, bool two_level, size_t* bound) {
    for (int b = 0; b < n_bands; ++b) bound[b] = (size_t)band_strips(lw[b + 1]) * ((lh[b + 1] + 1) / 2);
    for (int b = 0; two_level && b + 1 < n_bands; ++b) {
        const size_t blk2 = (size_t)band2_strips(lw[b + 1]) * lh[b + 2];
        if (blk2 > bound[b]) bound[b] = blk2;
        if (blk2 > bound[b + 1]) bound[b + 1] = blk2;
    }
}

// One row of a caller's workspace for n frames: per band [n][bound][2] floats at off[b] (off may be null); returns the row's
// floats, rounded up to 64.
static inline size_t pyramid_row_floats(const size_t* bound, int n_bands, int n, size_t* off) {
    size_t fl = 0;
    for (int b = 0; b < n_bands; ++b) {
        if (off) off[b] = fl;
        fl += (size_t)n * bound[b] * 2;
    }
    return (fl + 63) / 64 * 64;
}

// the row of a width x height frame with n_bands bands
static inline size_t pyramid_row_floats(int width, int height, int n_bands, int n, bool two_level, size_t* off) {
    int lw[FVVDP_MAX_BANDS + 1], lh[FVVDP_MAX_BANDS + 1];
    size_t bound[FVVDP_MAX_BANDS];
    pyramid_level_sizes(width, height, n_bands + 1, lw, lh);
    pyramid_item_bounds(lw, lh, n_bands, two_level, bound);
    return pyramid_row_floats(bound, n_bands, n, off);
}

// ---- foveated tables -----------------------------------------------------------------------------------------------------------
// What the kernels take of the three 32-knot axes (Y_log, rho_log, ecc_sqrt, in that order in `axes`) and of the display geometry
// (geom == nullptr, a user geometry: delta_rad = cos_delta = 0).
struct FovAxes {
    float first[3], inv_step[3];     // uniform-grid estimates of the three axes
    float grid_off[3];               // -first * inv_step
    float frac_scale[3];             // step / (step + 1e-6): fraction inside an interval from the grid position (interp.py:16)
    float delta_rad, cos_delta;      // half a pixel at the centre of the display, as an angle
    float y_lo, y_hi, rho_lo, rho_hi, ecc_lo, ecc_hi;       // the axes' ends in linear units
};

static inline FovAxes fov_axes(const float* axes, const fvvdp_geom* geom) {
    FovAxes f{};
    for (int ax = 0; ax < 3; ++ax) {
        const float* k = axes + ax * FVVDP_LUT_N;
        f.first[ax] = k[0];
        f.inv_step[ax] = (float)(FVVDP_LUT_N - 1) / (k[FVVDP_LUT_N - 1] - k[0]);
        const double step = ((double)k[FVVDP_LUT_N - 1] - (double)k[0]) / (FVVDP_LUT_N - 1);
        f.frac_scale[ax] = (float)(step / (step + 1e-6));
        f.grid_off[ax] = -f.first[ax] * f.inv_step[ax];
    }
    if (geom) {
        const double delta = (1.0 / (double)geom->ppd_centre) / 2.0 * M_PI / 180.0;
        f.delta_rad = (float)delta;
        f.cos_delta = (float)cos(delta);
    }
    const float *ya = axes, *ra = axes + FVVDP_LUT_N, *ea = axes + 2 * FVVDP_LUT_N;
    f.y_lo = exp2f(ya[0]);
    f.y_hi = exp2f(ya[FVVDP_LUT_N - 1]);
    f.rho_lo = exp2f(ra[0]);
    f.rho_hi = exp2f(ra[FVVDP_LUT_N - 1]);
    f.ecc_lo = ea[0] * ea[0];
    f.ecc_hi = ea[FVVDP_LUT_N - 1] * ea[FVVDP_LUT_N - 1];
    return f;
}
