// Stand-alone check of the launch plans, their bounds and the workspace rows of fovvideovdp_amd/csrc/pyramid_host.hpp
// (tests/test_pyramid_plan_cpu.py compiles it for the host with the address and undefined-behaviour sanitizers and runs it).  It
// includes nothing of the library but that header.  Four things:
//   1. restatement: the plan functions as they stood in fvvdp_hip.hip before the header existed, copied below, agree with the
//      header field for field;
//   2. bound: no plan, under any override, has more work items per frame than pyramid_item_bounds gives its band -- so the
//      library's refusal "internal: partial buffer too small" cannot fire;
//   3. cover: strips cover the columns, chunks the rows, exactly once, in order, none empty;
//   4. rows: the workspace rows have the documented layout and the byte counts tests/test_multitest_cpu.py and
//      tests/test_gazes_cpu.py assert.
#include <cstdio>
#include <vector>

#include "pyramid_host.hpp"

static int failures = 0;
#define EXPECT(cond, ...)                       \
    do {                                        \
        if (!(cond)) {                          \
            if (++failures <= 20) {             \
                fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
                fprintf(stderr, __VA_ARGS__);   \
                fprintf(stderr, "\n");          \
            }                                   \
        }                                       \
    } while (0)

// ---- the restatement: the functions of fvvdp_hip.hip that the header replaced, with the context's fields as parameters ---------
static int ref_band_strips(int wc) { return wc <= 62 ? 1 : 1 + (wc - 62 + 60 - 1) / 60; }

static int ref_band2_strips(int wb) { return (wb + 54 - 1) / 54; }

static void ref_chunking2(int hc, int n_strips, int n, long long capacity, int kr_override, int& n_chunks, int& kr) {
    double best = 1e300;
    kr = hc;
    for (int cand = 1; cand <= hc; ++cand) {
        const long long chunks = (hc + cand - 1) / cand;
        const long long waves = (long long)n * n_strips * chunks;
        const long long rounds = (waves + capacity - 1) / capacity;
        const double cost = (double)rounds * (2.0 * cand + 9.0) * (1.0 + 1e-4 * (double)chunks);
        if (cost < best) { best = cost; kr = cand; }
    }
    if (kr_override >= 1) kr = kr_override > hc ? hc : kr_override;
    n_chunks = (hc + kr - 1) / kr;
}

static void ref_chunking(int hc, int n_strips, int n, long long capacity, int& n_chunks, int& cr) {
    double best = 1e300;
    cr = hc;
    for (int cand = 2; cand <= hc || cand == 2; ++cand) {
        const int c = cand > hc ? hc : cand;
        const long long chunks = (hc + c - 1) / c;
        const long long waves = (long long)n * n_strips * chunks;
        const long long rounds = (waves + capacity - 1) / capacity;
        const double cost = (double)rounds * ((double)c + 8.0) * (1.0 + 1e-4 * (double)chunks);
        if (cost < best) { best = cost; cr = c; }
        if (cand >= hc) break;
    }
    n_chunks = (hc + cr - 1) / cr;
}

// the override as fill_band_args applied it after chunking()
static void ref_band_cr(int hc, int band_cr, int& n_chunks, int& cr) {
    if (band_cr >= 2) {
        cr = band_cr > hc ? hc : band_cr;
        n_chunks = (hc + cr - 1) / cr;
    }
}

static void ref_band2_plan(int wb, int hc, int plan_n, long long wave_capacity2, int env_band2_kr, int env_band2_kr2, int& n_strips,
                           int& n_chunks, int& kr, int& n_big, int& kr2_out) {
    n_strips = ref_band2_strips(wb);
    ref_chunking2(hc, n_strips, plan_n, wave_capacity2, env_band2_kr, n_chunks, kr);
    n_big = n_chunks;
    kr2_out = kr;
    const long long waves = (long long)plan_n * n_strips * n_chunks;
    int kr2 = (waves >= 2 * wave_capacity2 && n_chunks >= 3 && kr >= 16) ? (kr + 3) / 4 : 0;
    if (env_band2_kr2 >= 0) kr2 = env_band2_kr2;
    if (kr2 >= 1 && kr2 < kr && n_chunks >= 2) {
        n_big = n_chunks - 1;
        kr2_out = kr2;
        n_chunks = n_big + (hc - n_big * kr + kr2 - 1) / kr2;
    }
}

// max_blk[] as fvvdp_ctx_create filled it
static void ref_max_blk(const int* lw, const int* lh, int n_bands, int* max_blk) {
    for (int b = 0; b < n_bands; ++b) {
        const int n_strips = ref_band_strips(lw[b + 1]);
        const int max_chunks = (lh[b + 1] + 1) / 2;
        max_blk[b] = n_strips * max_chunks;
    }
    for (int b = 0; b + 1 < n_bands; ++b) {
        const int blk2 = ref_band2_strips(lw[b + 1]) * lh[b + 2];
        if (blk2 > max_blk[b]) max_blk[b] = blk2;
        if (blk2 > max_blk[b + 1]) max_blk[b + 1] = blk2;
    }
}

// ---- the sweep -----------------------------------------------------------------------------------------------------------------
static const int N_FRAMES[] = {1, 2, 3, 16, 60, 128};
static const long long CAPACITY[] = {1, 64, 4096, 8192};
static const int KR_OVERRIDE[] = {0, 1, 5, -1};          // -1: a value above hc
static const int KR2_OVERRIDE[] = {-1, 0, 1, 4};
static const int CR_OVERRIDE[] = {0, 2, 3, 7, -1};       // -1: a value above hc
static const int FRAME_SIDES[] = {4, 5, 7, 8, 63, 64, 65, 125, 248, 249, 1920, 3840, 7680};

// level heights: every value 1 ... 100, every seventh from there to 300 (thinned: the searches cost hc steps each, and the whole
// program is to finish in a few seconds under the sanitizers), 300, and the levels of 1080p ... 8K frames
static std::vector<int> level_heights() {
    std::vector<int> v;
    for (int h = 1; h <= 100; ++h) v.push_back(h);
    for (int h = 107; h < 300; h += 7) v.push_back(h);
    v.push_back(300);
    for (int h : {540, 1080, 2160, 2161, 4320}) v.push_back(h);
    return v;
}

// level widths: at, one below and one above every strip boundary up to four strips of either pitch, and the levels of 4K ... 16K
static std::vector<int> level_widths() {
    std::vector<int> v;
    for (int s = 0; s < 4; ++s)
        for (int d = -1; d <= 1; ++d) {
            v.push_back(62 + STRIP_J * s + d);
            v.push_back(F2_PITCH * (s + 1) + d);
        }
    for (int w : {1920, 3840, 7680}) v.push_back(w);
    return v;
}

// 3. chunks [0, n_big) of kr rows, then chunks of kr2 rows, as the kernels walk them, cover rows [0, hc) once, in order, none empty
static void check_chunks(int hc, int n_chunks, int kr, int n_big, int kr2, const char* what) {
    int next = 0;
    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        const bool big = chunk < n_big;
        const int ka = big ? chunk * kr : n_big * kr + (chunk - n_big) * kr2;
        const int kb = ka + (big ? kr : kr2) < hc ? ka + (big ? kr : kr2) : hc;
        EXPECT(ka == next && kb > ka, "%s: hc %d, chunk %d of %d (kr %d, n_big %d, kr2 %d) is rows [%d, %d) after %d", what, hc, chunk,
               n_chunks, kr, n_big, kr2, ka, kb, next);
        next = kb;
    }
    EXPECT(next == hc, "%s: hc %d: %d chunks (kr %d, n_big %d, kr2 %d) end at row %d", what, hc, n_chunks, kr, n_big, kr2, next);
}

// 3. strips of one pitch cover columns [0, w) once, none empty: strip s of the one-level kernels owns lanes [2, 62) of columns
// STRIP_J s + lane (strip 0: lanes [0, 62)), strip s of the two-level kernel columns [F2_PITCH s, F2_PITCH (s + 1))
static void check_strips(int w) {
    std::vector<int> seen((size_t)w, 0), seen2((size_t)w, 0);
    const int ns = band_strips(w);
    for (int s = 0; s < ns; ++s) {
        const int lo = s == 0 ? 0 : STRIP_J * s + 2, hi = STRIP_J * s + 62;
        EXPECT(lo < w, "width %d: strip %d of %d of pitch %d is empty", w, s, ns, STRIP_J);
        for (int j = lo; j < hi && j < w; ++j) seen[(size_t)j] += 1;
    }
    const int ns2 = band2_strips(w);
    for (int s = 0; s < ns2; ++s) {
        EXPECT(F2_PITCH * s < w, "width %d: strip %d of %d of pitch %d is empty", w, s, ns2, F2_PITCH);
        for (int j = F2_PITCH * s; j < F2_PITCH * (s + 1) && j < w; ++j) seen2[(size_t)j] += 1;
    }
    for (int j = 0; j < w; ++j)
        EXPECT(seen[(size_t)j] == 1 && seen2[(size_t)j] == 1, "width %d: column %d is covered %d times at pitch %d, %d times at pitch %d", w,
               j, seen[(size_t)j], STRIP_J, seen2[(size_t)j], F2_PITCH);
    EXPECT(ns == ref_band_strips(w) && ns2 == ref_band2_strips(w), "width %d: %d / %d strips", w, ns, ns2);
}

// 1. + 3. the one-level plan of a level of hc rows and `width` columns, under every override
static void check_plan1(int hc, int width, int n, long long capacity) {
    const int ns = band_strips(width);
    int ref_chunks = 0, ref_cr = 0;
    ref_chunking(hc, ref_band_strips(width), n, capacity, ref_chunks, ref_cr);
    for (int o : CR_OVERRIDE) {
        const int band_cr = o < 0 ? hc + 3 : o;
        int want_chunks = ref_chunks, want_cr = ref_cr;
        ref_band_cr(hc, band_cr, want_chunks, want_cr);
        const BandPlan p = chunking(hc, ns, n, capacity, band_cr);
        EXPECT(p.n_strips == ns && p.n_chunks == want_chunks && p.cr == want_cr,
               "chunking(hc %d, strips %d, n %d, capacity %lld, cr %d): {%d, %d, %d}, the restatement has {%d, %d}", hc, ns, n, capacity,
               band_cr, p.n_strips, p.n_chunks, p.cr, want_chunks, want_cr);
        EXPECT(p.n_chunks <= (hc + 1) / 2, "chunking(hc %d, cr override %d): %d chunks", hc, band_cr, p.n_chunks);
        check_chunks(hc, p.n_chunks, p.cr, p.n_chunks, p.cr, "one level");
    }
}

// 1. + 3. the two-level plan over a level B of `width` columns and a level C of hc rows, under every override
static void check_plan2(int hc, int width, int n, long long capacity) {
    for (int o : KR_OVERRIDE)
        for (int kr2_override : KR2_OVERRIDE) {
            const int kr_override = o < 0 ? hc + 3 : o;
            int n_strips, n_chunks, kr, n_big, kr2;
            ref_band2_plan(width, hc, n, capacity, kr_override, kr2_override, n_strips, n_chunks, kr, n_big, kr2);
            const Band2Plan p = band2_plan(width, hc, n, capacity, kr_override, kr2_override);
            EXPECT(p.n_strips == n_strips && p.n_chunks == n_chunks && p.kr == kr && p.n_big == n_big && p.kr2 == kr2,
                   "band2_plan(wb %d, hc %d, n %d, capacity %lld, kr %d, kr2 %d): {%d, %d, %d, %d, %d}, the restatement has {%d, %d, %d, %d, %d}",
                   width, hc, n, capacity, kr_override, kr2_override, p.n_strips, p.n_chunks, p.kr, p.n_big, p.kr2, n_strips, n_chunks, kr,
                   n_big, kr2);
            EXPECT(p.n_chunks <= hc, "band2_plan(hc %d, kr %d, kr2 %d): %d chunks", hc, kr_override, kr2_override, p.n_chunks);
            check_chunks(hc, p.n_chunks, p.kr, p.n_big, p.kr2, "two levels");
            if (kr2_override == 0) {          // uniform chunks: the restated plan is what the restated chunking2 left
                const Band2Plan u = chunking2(hc, n_strips, n, capacity, kr_override);
                EXPECT(u.n_strips == n_strips && u.n_chunks == n_chunks && u.kr == kr && u.n_big == n_chunks && u.kr2 == kr,
                       "chunking2(hc %d, strips %d, n %d, capacity %lld, kr %d): {%d, %d}, the restatement has {%d, %d}", hc, n_strips, n,
                       capacity, kr_override, u.n_chunks, u.kr, n_chunks, kr);
            }
        }
}

// 2. + 4. a frame of w x h with n_bands bands: every band's plans against its bound, and the rows laid out from the bounds
static void check_frame(int w, int h, int n_bands) {
    int lw[FVVDP_MAX_BANDS + 1], lh[FVVDP_MAX_BANDS + 1], max_blk[FVVDP_MAX_BANDS];
    size_t bound[FVVDP_MAX_BANDS], bound1[FVVDP_MAX_BANDS];
    pyramid_level_sizes(w, h, n_bands + 1, lw, lh);
    for (int i = 0; i <= n_bands; ++i)
        EXPECT(lw[i] == (i ? (lw[i - 1] + 1) / 2 : w) && lh[i] == (i ? (lh[i - 1] + 1) / 2 : h), "%dx%d: level %d is %dx%d", w, h, i, lw[i], lh[i]);
    pyramid_item_bounds(lw, lh, n_bands, true, bound);
    pyramid_item_bounds(lw, lh, n_bands, false, bound1);
    ref_max_blk(lw, lh, n_bands, max_blk);
    for (int b = 0; b < n_bands; ++b) {
        EXPECT(bound[b] == (size_t)max_blk[b], "%dx%d, %d bands: bound[%d] = %zu, max_blk %d", w, h, n_bands, b, bound[b], max_blk[b]);
        EXPECT(bound1[b] == (size_t)ref_band_strips(lw[b + 1]) * (size_t)((lh[b + 1] + 1) / 2) && bound1[b] <= bound[b],
               "%dx%d, %d bands: one-level bound[%d] = %zu", w, h, n_bands, b, bound1[b]);
    }
    for (int n : N_FRAMES) {
        for (long long capacity : CAPACITY)
            for (int b = 0; b < n_bands; ++b) {
                const int hc = lh[b + 1];
                for (int o : CR_OVERRIDE) {
                    const BandPlan p = chunking(hc, band_strips(lw[b + 1]), n, capacity, o < 0 ? hc + 3 : o);
                    const size_t nblk = (size_t)p.n_strips * (size_t)p.n_chunks;
                    EXPECT(nblk <= bound1[b] && nblk <= bound[b], "%dx%d band %d, n %d, capacity %lld, cr override %d: %zu items, bound %zu / %zu",
                           w, h, b, n, capacity, o, nblk, bound1[b], bound[b]);
                }
                if (b + 1 >= n_bands) continue;
                const int hc2 = lh[b + 2];
                for (int o : KR_OVERRIDE)
                    for (int kr2_override : KR2_OVERRIDE) {
                        const Band2Plan p = band2_plan(lw[b + 1], hc2, n, capacity, o < 0 ? hc2 + 3 : o, kr2_override);
                        const size_t nblk = (size_t)p.n_strips * (size_t)p.n_chunks;
                        // both bands the launch feeds; band b + 1's bound is also what the many-tests pass needs where it walks
                        // level B alone in this decomposition
                        EXPECT(nblk <= bound[b] && nblk <= bound[b + 1], "%dx%d bands %d+%d, n %d, capacity %lld, kr %d, kr2 %d: %zu items, bounds %zu, %zu",
                               w, h, b, b + 1, n, capacity, o, kr2_override, nblk, bound[b], bound[b + 1]);
                    }
            }
        // the rows: the context's own bound for the many-tests pass, the one-level bound for the many-gazes pass
        for (int two = 0; two < 2; ++two) {
            const size_t* bd = two ? bound : bound1;
            size_t off[FVVDP_MAX_BANDS], off2[FVVDP_MAX_BANDS];
            const size_t row = pyramid_row_floats(bd, n_bands, n, off);
            EXPECT(row == pyramid_row_floats(w, h, n_bands, n, two != 0, off2) && row == pyramid_row_floats(w, h, n_bands, n, two != 0, nullptr),
                   "%dx%d, %d bands, n %d: the row from the frame size", w, h, n_bands, n);
            size_t end = 0;
            for (int b = 0; b < n_bands; ++b) {
                EXPECT(off[b] == end && off2[b] == end, "%dx%d, %d bands, n %d: band %d starts at %zu, not %zu", w, h, n_bands, n, b, off[b], end);
                end += 2 * (size_t)n * bd[b];
            }
            EXPECT(row % 64 == 0 && row >= end && row - end < 64, "%dx%d, %d bands, n %d: row of %zu floats for %zu", w, h, n_bands, n, row, end);
        }
    }
}

int main() {
    int cases = 0;
    const std::vector<int> heights = level_heights(), widths = level_widths();
    for (int w : widths) check_strips(w);
    for (int hc : heights)
        for (int n : N_FRAMES)
            for (long long capacity : CAPACITY) {
                // a plan sees the width through its strip count only: widths that share the count share one case
                std::vector<int> planned1, planned2;
                for (int w : widths) {
                    bool done1 = false, done2 = false;
                    for (int k : planned1) done1 = done1 || k == band_strips(w);
                    for (int k : planned2) done2 = done2 || k == band2_strips(w);
                    if (!done1) {
                        planned1.push_back(band_strips(w));
                        check_plan1(hc, w, n, capacity);
                        cases += 1;
                    }
                    if (!done2) {
                        planned2.push_back(band2_strips(w));
                        check_plan2(hc, w, n, capacity);
                        cases += 1;
                    }
                }
            }
    for (int w : FRAME_SIDES)
        for (int h : FRAME_SIDES) {
            int most = 0;                    // levels 0 .. n_bands - 1 are at least 2x2 (fvvdp_ctx_create)
            for (int lw = w, lh = h; most < FVVDP_MAX_BANDS && lw >= 2 && lh >= 2; lw = (lw + 1) / 2, lh = (lh + 1) / 2) most += 1;
            for (int n_bands = 1; n_bands <= most; ++n_bands) {
                check_frame(w, h, n_bands);
                cases += 1;
            }
        }
    // 4. the byte counts of tests/test_multitest_cpu.py and tests/test_gazes_cpu.py, per row
    EXPECT(pyramid_row_floats(64, 48, 4, 3, true, nullptr) == (size_t)((3 * (12 + 12 + 6 + 3) * 2 + 63) / 64 * 64), "tests row of 64x48");
    EXPECT(pyramid_row_floats(64, 48, 4, 3, false, nullptr) == (size_t)((3 * (12 + 6 + 3 + 2) * 2 + 63) / 64 * 64), "gaze row of 64x48");
    EXPECT(pyramid_row_floats(3840, 2160, 1, 1, true, nullptr) == (size_t)((32 * 540 * 2 + 63) / 64 * 64), "tests row of one 4K band");
    EXPECT(pyramid_row_floats(3840, 2160, 1, 1, false, nullptr) == (size_t)((32 * 540 * 2 + 63) / 64 * 64), "gaze row of one 4K band");
    EXPECT(pyramid_row_floats(3840, 2160, 2, 2, true, nullptr) == (size_t)((2 * (36 * 540 + 36 * 540) * 2 + 63) / 64 * 64), "tests row of two 4K bands");
    cases += 5;
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("pyramid_host: %d cases pass\n", cases);
    return 0;
}
