// Stand-alone check of the index arithmetic of one resize axis, fovvideovdp_amd/csrc/resize_axis.hpp (tests/test_resize_axis_cpu.py
// compiles it for the host with the address and undefined-behaviour sanitizers and runs it).  It includes nothing of the library
// but that header.  Size pairs "n_in:n_out" on the command line are checked first (the wrapper passes the per-axis pairs of
// tests/resize_cases.py), then the pairs named below, then a fixed-seed sample; every pair in both directions, every target index:
//   area      the window equals ATen's start_index / end_index restated in 64-bit integers; 0 <= a0 < a1 <= n; the windows begin
//             at 0, end at n, never step back and leave no gap (a downscale's windows overlap in at most one sample)
//   the rest  every index lies in [0, n - 1]; nearest and the lower bilinear index never step back
//   reach     rz_axis_reach brackets the samples rz_axis_weight gives a weight: none outside [lo, hi] (three samples on either
//             side, and the whole axis where it is short); nearest, area and identity weigh EVERY sample of [lo, hi], with weights
//             that are the tap's; bilinear and bicubic (whose end taps may weigh exactly 0) have their taps' indices inside and the
//             weights over [lo, hi] add up to the sum of the taps' coefficients
// Signed overflow in the header's 32-bit products would end the program (-fsanitize=undefined, no recovery).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "resize_axis.hpp"

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

// ATen, AdaptiveAveragePooling.cpp: start_index(a, b, c) = (a * c) / b, end_index(a, b, c) = 1 + ((a + 1) * c - 1) / b
static void aten_window(int64_t o, int64_t n, int64_t n_out, int64_t& a0, int64_t& a1) {
    a0 = (o * n) / n_out;
    a1 = 1 + ((o + 1) * n - 1) / n_out;
}

template <int MODE>
static void check_reach(int o, int n, int n_out, float scale) {
    int lo, hi;
    rz_axis_reach<MODE>(o, n, n_out, scale, lo, hi);
    EXPECT(0 <= lo && lo <= hi && hi <= n - 1, "mode %d %d -> %d, target %d: reach [%d, %d]", MODE, n, n_out, o, lo, hi);
    if (!(0 <= lo && lo <= hi && hi <= n - 1)) return;
    const int from = n <= 512 ? 0 : (lo - 3 < 0 ? 0 : lo - 3), to = n <= 512 ? n - 1 : (hi + 3 > n - 1 ? n - 1 : hi + 3);
    float sum = 0.0f;
    for (int s = from; s <= to; ++s) {
        const float w = rz_axis_weight<MODE>(o, s, n, n_out, scale);
        if (s < lo || s > hi) {
            EXPECT(w == 0.0f, "mode %d %d -> %d, target %d: sample %d outside the reach [%d, %d] weighs %g", MODE, n, n_out, o, s, lo, hi,
                   (double)w);
        } else {
            sum += w;
            if (MODE == FVVDP_RESIZE_NEAREST || MODE == RZ_IDENTITY)
                EXPECT(w == 1.0f, "mode %d %d -> %d, target %d: sample %d weighs %g", MODE, n, n_out, o, s, (double)w);
            if (MODE == FVVDP_RESIZE_AREA)
                EXPECT(w == 1.0f / (float)(hi - lo + 1), "area %d -> %d, target %d: sample %d of [%d, %d] weighs %g", n, n_out, o, s, lo, hi,
                       (double)w);
        }
    }
    if (MODE == FVVDP_RESIZE_BILINEAR) {
        int i0, i1;
        float l1;
        rz_bilinear_axis(o, n, scale, i0, i1, l1);
        EXPECT(lo == i0 && hi == i1, "bilinear %d -> %d, target %d: taps %d, %d outside the reach [%d, %d]", n, n_out, o, i0, i1, lo, hi);
        EXPECT(0.0f <= l1 && l1 <= 1.0f && sum == (1.0f - l1) + l1, "bilinear %d -> %d, target %d: weights add up to %g", n, n_out, o,
               (double)sum);
    }
    if (MODE == FVVDP_RESIZE_BICUBIC) {
        int idx[4];
        float c[4];
        rz_cubic_axis(o, n, scale, idx, c);
        for (int k = 0; k < 4; ++k)
            EXPECT(lo <= idx[k] && idx[k] <= hi, "bicubic %d -> %d, target %d: tap %d at %d outside the reach [%d, %d]", n, n_out, o, k,
                   idx[k], lo, hi);
        // the coefficients add up to 1 within their roundings (intermediates of up to 6, four roundings each); so do the weights,
        // which are sums of the same four numbers in another order
        EXPECT(std::fabs(sum - 1.0f) <= 96.0f * 5.9604645e-8f, "bicubic %d -> %d, target %d: weights add up to %.9g", n, n_out, o, (double)sum);
    }
}

static void check_pair(int n, int n_out) {
    const float scale = (float)n / (float)n_out;                   // area_pixel_compute_scale without a scale factor
    int prev_a0 = 0, prev_a1 = 0, prev_near = 0, prev_i0 = 0;
    for (int o = 0; o < n_out; ++o) {
        int a0, a1;
        rz_area_axis(o, n, n_out, a0, a1);
        int64_t w0, w1;
        aten_window(o, n, n_out, w0, w1);
        EXPECT(a0 == w0 && a1 == w1, "area %d -> %d, target %d: [%d, %d), ATen [%lld, %lld)", n, n_out, o, a0, a1, (long long)w0, (long long)w1);
        EXPECT(0 <= a0 && a0 < a1 && a1 <= n, "area %d -> %d, target %d: [%d, %d)", n, n_out, o, a0, a1);
        if (o == 0) EXPECT(a0 == 0, "area %d -> %d: the first window starts at %d", n, n_out, a0);
        if (o > 0) {
            EXPECT(a0 >= prev_a0 && a1 >= prev_a1, "area %d -> %d, target %d: the window steps back", n, n_out, o);
            EXPECT(a0 <= prev_a1, "area %d -> %d, target %d: gap [%d, %d)", n, n_out, o, prev_a1, a0);
            if (n_out <= n) EXPECT(a0 >= prev_a1 - 1, "area %d -> %d, target %d: overlap [%d, %d)", n, n_out, o, a0, prev_a1);
        }
        if (o == n_out - 1) EXPECT(a1 == n, "area %d -> %d: the last window ends at %d", n, n_out, a1);
        prev_a0 = a0;
        prev_a1 = a1;

        const int near = rz_nearest_axis(o, n, scale);
        EXPECT(0 <= near && near <= n - 1 && near >= prev_near, "nearest %d -> %d, target %d: %d after %d", n, n_out, o, near, prev_near);
        prev_near = near;
        int i0, i1;
        float l1;
        rz_bilinear_axis(o, n, scale, i0, i1, l1);
        EXPECT(0 <= i0 && i0 <= i1 && i1 <= n - 1 && i1 - i0 <= 1 && i0 >= prev_i0, "bilinear %d -> %d, target %d: %d, %d", n, n_out, o, i0, i1);
        prev_i0 = i0;
        int idx[4];
        float c[4];
        rz_cubic_axis(o, n, scale, idx, c);
        for (int k = 0; k < 4; ++k)
            EXPECT(0 <= idx[k] && idx[k] <= n - 1 && (k == 0 || idx[k] >= idx[k - 1]), "bicubic %d -> %d, target %d: tap %d at %d", n, n_out, o,
                   k, idx[k]);

        check_reach<FVVDP_RESIZE_NEAREST>(o, n, n_out, scale);
        check_reach<FVVDP_RESIZE_BILINEAR>(o, n, n_out, scale);
        check_reach<FVVDP_RESIZE_BICUBIC>(o, n, n_out, scale);
        check_reach<FVVDP_RESIZE_AREA>(o, n, n_out, scale);
        if (n == n_out) check_reach<RZ_IDENTITY>(o, n, n_out, scale);
    }
}

int main(int argc, char** argv) {
    std::vector<std::pair<int, int>> pairs;
    for (int i = 1; i < argc; ++i) {
        int a = 0, b = 0;
        if (sscanf(argv[i], "%d:%d", &a, &b) != 2 || a < 1 || b < 1 || a > RZ_MAX_AXIS || b > RZ_MAX_AXIS) {
            fprintf(stderr, "bad size pair '%s'\n", argv[i]);
            return 2;
        }
        pairs.push_back({a, b});
    }
    // products of an index and a size beyond 2^24, where a float32 window leaves ATen's (5805 -> 2903: its last window would end at
    // n + 1); the largest sizes; one sample from many and many from one
    const int named[][2] = {{4100, 4099}, {4320, 4319}, {7680, 4097}, {5805, 2903}, {8192, 8191}, {32768, 30000}, {32768, 32767},
                            {32768, 1}, {1, 32768}, {32768, 32768}};
    for (const auto& p : named) pairs.push_back({p[0], p[1]});
    uint64_t state = 0x9E3779B97F4A7C15ull;                        // a fixed-seed sample (splitmix64)
    auto next = [&]() {
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    for (int i = 0; i < 300; ++i) {
        const int a = 1 + (int)(next() % RZ_MAX_AXIS), b = 1 + (int)(next() % RZ_MAX_AXIS);
        pairs.push_back({a, b});
    }
    int cases = 0;
    for (const auto& p : pairs) {
        check_pair(p.first, p.second);
        cases += 1;
        if (p.first != p.second) {
            check_pair(p.second, p.first);
            cases += 1;
        }
    }
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("resize_axis: %d cases pass\n", cases);
    return 0;
}
