// Stand-alone check of the launch windows and the window filler of fovvideovdp_amd/csrc/ingest_host.hpp against a direct
// restatement (tests/test_ingest_host_cpu.py compiles it for the host with the address and undefined-behaviour sanitizers and runs
// it).  It includes nothing of the library but that header; the argument block is a dummy with the members the filler names.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ingest_host.hpp"

struct DummyOut {
    float* lo;
    float* hi;
    size_t half_stride;
    int slot0;
};
struct DummyArgs {             // the members of TemporalArgs that the filler writes, guarded on both sides
    int guard0;
    int n_out, fl;
    DummyOut out;
    float taps2[64][2];
    int guard1;
    int idx[T_MAX_IDX];
    int guard2;
    int idx1[T_MAX_IDX];
    int guard3;
};
struct DummyArgs1 {            // one list for both streams (YuvArgs, YuvPlanesArgs, ResizedArgs)
    int n_out, fl;
    DummyOut out;
    float taps2[32][2];
    int idx[T_MAX_IDX];
};

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

// the restatement: ring length, most outputs of a launch, and entry u of the list of the window that starts at t0
static int ring_of(int fl) {
    if (fl <= 8) return 8;
    if (fl <= 16) return 16;
    if (fl <= 32) return 32;
    return 64;
}
static int max_out_of(int FL) {
    switch (FL) {
        case 8: return 313;
        case 16: return 305;
        case 32: return 289;
        default: return 257;
    }
}
static int entry_of(const std::vector<int32_t>& list, int fl, int t0, int u) {
    const int FL = ring_of(fl);
    int s = t0 + u - (FL - fl);          // the FL - fl slots before the true history show the list's first frame
    if (s < 0) s = 0;
    return list[(size_t)s];
}

static void check_case(int fl, int n_out, bool two_lists) {
    const int FL = ring_of(fl), max_out = max_out_of(FL), slot0 = 5;
    EXPECT(ingest_ring_length(fl) == FL, "fl %d", fl);
    EXPECT(max_out == T_MAX_IDX - (FL - 1), "FL %d", FL);
    // exactly the fl - 1 + n_out entries a caller owes: the sanitizer sees any read beyond them
    std::vector<int32_t> l0((size_t)(fl - 1 + n_out)), l1((size_t)(fl - 1 + n_out));
    for (size_t i = 0; i < l0.size(); ++i) {
        l0[i] = (int32_t)((i * 7 + 3) % 1000);
        l1[i] = (int32_t)((i * 11 + 1) % 977);
    }
    std::vector<float> taps((size_t)(2 * fl));
    for (int k = 0; k < 2 * fl; ++k) taps[(size_t)k] = 0.25f + (float)k;
    int next = 0, windows = 0;
    for (const IngestWindow wnd : IngestWindows(fl, n_out)) {
        EXPECT(wnd.t0 == next, "fl %d n_out %d: window %d starts at %d, not %d", fl, n_out, windows, wnd.t0, next);
        EXPECT(wnd.nn >= 1 && wnd.nn <= max_out, "fl %d n_out %d: window of %d outputs", fl, n_out, wnd.nn);
        EXPECT(wnd.nn == max_out || wnd.t0 + wnd.nn == n_out, "fl %d n_out %d: a short window before the last", fl, n_out);
        next = wnd.t0 + wnd.nn;
        windows += 1;
        DummyArgs a;
        memset(&a, 0, sizeof(a));
        a.guard0 = a.guard1 = a.guard2 = a.guard3 = 0x5a5a5a5a;
        const int32_t* neg = ingest_fill_window(a, wnd, slot0, taps.data(), fl, l0.data(), two_lists ? l1.data() : nullptr);
        EXPECT(neg == nullptr, "fl %d n_out %d: a list without negative entries is refused", fl, n_out);
        EXPECT(a.n_out == wnd.nn && a.fl == fl && a.out.slot0 == slot0 + wnd.t0, "fl %d n_out %d t0 %d: n_out %d fl %d slot0 %d", fl,
               n_out, wnd.t0, a.n_out, a.fl, a.out.slot0);
        EXPECT(a.out.lo == nullptr && a.out.hi == nullptr && a.out.half_stride == 0, "the filler touched the level's address");
        for (int k = 0; k < 64; ++k) {
            const float s = k < fl ? taps[(size_t)k] : 0.0f, t = k < fl ? taps[(size_t)(fl + k)] : 0.0f;
            EXPECT(a.taps2[k][0] == s && a.taps2[k][1] == t, "fl %d: tap pair %d is {%g, %g}", fl, k, a.taps2[k][0], a.taps2[k][1]);
        }
        for (int u = 0; u < T_MAX_IDX; ++u) {
            const bool used = u < FL - 1 + wnd.nn;
            const int w0 = used ? entry_of(l0, fl, wnd.t0, u) : 0;
            const int w1 = used ? entry_of(two_lists ? l1 : l0, fl, wnd.t0, u) : 0;
            EXPECT(a.idx[u] == w0, "fl %d n_out %d t0 %d: idx[%d] = %d, not %d", fl, n_out, wnd.t0, u, a.idx[u], w0);
            EXPECT(a.idx1[u] == w1, "fl %d n_out %d t0 %d: idx1[%d] = %d, not %d", fl, n_out, wnd.t0, u, a.idx1[u], w1);
        }
        EXPECT(a.guard0 == 0x5a5a5a5a && a.guard1 == 0x5a5a5a5a && a.guard2 == 0x5a5a5a5a && a.guard3 == 0x5a5a5a5a,
               "fl %d n_out %d: a write outside the arrays", fl, n_out);
        if (fl <= 32 && !two_lists) {       // the block with one list
            DummyArgs1 b;
            memset(&b, 0, sizeof(b));
            EXPECT(ingest_fill_window(b, wnd, slot0, taps.data(), fl, l0.data()) == nullptr, "fl %d n_out %d", fl, n_out);
            EXPECT(b.n_out == a.n_out && b.fl == a.fl && b.out.slot0 == a.out.slot0, "fl %d n_out %d: one-list block", fl, n_out);
            EXPECT(memcmp(b.idx, a.idx, sizeof(b.idx)) == 0, "fl %d n_out %d: one-list block's idx", fl, n_out);
            EXPECT(memcmp(b.taps2, a.taps2, sizeof(b.taps2)) == 0, "fl %d n_out %d: one-list block's taps", fl, n_out);
        }
    }
    EXPECT(next == n_out, "fl %d n_out %d: the windows end at %d", fl, n_out, next);
    EXPECT(windows == (n_out + max_out - 1) / max_out, "fl %d n_out %d: %d windows", fl, n_out, windows);

    // a negative entry is refused: by the window that reads it, in whichever list it stands, and by no other window
    const int at = (fl - 1 + n_out) / 2;
    for (int which = 0; which < (two_lists ? 2 : 1); ++which) {
        std::vector<int32_t>& bad = which ? l1 : l0;
        const int32_t keep = bad[(size_t)at];
        bad[(size_t)at] = -3;
        int refused = 0;
        for (const IngestWindow wnd : IngestWindows(fl, n_out)) {
            DummyArgs a;
            memset(&a, 0, sizeof(a));
            const int32_t* neg = ingest_fill_window(a, wnd, slot0, taps.data(), fl, l0.data(), two_lists ? l1.data() : nullptr);
            // the window reads entries [max(0, t0 - (FL - fl)), t0 + fl - 1 + nn) of the list
            const int first = wnd.t0 - (FL - fl) < 0 ? 0 : wnd.t0 - (FL - fl), last = wnd.t0 + fl - 1 + wnd.nn;
            const bool reads = at >= first && at < last;
            EXPECT((neg != nullptr) == reads, "fl %d n_out %d t0 %d: negative entry at %d %s", fl, n_out, wnd.t0, at,
                   neg ? "refused by a window that does not read it" : "passed");
            if (neg) {
                EXPECT(neg == &bad[(size_t)at] && *neg == -3, "fl %d n_out %d: the entry reported is not the negative one", fl, n_out);
                refused += 1;
            }
        }
        EXPECT(refused >= 1, "fl %d n_out %d: no window refused the negative entry", fl, n_out);
        bad[(size_t)at] = keep;
    }
}

int main() {
    static_assert(ingest_sample_bytes(FVVDP_U8) == 1 && ingest_sample_bytes(FVVDP_U16) == 2 && ingest_sample_bytes(FVVDP_F32) == 4 &&
                  ingest_sample_bytes(FVVDP_F16) == 2 && ingest_sample_bytes(FVVDP_BF16) == 2, "bytes per sample");
    const int fls[] = {1, 7, 8, 9, 13, 16, 30, 32, 33, 60, 64};
    int cases = 0;
    for (int fl : fls) {
        const int max_out = max_out_of(ring_of(fl));
        const int n_outs[] = {1, 2, max_out - 1, max_out, max_out + 1, 2 * max_out + 3};
        for (int n_out : n_outs)
            for (int two = 0; two < 2; ++two) {
                check_case(fl, n_out, two != 0);
                cases += 1;
            }
    }
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("ingest_host: %d cases pass\n", cases);
    return 0;
}
