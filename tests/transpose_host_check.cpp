// Stand-alone check of fovvideovdp_amd/csrc/transpose_host.hpp, the host code the four clip backwards share for their temporal
// transpose, against a restatement of the loops as they stood in the four entry points (tests/test_transpose_host_cpu.py compiles
// it for the host with the address and undefined-behaviour sanitizers and runs it).  It includes nothing of the library but that
// header.  The window index lists and their fold lists are restated from fvvdp.window_frame_indices and grad_passes.fold_list.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "transpose_host.hpp"

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

// ---- the restatement ----------------------------------------------------------------------------------------------------------------
struct Verdict {
    int code;
    std::string msg;
};
static Verdict refuse(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static Verdict refuse(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return Verdict{FVVDP_EINVAL, buf};
}

// the fold-list loop of fvvdp_video_grad_input_st, fvvdp_video_grad_luminance and fvvdp_video_display_sums (source == false) and
// of fvvdp_video_grad_input_held (source == true: "names source frame")
static Verdict old_check_fold(const int32_t* h_fold_frame, const int32_t* h_fold_pos, int fl, int n_frames, bool source) {
    bool seen[64] = {false};
    for (int i = 0; i < fl; ++i) {
        const int f = h_fold_frame[i], p = h_fold_pos[i];
        if (f < 0 || f >= n_frames) {
            if (source) return refuse("fold list entry %d names source frame %d outside [0, %d)", i, f, n_frames);
            return refuse("fold list entry %d names frame %d outside [0, %d)", i, f, n_frames);
        }
        if (p < 0 || p >= fl || seen[p]) return refuse("fold list entry %d: head position %d is outside [0, %d) or listed twice", i, p, fl);
        seen[p] = true;
        if (i > 0 && (f < h_fold_frame[i - 1] || (f == h_fold_frame[i - 1] && p < h_fold_pos[i - 1])))
            return refuse("fold list must be sorted by frame, then by position (entry %d)", i);
    }
    return Verdict{FVVDP_OK, ""};
}
// mb: the bytes of the frame map in front of the head (held entry point), else 0
static Verdict old_check_head_bytes(size_t head_bytes, int fl, size_t HW, size_t mb) {
    if (head_bytes < mb + (size_t)fl * HW * sizeof(float))
        return refuse("side buffer of %zu bytes is below the %zu needed", head_bytes, mb + (size_t)fl * HW * sizeof(float));
    return Verdict{FVVDP_OK, ""};
}
static int old_ring_length(int fl) { return fl <= 8 ? 8 : (fl <= 16 ? 16 : (fl <= 32 ? 32 : 64)); }
static int old_ring_length_held(int fl) { return fl <= 8 ? 8 : (fl <= 16 ? 16 : 32); }
static size_t old_pxv(int FL) { return FL <= 16 ? 4 : 2; }

struct OldBlock {               // the members the four fill loops wrote, guarded on both sides
    int guard0;
    float tapsT[64][2];
    int guard1;
    int fold_frame[64];
    int guard2;
    int fold_pos[64];
    int guard3;
};
static void old_fill(OldBlock& ia, const float* h_taps, int fl, const int32_t* h_fold_frame, const int32_t* h_fold_pos) {
    for (int m = 0; m < fl; ++m) {
        ia.tapsT[m][0] = h_taps[fl - 1 - m];
        ia.tapsT[m][1] = h_taps[fl + fl - 1 - m];
    }
    for (int i = 0; i < 64; ++i) {
        ia.fold_frame[i] = i < fl ? h_fold_frame[i] : -1;
        ia.fold_pos[i] = i < fl ? h_fold_pos[i] : 0;
    }
}

// fvvdp.window_frame_indices: the head of the list, fl entries (the rest is frames 1 .. N - 1)
static std::vector<int> head_of(int N, int fl, int padding) {
    std::vector<int> first;
    if (padding == 0) {                 // replicate
        first.assign((size_t)fl, 0);
    } else if (padding == 1) {          // circular
        for (int kk = 0; kk < fl; ++kk) first.push_back((((N - 1 - fl + kk) % N) + N) % N);
    } else {                            // pingpong
        std::vector<int> seq, hist;
        for (int f = 0; f < N; ++f) seq.push_back(f);
        for (int f = N - 2; f > 0; --f) seq.push_back(f);
        while ((int)hist.size() < fl - 1) hist.insert(hist.end(), seq.begin(), seq.end());
        first.assign(hist.end() - (fl - 1), hist.end());
        first.push_back(0);
    }
    return first;
}
// grad_passes.fold_list and _fold_arrays: for every frame in ascending order the ascending head positions that show it
static void fold_of(const std::vector<int>& head, int N, std::vector<int32_t>& ff, std::vector<int32_t>& fp) {
    ff.clear();
    fp.clear();
    for (int j = 0; j < N; ++j)
        for (int p = 0; p < (int)head.size(); ++p)
            if (head[(size_t)p] == j) {
                ff.push_back(j);
                fp.push_back(p);
            }
}

// ---- the comparison -----------------------------------------------------------------------------------------------------------------
static long lists = 0;
// both wordings of the check on one list; `valid`: what the list must be found to be
static void compare_fold(const std::vector<int32_t>& ff, const std::vector<int32_t>& fp, int fl, int N, bool valid, const char* what) {
    for (int source = 0; source < 2; ++source) {
        const Verdict o = old_check_fold(ff.data(), fp.data(), fl, N, source != 0);
        const TransposeVerdict n = transpose_check_fold(ff.data(), fp.data(), fl, N, source ? "source frame" : "frame");
        EXPECT(o.code == n.code && o.msg == n.msg, "fl %d N %d (%s): '%s' (%d) became '%s' (%d)", fl, N, what, o.msg.c_str(), o.code, n.msg,
               n.code);
        EXPECT((n.code == FVVDP_OK) == valid && (valid || n.msg[0]), "fl %d N %d (%s): verdict %d '%s'", fl, N, what, n.code, n.msg);
    }
    lists += 1;
}

static void check_case(int fl, int N, int padding) {
    const std::vector<int> head = head_of(N, fl, padding);
    EXPECT((int)head.size() == fl, "fl %d N %d padding %d: a head of %zu entries", fl, N, padding, head.size());
    // exactly the fl entries and 2 fl taps a caller owes: the sanitizer sees any read beyond them
    std::vector<int32_t> ff, fp;
    fold_of(head, N, ff, fp);
    EXPECT((int)ff.size() == fl, "fl %d N %d padding %d: the head names a frame outside the clip", fl, N, padding);
    if ((int)ff.size() != fl) return;
    compare_fold(ff, fp, fl, N, true, "valid");

    // ring length and pixels per lane
    const int FL = old_ring_length(fl);
    EXPECT(transpose_ring_length(fl, 64) == FL, "fl %d", fl);
    if (fl <= 32) EXPECT(transpose_ring_length(fl, 32) == old_ring_length_held(fl), "fl %d (held)", fl);
    EXPECT((size_t)transpose_px(FL) == old_pxv(FL), "FL %d", FL);
    int reached = 0;
    transpose_dispatch<64>(FL, [&](auto c) { reached = c.value; });
    EXPECT(reached == FL, "FL %d dispatched to %d", FL, reached);
    if (fl <= 32) {
        reached = 0;
        transpose_dispatch<32>(old_ring_length_held(fl), [&](auto c) { reached = c.value; });
        EXPECT(reached == old_ring_length_held(fl), "FL %d dispatched to %d (held)", old_ring_length_held(fl), reached);
    }

    // the fill
    std::vector<float> taps((size_t)(2 * fl));
    for (int k = 0; k < 2 * fl; ++k) taps[(size_t)k] = 0.25f + (float)k;
    OldBlock o;
    memset(&o, 0, sizeof(o));
    o.guard0 = o.guard1 = o.guard2 = o.guard3 = 0x5a5a5a5a;
    old_fill(o, taps.data(), fl, ff.data(), fp.data());
    struct { int guard0; TransposeArgs t; int guard1; } n;
    memset(&n, 0, sizeof(n));
    n.guard0 = n.guard1 = 0x5a5a5a5a;
    float g0 = 0.0f, hd = 0.0f;
    transpose_fill(n.t, &g0, &hd, (size_t)35, N, fl, taps.data(), ff.data(), fp.data());
    EXPECT(n.t.g0 == &g0 && n.t.head == &hd && n.t.HW == 35 && n.t.N == N && n.t.fl == fl, "fl %d N %d: the scalars", fl, N);
    static_assert(sizeof(n.t.tapsT) == sizeof(o.tapsT) && sizeof(n.t.fold_frame) == sizeof(o.fold_frame) &&
                  sizeof(n.t.fold_pos) == sizeof(o.fold_pos), "64 slots");
    EXPECT(memcmp(n.t.tapsT, o.tapsT, sizeof(o.tapsT)) == 0, "fl %d: tapsT", fl);
    EXPECT(memcmp(n.t.fold_frame, o.fold_frame, sizeof(o.fold_frame)) == 0, "fl %d N %d: fold_frame and its padding", fl, N);
    EXPECT(memcmp(n.t.fold_pos, o.fold_pos, sizeof(o.fold_pos)) == 0, "fl %d N %d: fold_pos and its padding", fl, N);
    for (int i = fl; i < 64; ++i)
        EXPECT(n.t.fold_frame[i] == -1 && n.t.fold_pos[i] == 0 && n.t.tapsT[i][0] == 0.0f && n.t.tapsT[i][1] == 0.0f, "fl %d: slot %d", fl, i);
    EXPECT(n.guard0 == 0x5a5a5a5a && n.guard1 == 0x5a5a5a5a && o.guard0 == 0x5a5a5a5a && o.guard1 == 0x5a5a5a5a &&
           o.guard2 == 0x5a5a5a5a && o.guard3 == 0x5a5a5a5a, "fl %d N %d: a write outside the block", fl, N);

    // every single-defect mutation of the valid list
    for (int i = 0; i < fl; ++i) {
        const int32_t f = ff[(size_t)i], p = fp[(size_t)i];
        for (int32_t bad : {-1, N, N + 7}) {                // a frame out of range
            ff[(size_t)i] = bad;
            compare_fold(ff, fp, fl, N, false, "frame out of range");
        }
        ff[(size_t)i] = f;
        for (int32_t bad : {-1, fl, fl + 5}) {              // a position outside [0, fl)
            fp[(size_t)i] = bad;
            compare_fold(ff, fp, fl, N, false, "position out of range");
        }
        for (int k : {0, i - 1, i + 1, fl - 1}) {           // a position listed twice: that of the first, a neighbour, the last
            if (k == i || k < 0 || k >= fl) continue;
            fp[(size_t)i] = fp[(size_t)k];
            compare_fold(ff, fp, fl, N, false, "position listed twice");
        }
        fp[(size_t)i] = p;
        for (int k : {i + 1, fl - 1}) {                     // two entries swapped: the next one, the last one
            if (k <= i || k >= fl) continue;
            std::swap(ff[(size_t)i], ff[(size_t)k]);
            std::swap(fp[(size_t)i], fp[(size_t)k]);
            compare_fold(ff, fp, fl, N, false, "two entries swapped");
            std::swap(ff[(size_t)i], ff[(size_t)k]);
            std::swap(fp[(size_t)i], fp[(size_t)k]);
        }
    }
    compare_fold(ff, fp, fl, N, true, "restored");

    // the side buffer on both sides of its size, with and without a frame map in front
    for (size_t HW : {(size_t)1, (size_t)35, (size_t)1920 * 1080})
        for (size_t mb : {(size_t)0, (size_t)256})
            for (int d = -1; d <= 1; ++d) {
                const size_t bytes = mb + (size_t)fl * HW * 4 + (size_t)d;
                const Verdict ov = old_check_head_bytes(bytes, fl, HW, mb);
                const TransposeVerdict nv = transpose_check_head_bytes(bytes, fl, HW, mb);
                EXPECT(ov.code == nv.code && ov.msg == nv.msg, "fl %d HW %zu: '%s' became '%s'", fl, HW, ov.msg.c_str(), nv.msg);
                EXPECT((nv.code == FVVDP_OK) == (d >= 0), "fl %d HW %zu: %zu bytes", fl, HW, bytes);
            }
}

// the vector rule as each entry point stated it, at sizes, strides and pointer offsets on both sides of each alignment
static long check_vector_rule() {
    long n = 0;
    for (int FL : {8, 16, 32, 64}) {
        const size_t pxv = old_pxv(FL);
        for (size_t HW : {(size_t)8, (size_t)9, (size_t)10, (size_t)12, (size_t)35})
            for (size_t fs_extra : {(size_t)0, (size_t)1, (size_t)2, (size_t)4})
                for (size_t cs_extra : {(size_t)0, (size_t)1, (size_t)2, (size_t)4, (size_t)~(size_t)0})        // ~0: one channel, stride 0
                    for (uintptr_t g0_off : {0u, 4u, 8u, 16u})
                        for (uintptr_t head_off : {0u, 4u, 8u, 16u})
                            for (size_t es : {(size_t)4, (size_t)2})
                                for (uintptr_t s_off : {0u, 1u, 2u, 4u, 8u}) {
                                    const size_t frame_stride = HW + fs_extra;
                                    const size_t chan_stride = cs_extra == ~(size_t)0 ? 0 : 5 * frame_stride + cs_extra;
                                    const uintptr_t g0 = 0x10000 + g0_off, head = 0x20000 + head_off;
                                    const uintptr_t test = 0x30000 + s_off * es, grad = 0x40000;
                                    const uintptr_t ptrs = g0 | head, sptrs = test | grad;
                                    // fvvdp_video_grad_input_st
                                    bool o = HW % pxv == 0 && frame_stride % pxv == 0 && chan_stride % pxv == 0 && ptrs % (4 * pxv) == 0 &&
                                             sptrs % (es * pxv) == 0;
                                    EXPECT(transpose_vector_ok(FL, HW, frame_stride | chan_stride, ptrs, sptrs, es) == o, "video: FL %d HW %zu", FL, HW);
                                    // fvvdp_video_grad_luminance (gL among the fp32 buffers)
                                    const uintptr_t lptrs = g0 | head | (0x50000 + s_off * 4);
                                    o = HW % pxv == 0 && lptrs % (4 * pxv) == 0;
                                    EXPECT(transpose_vector_ok(FL, HW, 0, lptrs) == o, "luminance: FL %d HW %zu", FL, HW);
                                    // fvvdp_video_display_sums (the fp32 samples among the fp32 buffers)
                                    const uintptr_t dptrs = g0 | head | (0x30000 + s_off * 4);
                                    o = HW % pxv == 0 && frame_stride % pxv == 0 && chan_stride % pxv == 0 && dptrs % (4 * pxv) == 0;
                                    EXPECT(transpose_vector_ok(FL, HW, frame_stride | chan_stride, dptrs) == o, "display: FL %d HW %zu", FL, HW);
                                    // fvvdp_video_grad_input_held (the head is 256-byte aligned behind a map of a multiple of 256 bytes)
                                    o = HW % pxv == 0 && frame_stride % pxv == 0 && chan_stride % pxv == 0 && g0 % (4 * pxv) == 0 &&
                                        sptrs % (es * pxv) == 0;
                                    EXPECT(transpose_vector_ok(FL, HW, frame_stride | chan_stride, g0, sptrs, es) == o, "held: FL %d HW %zu", FL, HW);
                                    n += 1;
                                }
    }
    return n;
}

int main() {
    static_assert(TRANSPOSE_MAX_FL == 64, "the restatement's arrays");
    static_assert(offsetof(TransposeArgs, tapsT) % 4 == 0, "the taps are read as dwords");
    int cases = 0;
    for (int fl = 1; fl <= 64; ++fl) {
        const int Ns[] = {1, 2, fl - 1, fl, fl + 1, 2 * fl + 3};
        for (int N : Ns) {
            if (N < 1) continue;
            for (int padding = 0; padding < 3; ++padding) {
                check_case(fl, N, padding);
                cases += 1;
            }
        }
    }
    const long rules = check_vector_rule();
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("transpose_host: %d cases, %ld fold lists, %ld vector rules pass\n", cases, lists, rules);
    return 0;
}
