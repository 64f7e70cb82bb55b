// Stand-alone table test of np::lane::lane_decide / range_of / touch (numpower_amd/csrc/np_sgemm_lane.h): no device, no
// library, built with -fsanitize=address,undefined by tests/test_sgemm_overlap_decide_cpu.py.  Exit status = failed rows.
#include <stdio.h>

#include <initializer_list>

#include "np_sgemm_lane.h"

using namespace np::lane;

namespace {

int failures = 0;

void expect(bool ok, const char *what) {
    if (!ok) {
        ++failures;
        printf("FAILED: %s\n", what);
    }
}

const char *name(Where w) { return w == SIDE ? "SIDE" : w == MAIN_BEHIND_PREV ? "MAIN_BEHIND_PREV" : "MAIN_JOINED"; }

// operands as float offsets into one imaginary arena (the decision only compares addresses)
float *const arena = (float *)(uintptr_t)0x10000000u;

struct Mat {
    size_t at, rows, ld, cols;
};
Range rng(Mat m) { return range_of(arena + m.at, m.rows, m.ld, m.cols); }
Gemm gemm(Mat a, Mat b, Mat c, unsigned long long seq = 0) { return Gemm{rng(a), rng(b), rng(c), seq}; }

void decide(const char *what, const Gemm &prev, const Gemm &cur, unsigned long long main_seq, unsigned flags, Where want) {
    const Where got = lane_decide(prev, cur, main_seq, flags);
    if (got != want) {
        ++failures;
        printf("FAILED: %s: %s, expected %s\n", what, name(got), name(want));
    }
}

}  // namespace

int main() {
    // ---- ranges ----
    {
        const Range r = rng(Mat{0, 4, 8, 8});   // dense 4 x 8
        expect(r.hi - r.lo == 4 * 8 * 4, "dense extent");
        const Range w = rng(Mat{0, 4, 8, 3});   // a window: 3 rows of 8 and 3 more floats
        expect(w.hi - w.lo == (3 * 8 + 3) * 4, "window extent");
        const Range f = rng(Mat{0, 4, 2, 8});   // ld < cols: rows folded over each other
        expect(f.hi - f.lo == (3 * 2 + 8) * 4, "folded extent");
        expect(rng(Mat{5, 0, 8, 8}).lo == rng(Mat{5, 0, 8, 8}).hi, "no rows: empty");
        expect(rng(Mat{5, 8, 8, 0}).lo == rng(Mat{5, 8, 8, 0}).hi, "no columns: empty");
        const Range big = range_of(arena, 70000, 70000, 70000);   // past 2^32 bytes
        expect(big.hi - big.lo == (uintptr_t)70000 * 70000 * 4, "extent past 4 GiB");
    }
    // ---- touch ----
    {
        const Range x = rng(Mat{0, 4, 8, 8});   // floats [0, 32)
        expect(touch(x, x), "a range touches itself");
        expect(!touch(x, rng(Mat{32, 4, 8, 8})) && !touch(rng(Mat{32, 4, 8, 8}), x), "abutting ranges share no byte");
        expect(touch(x, rng(Mat{31, 4, 8, 8})) && touch(rng(Mat{31, 4, 8, 8}), x), "one shared float");
        expect(touch(x, rng(Mat{8, 1, 8, 8})) && touch(rng(Mat{8, 1, 8, 8}), x), "nested");
        expect(!touch(x, rng(Mat{8, 0, 8, 8})) && !touch(rng(Mat{8, 0, 8, 8}), x), "an empty range inside touches nothing");
        expect(!touch(rng(Mat{8, 0, 8, 8}), rng(Mat{8, 0, 8, 8})), "two empty ranges");
        // two windows of one 4 x 8 matrix, columns 0-3 and 4-7: no common byte, but the spans interleave -> dependent (conservative)
        expect(touch(rng(Mat{0, 4, 8, 4}), rng(Mat{4, 4, 8, 4})), "interleaved windows count as touching");
        // ... while the last row of the left window ends where a block behind it starts
        expect(!touch(rng(Mat{0, 4, 8, 4}), rng(Mat{28, 1, 4, 4})), "behind the last row of a window");
        expect(touch(rng(Mat{0, 4, 8, 4}), rng(Mat{27, 1, 4, 4})), "inside the last row of a window");
        // byte granularity: ranges of operands one BYTE apart
        const Range p = Range{100, 104}, q = Range{103, 107}, r = Range{104, 108};
        expect(touch(p, q) && !touch(p, r), "byte granularity");
    }
    // ---- the decision ----
    const Mat A1{0, 16, 16, 16}, B1{256, 16, 16, 16}, C1{512, 16, 16, 16};
    const Mat A2{1024, 16, 16, 16}, B2{1280, 16, 16, 16}, C2{1536, 16, 16, 16};
    const Gemm g1 = gemm(A1, B1, C1, 7), g2 = gemm(A2, B2, C2);
    const unsigned on_main = kGate | kPrevValid, on_side = kGate | kPrevValid | kPrevOnSide;
    decide("independent, previous on main", g1, g2, 7, on_main, SIDE);
    decide("independent, previous on the lane", g1, g2, 7, on_side, MAIN_BEHIND_PREV);
    decide("no previous launch", g1, g2, 7, kGate, MAIN_JOINED);
    decide("no previous launch (stale on-side bit)", g1, g2, 7, kGate | kPrevOnSide, MAIN_JOINED);
    decide("the main stream was handed out in between", g1, g2, 8, on_main, MAIN_JOINED);
    decide("... also with the previous on the lane", g1, g2, 8, on_side, MAIN_JOINED);
    decide("sequence number wrapped", gemm(A1, B1, C1, ~0ull), g2, 0, on_main, MAIN_JOINED);
    decide("sequence number at its largest", gemm(A1, B1, C1, ~0ull), g2, ~0ull, on_main, SIDE);
    for (unsigned missing : {(unsigned)kOwnStream, (unsigned)kNotCapturing, (unsigned)kKnobOn, (unsigned)kBigEnough}) {
        decide("a gate bit missing, previous on main", g1, g2, 7, on_main & ~missing, MAIN_JOINED);
        decide("a gate bit missing, previous on the lane", g1, g2, 7, on_side & ~missing, MAIN_JOINED);
    }
    decide("no flag at all", g1, g2, 7, 0, MAIN_JOINED);
    // hazards: always joined, wherever the previous launch went
    for (unsigned flags : {on_main, on_side}) {
        decide("RAW: C1 is A2", g1, gemm(C1, B2, C2), 7, flags, MAIN_JOINED);
        decide("RAW: C1 is B2", g1, gemm(A2, C1, C2), 7, flags, MAIN_JOINED);
        decide("WAW: same C", g1, gemm(A2, B2, C1), 7, flags, MAIN_JOINED);
        decide("WAR: C2 is A1", g1, gemm(A2, B2, A1), 7, flags, MAIN_JOINED);
        decide("WAR: C2 is B1", g1, gemm(A2, B2, B1), 7, flags, MAIN_JOINED);
        decide("C2 nested in C1", g1, gemm(A2, B2, Mat{512 + 16, 2, 16, 16}), 7, flags, MAIN_JOINED);
        decide("C1 nested in A2", g1, gemm(Mat{256, 48, 16, 16}, B2, C2), 7, flags, MAIN_JOINED);
        decide("C2 starts on A1's last float", g1, gemm(A2, B2, Mat{255, 16, 16, 16}), 7, flags, MAIN_JOINED);
        decide("C2 ends on C1's first float", g1, gemm(A2, B2, Mat{512 - 255, 16, 16, 16}), 7, flags, MAIN_JOINED);
    }
    // The decision sees ONE previous launch.  P0 P1 P2 P3 P4: P4 reading or overwriting C1 (three launches back, on the other stream) is
    // compared with P3 alone and goes next to it; what keeps it behind P1 is not this function but the mark each stream records in
    // front of its launches, which the other stream's next launch waits for (np_runtime.hip; tests/test_gpu_sgemm_overlap.py
    // test_cross_stream_dependencies_three_launches_back).  The rows pin that division of labour.
    {
        const Mat A3{4096, 16, 16, 16}, B3{4352, 16, 16, 16}, C3{4608, 16, 16, 16};
        const Gemm p3 = gemm(A3, B3, C3, 7);
        decide("P4 reads C1, independent of P3 on the lane", p3, gemm(C1, B2, C2), 7, on_side, MAIN_BEHIND_PREV);
        decide("P4 overwrites C1, independent of P3 on the lane", p3, gemm(A2, B2, C1), 7, on_side, MAIN_BEHIND_PREV);
        decide("the same, mirrored: P3 on main", p3, gemm(C1, B2, C2), 7, on_main, SIDE);
    }
    // shared INPUTS are no hazard, nor are outputs that abut
    decide("same A and B, different C", g1, gemm(A1, B1, C2), 7, on_main, SIDE);
    decide("A2 is B1", g1, gemm(B1, A1, C2), 7, on_side, MAIN_BEHIND_PREV);
    decide("C2 abuts C1 from behind", g1, gemm(A2, B2, Mat{768, 16, 16, 16}), 7, on_main, SIDE);
    decide("C2 abuts A1 from the front", gemm(Mat{4096, 16, 16, 16}, B1, C1, 7), gemm(A2, B2, Mat{4096 - 256, 16, 16, 16}), 7, on_main, SIDE);
    // zero-size operands touch nothing
    decide("zero-row C2 inside C1", g1, gemm(A2, B2, Mat{520, 0, 16, 16}), 7, on_main, SIDE);
    decide("zero-column C1 inside A2", gemm(A1, B1, Mat{1030, 16, 16, 0}, 7), g2, 7, on_main, SIDE);
    // windows of wider matrices (ld > cols): spans decide
    decide("C2 = right half of the matrix whose left half is C1", gemm(A1, B1, Mat{2048, 16, 32, 16}, 7), gemm(A2, B2, Mat{2048 + 16, 16, 32, 16}), 7,
           on_main, MAIN_JOINED);
    decide("C2 = a window behind the window C1", gemm(A1, B1, Mat{2048, 16, 32, 16}, 7), gemm(A2, B2, Mat{2048 + 15 * 32 + 16, 16, 32, 16}), 7, on_main, SIDE);
    decide("C2 = a window starting inside the last row of the window A1", gemm(Mat{2048, 16, 32, 16}, B1, C1, 7),
           gemm(A2, B2, Mat{2048 + 15 * 32 + 15, 16, 32, 16}), 7, on_main, MAIN_JOINED);
    // ld < cols: rows folded over each other still span (rows - 1) * ld + cols
    decide("folded A1, C2 on its last float", gemm(Mat{3000, 4, 2, 8}, B1, C1, 7), gemm(A2, B2, Mat{3000 + 13, 2, 2, 2}), 7, on_main, MAIN_JOINED);
    decide("folded A1, C2 just behind it", gemm(Mat{3000, 4, 2, 8}, B1, C1, 7), gemm(A2, B2, Mat{3000 + 14, 2, 2, 2}), 7, on_main, SIDE);
    if (failures) printf("%d rows failed\n", failures);
    else printf("lane_decide: all rows pass\n");
    return failures;
}
