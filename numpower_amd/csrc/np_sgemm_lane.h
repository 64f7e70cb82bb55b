// Where an np_sgemm launch goes when the runtime keeps a side lane (np_runtime.hip, DeviceState::lane): the decision alone,
// free of any device call, so that a host program can run it through a table (tests/test_sgemm_overlap_decide_cpu.py).
//
// The protocol it serves.  Large independent products alternate between the library stream ("main") and ONE side stream:
//   GEMM n   on main, behind an event (main_mark) recorded on main just before it;
//   GEMM n+1 on the lane behind hipStreamWaitEvent(lane, main_mark): it sees everything main was given before n, not n itself,
//            so its workgroups take the CU slots n's workgroups give up while those are still storing C.  An event (lane_mark)
//            is recorded on the lane just before it;
//   GEMM n+2 back on main behind hipStreamWaitEvent(main, lane_mark): behind n by stream order and behind everything the lane was
//            given before n+1, not n+1 itself; and so on, symmetrically.
// So a launch is unordered with respect to the ONE launch before it and nothing else, and only when the two do not touch each
// other's bytes — which is why comparing with that one launch (lane_decide sees no other) is enough: a product four launches
// back on the other stream is behind the mark.  Everything else the library does fetches the main stream through np::stream(),
// which first makes main wait for the lane (the join) and bumps a sequence number; a GEMM that finds the number changed since
// the previous GEMM knows something was enqueued in between that it might depend on, and joins too.  A hazard is never resolved
// by reordering, only by joining.
#ifndef NUMPOWER_AMD_NP_SGEMM_LANE_H
#define NUMPOWER_AMD_NP_SGEMM_LANE_H

#include <stddef.h>
#include <stdint.h>

namespace np {
namespace lane {

// Half-open byte range [lo, hi) an operand may touch; lo == hi: nothing.
struct Range {
    uintptr_t lo, hi;
};

// rows x cols floats, row stride ld floats (ld < cols, rows folded over each other, still spans (rows - 1) * ld + cols)
inline Range range_of(const void *p, size_t rows, size_t ld, size_t cols) {
    const uintptr_t lo = (uintptr_t)p;
    if (rows == 0 || cols == 0) return Range{lo, lo};
    return Range{lo, lo + (uintptr_t)(((rows - 1) * ld + cols) * sizeof(float))};
}

// Two ranges share at least one byte.  Spans, not footprints: a window whose rows interleave with another's (ld > cols)
// counts as touching it, which only ever costs a join.
inline bool touch(Range x, Range y) { return x.lo < x.hi && y.lo < y.hi && x.lo < y.hi && y.lo < x.hi; }

struct Gemm {
    Range a, b, c;
    unsigned long long seq;   // prev: the main-stream sequence number right after it was launched
};

// cur may run unordered next to prev: neither writes what the other reads or writes
inline bool independent(const Gemm &prev, const Gemm &cur) {
    return !touch(cur.c, prev.a) && !touch(cur.c, prev.b) && !touch(cur.c, prev.c) && !touch(prev.c, cur.a) && !touch(prev.c, cur.b);
}

enum Where {
    MAIN_JOINED = 0,        // main, behind everything the lane holds (what every other launch of the library does)
    MAIN_BEHIND_PREV = 1,   // main behind lane_mark, not joined: behind all but the previous GEMM, which runs next to it on the lane
    SIDE = 2,               // the lane behind main_mark: behind all but the previous GEMM, which runs next to it on main
};

enum Flags : unsigned {
    kOwnStream = 1u,      // the library stream is the library's own (np_set_stream installed none)
    kNotCapturing = 2u,   // ... and is not being captured into a graph
    kKnobOn = 4u,         // np_sgemm_set_variant(-28) / NP_SGEMM_OVERLAP
    kBigEnough = 8u,      // flop >= the threshold
    kGate = kOwnStream | kNotCapturing | kKnobOn | kBigEnough,   // all four: the launch may take part at all
    kPrevValid = 16u,     // prev describes a launch that passed the gate
    kPrevOnSide = 32u,    // ... and went to the lane
};

inline Where lane_decide(const Gemm &prev, const Gemm &cur, unsigned long long main_seq, unsigned flags) {
    if ((flags & kGate) != kGate) return MAIN_JOINED;
    if (!(flags & kPrevValid) || prev.seq != main_seq) return MAIN_JOINED;   // first of a run, or the main stream was handed out in between
    if (!independent(prev, cur)) return MAIN_JOINED;
    return (flags & kPrevOnSide) ? MAIN_BEHIND_PREV : SIDE;
}

}  // namespace lane
}  // namespace np

#endif
