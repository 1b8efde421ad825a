// rsc_arena.h — layout arithmetic of the batched matchers' staging arena, host only
// and free of HIP.  One device buffer with a pinned mirror holds, in this order,
//     problem table | uploaded inputs   [0, up)      host -> device before the launch
//     scratch                           [up, back)   never copied
//     outputs | count words             [back, bytes) device -> host after the launch
// and every section is problem-major: all problems' uploaded pieces, then all scratch, then all outputs.
// A cursor hands the pieces out in that order; the entry point marks where the two copies end and begin.
#pragma once
#include <cstddef>

namespace rsc {

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Arena {
    size_t off = 0;  // the cursor
    size_t up = 0, back = 0, bytes = 0;
    // a piece at the cursor; the cursor moves on to the next 256-byte boundary
    size_t take(size_t n) {
        const size_t o = off;
        off = al256(off + n);
        return o;
    }
    // the count words that close a problem's outputs: no padding behind them, so the next problem's
    // outputs start where they end (a multiple of their own size, not of 256)
    size_t take_packed(size_t n) {
        const size_t o = off;
        off += n;
        return o;
    }
    void end_upload() { up = off; }
    void end_scratch() { back = off; }
    void finish() { bytes = al256(off); }
};

}  // namespace rsc
