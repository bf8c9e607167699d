// ws_plan.h -- host-side arithmetic of the workspaces: alignment, launch counts, the carving of one allocation into arrays and the bound on
// a device sort's scratch.  No HIP include in here: bvh_build_plan.h (and with it the stand-alone host program of
// tests/test_bvh_build_cpu.py) compiles it with a plain C++ compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace nero_ws {

constexpr size_t align256(size_t x) { return (x + 255) / 256 * 256; }

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }  // launches of 256 threads

inline int bit_length(int64_t x) {
    int n = 0;
    while (x > 0) {
        ++n;
        x >>= 1;
    }
    return n;
}

// consecutive 256-byte-aligned arrays of one allocation: take() returns the offset of the next one
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t here = at;
        at += align256(bytes);
        return here;
    }
};

// The scratch of the scans and sorts where a workspace must grow with its mesh.  hipCUB chooses its algorithm, and with it its scratch, by the
// item count, and the answer is not monotone in it; such a workspace must be (a caller may size it once for its largest mesh), so the
// scratch is an explicit bound: a copy of the keys and values (the merge-sort and the out-of-place passes), and the histograms and look-back
// words of the radix passes.  The checked calls of cub_calls.h compare it with the call's own query before anything runs.
inline size_t sort_temp_bound(int64_t items, size_t bytes_per_item) { return align256((size_t)items * (bytes_per_item + 4) + ((size_t)4 << 20)); }

}  // namespace nero_ws
