// bvh_build_plan.h -- host-side planning of the device BVH build (bvh_build.hip): the level table, the node count I(n), the walk that
// gives every range its position and its node index, and the carving of the workspace.  No HIP call in here: plain arithmetic, also
// compiled into a stand-alone host program by tests/test_bvh_build_cpu.py (address and undefined-behaviour sanitizers).
//
// The tree of Builder::build (bvh.hip) splits a range of n > 4 triangles at lo + n / 2, so its shape is a function of nT alone:
//   * level l (root = level 0) holds the ranges reached by l splits; their sizes are a_l = nT >> l and a_l + 1, nothing else
//     (halving {a, a + 1} gives {a >> 1, (a >> 1) + 1});
//   * levels 0 .. n_levels - 1 hold inner nodes, n_levels = max_depth = the first l with ceil(nT / 2^l) <= 4.  Every range of a level
//     below n_levels - 1 is inner; on the last one the ranges of 5 are inner and those of 4 (or fewer) are leaves;
//   * nodes are numbered in DFS pre-order: left child = me + 1, right child = me + 1 + I(n / 2), I(n) = 0 for n <= 4, otherwise
//     1 + I(n / 2) + I(n - n / 2).  The table keeps I(a_l) and I(a_l + 1) per level, which is all the walk needs.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "ws_plan.h"

#if defined(__HIPCC__)
#define NERO_BVH_HD __host__ __device__
#else
#define NERO_BVH_HD
#endif

namespace nero_bvh_plan {

constexpr int LEAF_MAX = 4;
constexpr int MAX_LEVELS = 30;                    // nT < 2^27: a_l <= 3 from level 26 on
constexpr int MAX_TRIS = (1 << 27) - 1;           // leaf references -(lo * 8 + n) - 1 must stay above the NONE sentinel, -2^30

struct Level { int a, ia, ib; };                  // the smaller range size of the level, I(a), I(a + 1)

struct Plan {
    int nT, n_levels, n_nodes, root, hand_off, n_table;
    Level lv[MAX_LEVELS];
};

struct Range { int lo, n, node, valid; };         // valid = 0: the path runs through a leaf, no such range

NERO_BVH_HD inline int inner_count(const Plan& p, int l, int n) {          // I(n) for a size n that occurs on level l
    if (n <= LEAF_MAX || l >= p.n_table) return 0;
    return n == p.lv[l].a ? p.lv[l].ia : p.lv[l].ib;
}

// range k of level l (the bits of k, most significant first, are the turns from the root: 0 = left), with its pre-order node index
NERO_BVH_HD inline Range range_of(const Plan& p, int l, int k) {
    Range r = {0, p.nT, 0, 1};
    for (int d = 0; d < l; ++d) {
        if (r.n <= LEAF_MAX) { r.valid = 0; return r; }
        const int h = r.n / 2;
        if ((k >> (l - 1 - d)) & 1) { r.node += 1 + inner_count(p, d + 1, h); r.lo += h; r.n -= h; }
        else { r.node += 1; r.n = h; }
    }
    return r;
}

// the range of level l that holds position i: returns its index k on that level (all levels above must be inner: l <= n_levels - 1 or
// sizes > LEAF_MAX on the way), lo and n by reference.  Stops early at a leaf: then *level is the leaf's level.
NERO_BVH_HD inline int locate(int nT, int l, int i, int* lo, int* n, int* level) {
    int k = 0, a = 0, m = nT, d = 0;
    for (; d < l && m > LEAF_MAX; ++d) {
        const int h = m / 2;
        if (i >= a + h) { a += h; m -= h; k = 2 * k + 1; }
        else { m = h; k = 2 * k; }
    }
    *lo = a; *n = m; *level = d;
    return k;
}

inline int ceil_shift(int n, int l) { return (int)(((int64_t)n + ((int64_t)1 << l) - 1) >> l); }

// lds_capacity: S of the finishing kernel.  hand_off = the first level whose ranges all fit S (they are finished in LDS; the levels above
// are sorted globally), capped at n_levels.
inline bool make_plan(int nT, int lds_capacity, Plan* out) {
    if (nT < 1 || nT > MAX_TRIS || lds_capacity < 2 * LEAF_MAX) return false;
    Plan p = {};
    p.nT = nT;
    int l = 0;
    while (ceil_shift(nT, l) > LEAF_MAX) ++l;
    p.n_levels = l;
    int t = 0;
    while ((nT >> t) > LEAF_MAX - 1) ++t;          // the table runs down to the first level with a + 1 <= 4
    p.n_table = t + 1;
    if (p.n_table > MAX_LEVELS) return false;
    for (int i = 0; i < p.n_table; ++i) p.lv[i].a = nT >> i;
    p.lv[t].ia = p.lv[t].ib = 0;
    for (int i = t - 1; i >= 0; --i) {
        const Level& c = p.lv[i + 1];
        auto I = [&c](int n) { return n <= LEAF_MAX ? 0 : (n == c.a ? c.ia : c.ib); };
        const int a = p.lv[i].a, b = a + 1;
        p.lv[i].ia = a <= LEAF_MAX ? 0 : 1 + I(a / 2) + I(a - a / 2);
        p.lv[i].ib = b <= LEAF_MAX ? 0 : 1 + I(b / 2) + I(b - b / 2);
    }
    p.n_nodes = p.lv[0].ia;
    p.root = nT <= LEAF_MAX ? -(0 * 8 + nT) - 1 : 0;
    int h = 0;
    while (h < p.n_levels && ceil_shift(nT, h) > lds_capacity) ++h;
    p.hand_off = h;
    *out = p;
    return true;
}

// ---- workspace ------------------------------------------------------------------------------------------------------------------------
struct Layout {
    size_t hdr, cen, bmin, bmax, order_a, order_b, key_a, key_b, ext, heap, temp, temp_bytes, total;
    size_t ext_ranges, heap_boxes;
};

inline Layout layout(const Plan& p) {
    Layout w = {};
    nero_ws::Carve c;
    const size_t T = (size_t)p.nT;
    w.hdr = c.take(256);                                        // the bad-triangle counter
    w.cen = c.take(T * 3 * sizeof(float));                      // [3][nT]
    w.bmin = c.take(T * 3 * sizeof(float));                     // [nT][3]
    w.bmax = c.take(T * 3 * sizeof(float));
    w.order_a = c.take(T * sizeof(uint32_t));
    w.order_b = c.take(T * sizeof(uint32_t));
    w.key_a = c.take(T * sizeof(uint64_t));
    w.key_b = c.take(T * sizeof(uint64_t));
    w.ext_ranges = (size_t)1 << (p.hand_off > 0 ? p.hand_off - 1 : 0);          // the widest globally sorted level
    w.ext = c.take(w.ext_ranges * 6 * sizeof(uint32_t));
    w.heap_boxes = (size_t)2 << p.n_levels;                   // box of range k of level l at (1 << l) - 1 + k, levels 0 .. n_levels
    w.heap = c.take(w.heap_boxes * 6 * sizeof(float));
    w.temp_bytes = nero_ws::sort_temp_bound((int64_t)T, 12);
    w.temp = c.take(w.temp_bytes);
    w.total = c.at + 256;                                       // (+ 256: the caller's pointer is aligned up)
    return w;
}

}  // namespace nero_bvh_plan
