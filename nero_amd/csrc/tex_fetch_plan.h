// tex_fetch_plan.h -- the mip pyramid's level count, sizes and offsets and the argument checks of tex_fetch.hip, free of HIP calls:
// tests/tex_fetch_plan_main.cpp is a stand-alone program over it that the CPU tests build with the address and undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace nero_texfetch {

constexpr int MAX_SIZE = 16384;                                // h and w of level 0 lie in [1, MAX_SIZE], as everywhere in texture.hip
constexpr int MAX_LEVELS = 15;                                 // 1 + log2(MAX_SIZE)
constexpr int RECORD_BYTES = 8;                                // (r, g, b, metallic, roughness, 0, 0, 0): a tap is one 8-byte load
constexpr int THREADS = 256;                                   // a workgroup; the 256-entry table is staged by one thread per entry
constexpr int64_t MAX_COUNT = 2147483647ll;                    // counts stay below it: an index fits an int32 with room for a sentinel
constexpr int NO_OWNER = 2147483647;                           // owner_ws of a vertex no face names

inline bool size_ok(int64_t h, int64_t w) { return h >= 1 && w >= 1 && h <= MAX_SIZE && w <= MAX_SIZE; }
inline bool count_ok(int64_t n) { return n >= 0 && n < MAX_COUNT; }
inline bool corners_ok(int64_t T) { return T >= 0 && T < MAX_COUNT / 3; }       // a corner number 3 f + c fits an int32 below NO_OWNER

// A level exists while both sizes of the one below are even: 1 + min(ctz(h), ctz(w)), capped; 0 for a size out of range.
inline int levels(int64_t h, int64_t w) {
    if (!size_ok(h, w)) return 0;
    int L = 1;
    while (L < MAX_LEVELS && h % 2 == 0 && w % 2 == 0) {
        h /= 2;
        w /= 2;
        ++L;
    }
    return L;
}

// The pyramid of one map: level k is h[k] x w[k] records and begins at record off[k]; the levels lie back to back, level 0 first.
struct Plan {
    int L;
    int h[MAX_LEVELS], w[MAX_LEVELS];
    int64_t off[MAX_LEVELS];
    int64_t records;                                           // of all levels: below 4/3 2^28
};

inline bool make_plan(int64_t h, int64_t w, Plan* P) {
    *P = Plan{};
    P->L = levels(h, w);
    if (P->L == 0) return false;
    int64_t at = 0;
    for (int k = 0; k < P->L; ++k) {
        P->h[k] = (int)(h >> k);
        P->w[k] = (int)(w >> k);
        P->off[k] = at;
        at += (int64_t)P->h[k] * P->w[k];
    }
    P->records = at;
    return true;
}

inline size_t pyramid_bytes(int64_t h, int64_t w) {
    Plan P;
    return make_plan(h, w, &P) ? (size_t)P.records * RECORD_BYTES : 0;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + THREADS - 1) / THREADS); }   // n < 2^31: below 2^23 workgroups

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace nero_texfetch
