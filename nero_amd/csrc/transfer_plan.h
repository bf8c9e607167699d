// transfer_plan.h -- the limits, argument checks and workspace arithmetic of detail_transfer.hip, free of HIP calls.  The pyramid of
// normal-map records has the levels, sizes and offsets of tex_fetch_plan.h's Plan; only the record is smaller.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "normals_plan.h"
#include "tex_fetch_plan.h"

namespace nero_transfer {

constexpr int MAX_CHANNELS = 8;                                // C of nero_mesh_attr_at lies in [1, MAX_CHANNELS]
constexpr int NMAP_RECORD_BYTES = 4;                           // (x, y, z, 0): a tap is one 4-byte load
constexpr int SPACE_TANGENT = 0, SPACE_OBJECT = 1;
constexpr int THREADS = nero_texfetch::THREADS;

inline bool channels_ok(int C) { return C >= 1 && C <= MAX_CHANNELS; }
inline bool space_ok(int space) { return space == SPACE_TANGENT || space == SPACE_OBJECT; }
using nero_texfetch::aligned;
using nero_texfetch::blocks_of;
using nero_texfetch::count_ok;
using nero_texfetch::size_ok;

inline size_t nmap_bytes(int64_t h, int64_t w) {
    nero_texfetch::Plan P;
    return nero_texfetch::make_plan(h, w, &P) ? (size_t)P.records * NMAP_RECORD_BYTES : 0;
}

// the tangent sums: the layout of the vertex-normal sums (normals_plan.h), one triple per UV vertex, and the area mode's term width: a
// component of (t / |t|) |c| is at most max |c| < 2^e in magnitude, so |llrint(x 2^(B - e))| <= 2^B and T of them stay within 2^61
inline size_t tangent_workspace_bytes(int64_t Vt) { return nero_normals::workspace_bytes(Vt); }
inline int tangent_term_bits(int64_t T) { return nero_normals::term_bits(T, nero_normals::WEIGHT_AREA); }

}  // namespace nero_transfer
