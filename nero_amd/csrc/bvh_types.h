// bvh_types.h -- the device tree of the mesh ray tracer, shared by bvh.hip (host build, traversal) and bvh_build.hip (device build)
#pragma once

namespace nero_bvh {

constexpr int NONE = -(1 << 30);          // "no node" sentinel (leaf references are > -2^30: fewer than 2^27 triangles)
constexpr int PL_STACK = 24;              // LDS stack entries per ray (6 KB per workgroup); deeper trees take trace_kernel

struct Node {                 // 64 bytes
    float lmin[3], lmax[3], rmin[3], rmax[3];
    int left, right;          // >= 0: node index; < 0: leaf, -(start*8 + count) - 1
    int pad[2];
};
struct Tri { float v0[3], e1[3], e2[3], pad[3]; };   // 48 bytes, leaf order

struct Bvh {
    Node* d_nodes = nullptr;
    Tri* d_tris = nullptr;
    int* d_face = nullptr;    // [n_tris] leaf slot -> the caller's face index (the builders' leaf-order permutation)
    int n_nodes = 0, n_tris = 0;
};

struct Handle { Bvh b; int root; int max_depth; int mode; };

}  // namespace nero_bvh
