"""Brute-force closest-hit ray/mesh oracle (Moeller-Trumbore over every triangle, float64).  TEST INFRASTRUCTURE ONLY.
The reference's tracer is the un-vendored third-party `_raytracing` CUDA extension (no source, no pin, no tests under
/root/reference): parity of the HIP BVH is therefore pinned against this restatement of the contract NeRO relies on
(raytracing/raytracer.py:21-54; network/renderer.py:719-729): closest hit with t > 0, geometric face normal from the vertex
winding, depth >= 10 <=> miss.  'parity unpinned' w.r.t. the third-party binary itself."""
import os
import platform

import numpy as np


def trace_bruteforce(verts, tris, o, d, miss_depth=10.0):
    v0 = verts[tris[:, 0]].astype(np.float64)
    e1 = verts[tris[:, 1]].astype(np.float64) - v0
    e2 = verts[tris[:, 2]].astype(np.float64) - v0
    o = o.astype(np.float64)
    d = d.astype(np.float64)
    n = o.shape[0]
    depth = np.full(n, miss_depth)
    tri = np.full(n, -1, np.int64)
    for r in range(n):
        p = np.cross(d[r], e2)
        det = np.einsum('ij,ij->i', e1, p)
        ok = np.abs(det) > 1e-20
        inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
        tv = o[r] - v0
        u = np.einsum('ij,ij->i', tv, p) * inv
        q = np.cross(tv, e1)
        v = (q @ d[r]) * inv
        t = np.einsum('ij,ij->i', e2, q) * inv
        hit = ok & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < miss_depth)
        if hit.any():
            tt = np.where(hit, t, np.inf)
            k = int(np.argmin(tt))
            depth[r], tri[r] = tt[k], k
    nrm = np.zeros((n, 3))
    h = tri >= 0
    nn = np.cross(e1[tri[h]], e2[tri[h]])
    nrm[h] = nn / np.linalg.norm(nn, axis=1, keepdims=True)
    pos = o + depth[:, None] * d
    return pos, nrm, depth, tri


_C_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc', 'tracer_oracle.c')
_C_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), '_build', 'libtracer_oracle.so')


# -ffp-contract=off: the float32 tracer model below fuses exactly the multiply-adds the kernels write out as fmaf, and no others.
# -mfma (x86-64 only): fmaf as one instruction instead of a libm call -- the same correctly rounded result, ~20x faster.
C_FLAGS = ['-O2', '-ffp-contract=off', '-fopenmp', '-shared', '-fPIC'] + (['-mfma'] if platform.machine() in ('x86_64', 'AMD64') else [])


def build_c(force=False):
    """gcc-compile oracle/csrc/tracer_oracle.c (the C restatement of trace_bruteforce) into oracle/_build/.  -> library path"""
    import subprocess
    if force or not os.path.exists(_C_LIB) or os.path.getmtime(_C_LIB) < os.path.getmtime(_C_SRC):
        os.makedirs(os.path.dirname(_C_LIB), exist_ok=True)
        subprocess.check_call(['gcc'] + C_FLAGS + ['-o', _C_LIB, _C_SRC, '-lm'])
    return _C_LIB


def trace_bruteforce_margins(verts, tris, o, d, miss_depth=10.0, eps_edge=2e-5, eps_t=2e-6):
    """trace_bruteforce through its C restatement (oracle/csrc/tracer_oracle.c: identical float64 arithmetic and predicates,
    OpenMP over rays; tests/test_tracer_oracle_c.py pins it to the numpy version above), plus a per-ray AMBIGUITY flag: True
    when the fp64 answer sits within `eps_edge` (barycentric units) of a triangle edge that could change the closest hit, or a
    candidate intersection lies within `eps_t` of the ray origin (Stage-II secondary rays start 1e-5 off the surface along the
    direction, network/field.py:859: the triangle they left sits at t = -1e-5 cos(theta), i.e. at ~0 for grazing directions).
    The defaults are ~20x the float32 rounding of Moeller-Trumbore at this scene scale (coordinates ~0.5, ulp 6e-8): a float32
    tracer may legitimately answer differently on exactly those rays and on no others.
    -> pos [n,3], nrm [n,3], depth [n], tri [n], ambiguous [n] bool"""
    import ctypes as C
    lib = C.CDLL(build_c())
    V = np.ascontiguousarray(verts, dtype=np.float32)
    F = np.ascontiguousarray(tris, dtype=np.int32)
    O = np.ascontiguousarray(o, dtype=np.float64)
    D = np.ascontiguousarray(d, dtype=np.float64)
    n = O.shape[0]
    pos, nrm, depth = np.empty((n, 3)), np.empty((n, 3)), np.empty(n)
    tri, amb = np.empty(n, np.int64), np.zeros(n, np.uint8)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.tracer_oracle_trace.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double,
                                        C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = lib.tracer_oracle_trace(P(V), V.shape[0], P(F), F.shape[0], P(O), P(D), n, miss_depth, eps_edge, eps_t, P(pos), P(nrm), P(depth),
                                 P(tri), P(amb))
    assert rc == 0
    return pos, nrm, depth, tri, amb.astype(bool)


# ---- the float32 model of the tracer (oracle/csrc/tracer_oracle.c, second half) --------------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _model_lib(lib_path=None):
    import ctypes as C
    lib = C.CDLL(lib_path or build_c())
    V = C.c_void_p
    lib.tracer_model_brute32.argtypes = [V, C.c_int, V, V, C.c_int64, C.c_float, C.c_double, C.c_int, C.c_double, V, V, V, V, V, V, V]
    lib.tracer_model_walk32.argtypes = [V, V, C.c_int, V, V, C.c_int64, C.c_float, C.c_int, C.c_float, V, V, V, V, V]
    return lib


def box_pad():
    """BOX_PAD of nero_amd/csrc/bvh_walk.h, the length by which box_hit grows every box: read from the header, so that the model follows the
    kernels' constant (0.0 for a header without one: the bare slab test)"""
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'nero_amd', 'csrc', 'bvh_walk.h')) as f:
        m = re.search(r'constexpr\s+float\s+BOX_PAD\s*=\s*([^;]+?)f?\s*;', f.read())
    return float.fromhex(m.group(1)) if m else 0.0


def trace_brute32(tri_records, o, d, tmax=10.0, band=1e-5, max_acc=64, margin=2.0 ** -19, lib_path=None):
    """tri_test of nero_amd/csrc/bvh_walk.h, in float32 with the kernels' operation order, over EVERY triangle record (48 bytes each, leaf
    order, as nero_bvh_export / tests.bvh_build_ref.build give them) in order.
    -> depth [n] float32 (tmax: miss), slot [n] int32 (-1: miss; the first slot with the smallest tt), and the accepted set of every ray:
    n_acc [n] = how many slots pass the predicates with 0 < tt < tmax and tt <= depth + band, acc_slot / acc_t [n, max_acc] the first
    max_acc of them (-1 / NaN beyond) with their own tt.
    t_inside / t_outside [n]: the smallest accepted tt below tmax among the triangles whose reported point o + tt d lies within `margin` of
    the triangle's OWN bounding box / farther outside it (inf: none).  The second kind is tri_test answering for a triangle the ray is
    nowhere near (a ray almost in the triangle's plane, a sliver): no bounding-volume walk can be expected to visit that triangle.
    -> dict(depth, slot, acc_slot, acc_t, n_acc, t_inside, t_outside)"""
    T = np.ascontiguousarray(tri_records)
    assert T.dtype.itemsize == 48
    O, D = _f32(o), _f32(d)
    n = O.shape[0]
    depth, slot = np.empty(n, np.float32), np.empty(n, np.int32)
    acc_slot, acc_t, n_acc = np.empty((n, max_acc), np.int32), np.empty((n, max_acc), np.float32), np.empty(n, np.int32)
    t_in, t_out = np.empty(n, np.float32), np.empty(n, np.float32)
    P = lambda a: a.ctypes.data
    rc = _model_lib(lib_path).tracer_model_brute32(P(T), len(T), P(O), P(D), n, tmax, band, max_acc, margin, P(depth), P(slot), P(acc_slot),
                                                   P(acc_t), P(n_acc), P(t_in), P(t_out))
    assert rc == 0
    return dict(depth=depth, slot=slot, acc_slot=acc_slot, acc_t=acc_t, n_acc=n_acc, t_inside=t_in, t_outside=t_out)


def trace_walk32(node_records, tri_records, root, o, d, tmax=10.0, any_hit=False, pad=None, lib_path=None):
    """The walk of NERO_WALK_PRIVATE (box_hit, ray_inverse, tri_test, the visit order) over an exported tree -- 64-byte node records, 48-byte
    triangle records, the root reference -- and write_hit's position and normal, in float32 operation by operation: what nero_bvh_trace
    has to return bit for bit.  any_hit: the walk ends at the first accepted triangle below tmax (nero_bvh_occluded's flag is slot >= 0).
    pad: box_hit's BOX_PAD (None: the header's).
    -> dict(pos [n,3], nrm [n,3], depth [n] float32, slot [n] int32 leaf order (-1: miss), steps [n] nodes visited)"""
    N, T = np.ascontiguousarray(node_records), np.ascontiguousarray(tri_records)
    assert T.dtype.itemsize == 48 and (len(N) == 0 or N.dtype.itemsize == 64)
    O, D = _f32(o), _f32(d)
    n = O.shape[0]
    pos, nrm, depth = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty(n, np.float32)
    slot, steps = np.empty(n, np.int32), np.empty(n, np.int32)
    P = lambda a: a.ctypes.data
    rc = _model_lib(lib_path).tracer_model_walk32(P(N) if len(N) else None, P(T), int(root), P(O), P(D), n, tmax, int(bool(any_hit)),
                                                  box_pad() if pad is None else pad, P(pos), P(nrm),
                                                  P(depth), P(slot), P(steps))
    assert rc == 0, 'a walk needed more than 64 stack entries'
    return dict(pos=pos, nrm=nrm, depth=depth, slot=slot, steps=steps)
