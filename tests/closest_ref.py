"""numpy restatement of the closest-point query (nero_amd/csrc/closest_point_math.h, closest_point.hip; include/nero_closest.h), generic over
the dtype: one numpy operation per operation of the C++ source, in its order, so that in float32 it computes the kernel's bits and in float64
the value they are measured against.  Not a test module: tests/test_closest_point_cpu.py holds walk() to exhaustive() and the stand-alone
host program to point_triangle(); tests/test_closest_point_gpu.py holds the kernel to exhaustive().

  * point_triangle(p, v0, e1, e2)      -> (d2, b1, b2), broadcasting over leading axes
  * exhaustive(points, tri_array, order) -> dict(d2, face, b1, b2, slot): the minimum over ALL triangles, lowest caller face among ties
  * walk(points, tree, pad)              the kernel's walk over tests.tracer_ref.tree(name): its bound, its pad, its order of visits
  * query_set(name, which)               the seeded point sets of the tests; reference(name, which, dtype): exhaustive() over them, cached
  * bounds                               EVAL, EDGE, interior_factor: the derived float32-against-float64 bounds"""
import functools

import numpy as np

from tests import tracer_ref as TR

CP_PAD = 2.0 ** -15                     # closest_point_math.h: CP_PAD
NONE = -(1 << 30)
U = 2.0 ** -24                          # unit roundoff of float32
N_POINTS = 300

# ---- the derived bounds, in units of u * D, D = the distance from the point to the farthest corner of the mesh's box --------
EVAL = 10.0          # computed sqrt(d2) of given weights against the exact distance to the point of the triangle they name
EDGE = 14.0          # how far the computed nearest point of an edge segment lies from the true one, as a length


def interior_factor(s):
    """how far the computed foot of the perpendicular lies from the true one, as a length in units of u D, on a triangle whose edges at v0
    enclose an angle of sine s"""
    return 20.0 + 38.0 / s + 6.0 / (s * s)


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _clamp(t, hi):
    zero = np.zeros((), t.dtype)
    with np.errstate(invalid='ignore'):
        return np.where(t > 0, np.where(t < hi, t, hi), zero)


def _segment(w, e):
    one, zero = np.ones((), w.dtype), np.zeros((), w.dtype)
    len2 = _dot(e, e)
    ok = len2 > 0
    t = _dot(w, e) / np.where(ok, len2, one)
    return np.where(ok, _clamp(t, one), zero)


def _candidate(d, e1, e2, b1, b2, best):
    r = d - (b1[..., None] * e1 + b2[..., None] * e2)
    d2 = _dot(r, r)
    take = d2 < best[0]
    return np.where(take, d2, best[0]), np.where(take, b1, best[1]), np.where(take, b2, best[2])


def point_triangle(p, v0, e1, e2):
    """the arrays broadcast against each other over their leading axes; all of one floating dtype"""
    dt = np.result_type(p, v0)
    assert p.dtype == v0.dtype == e1.dtype == e2.dtype == dt
    one, zero = np.ones((), dt), np.zeros((), dt)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore', under='ignore'):
        d = p - v0
        e1, e2 = np.broadcast_to(e1, d.shape), np.broadcast_to(e2, d.shape)
        z = np.zeros(d.shape[:-1], dt)
        best = (np.full(d.shape[:-1], np.inf, dt), z, z)
        best = _candidate(d, e1, e2, _segment(d, e1), z, best)
        best = _candidate(d, e1, e2, z, _segment(d, e2), best)
        b1 = one - _segment(d - e1, e2 - e1)
        best = _candidate(d, e1, e2, b1, one - b1, best)
        n = _cross(e1, e2)
        nn = _dot(n, n)
        ok = nn > 0
        den = np.where(ok, nn, one)
        lim = one - _clamp(_dot(_cross(d, e2), n) / den, one)
        b2 = _clamp(_dot(_cross(e1, d), n) / den, lim)
        inner = _candidate(d, e1, e2, one - lim, b2, best)
        best = tuple(np.where(ok, a, b) for a, b in zip(inner, best))
    return best


def box_bound(mn, mx, p, pad):
    dt = p.dtype
    g = np.maximum(np.maximum(mn - p, p - mx) - np.asarray(pad, dt), np.zeros((), dt))
    return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


def _records(tri_array, dtype):
    return tuple(np.ascontiguousarray(tri_array[k]).astype(dtype) for k in ('v0', 'e1', 'e2'))


def exhaustive(points, tri_array, order, dtype=np.float32, r2=np.inf, chunk=64):
    """the minimum of point_triangle over every leaf record of tri_array (the triangles AS THE TREE STORES THEM, cast to dtype), accepted on
    d2 < best or (d2 == best and face < best face), face = order[slot]; best starts at r2 with no face.  -> dict of [n] arrays: d2, face
    (-1: nothing within r2), b1, b2, slot"""
    p = np.ascontiguousarray(points).astype(dtype)
    v0, e1, e2 = _records(tri_array, dtype)
    face_of = np.asarray(order, np.int64)
    n = len(p)
    out = {'d2': np.empty(n, dtype), 'b1': np.empty(n, dtype), 'b2': np.empty(n, dtype), 'face': np.empty(n, np.int64), 'slot': np.empty(n, np.int64)}
    for lo in range(0, n, chunk):
        sl = slice(lo, min(n, lo + chunk))
        d2, b1, b2 = point_triangle(p[sl, None, :], v0[None], e1[None], e2[None])
        dmin = d2.min(1)
        tie = d2 == dmin[:, None]
        slot = np.where(tie, face_of[None, :], np.iinfo(np.int64).max).argmin(1)
        rows = np.arange(len(dmin))
        out['d2'][sl], out['b1'][sl], out['b2'][sl] = dmin, b1[rows, slot], b2[rows, slot]
        out['face'][sl], out['slot'][sl] = face_of[slot], slot
    miss = ~(out['d2'] <= np.asarray(r2, dtype))
    out['d2'][miss], out['b1'][miss], out['b2'][miss], out['face'][miss], out['slot'][miss] = np.inf, 0, 0, -1, -1
    return out


def outputs(res, tri_array):
    """(dist, face, bary, point) as nero_bvh_closest writes them, from a float32 result of exhaustive() / walk()"""
    f32 = np.float32
    found = res['face'] >= 0
    slot = np.where(found, res['slot'], 0)
    v0, e1, e2 = (np.ascontiguousarray(tri_array[k], f32)[slot] for k in ('v0', 'e1', 'e2'))
    b1, b2 = res['b1'].astype(f32), res['b2'].astype(f32)
    point = np.where(found[:, None], v0 + (b1[:, None] * e1 + b2[:, None] * e2), f32(0))
    with np.errstate(invalid='ignore'):
        dist = np.where(found, np.sqrt(res['d2'].astype(f32)), f32(np.inf))
    return dist.astype(f32), res['face'].astype(np.int32), np.stack([b1, b2], 1), point.astype(f32)


def walk(points, tree, pad=CP_PAD, dtype=np.float32, r2=np.inf):
    """closest_kernel's walk, all points in step (one node per point and iteration): nearer child first, the left one on equal bounds; a
    child is opened unless its padded bound EXCEEDS the best d2; a deferred sibling travels with its bound and is dropped when popped if the
    best d2 has passed it; the leaves of a node are tested after the next node is chosen.  -> as exhaustive(), plus 'visits' [n]"""
    p = np.ascontiguousarray(points).astype(dtype)
    nodes, tri_array, order = tree['node_array'], tree['tri_array'], np.asarray(tree['order'], np.int64)
    root = tree['info'][3]
    v0, e1, e2 = _records(tri_array, dtype)
    n = len(p)
    best = np.full(n, r2, dtype)
    face = np.full(n, np.iinfo(np.int64).max)
    slot = np.full(n, -1, np.int64)
    b1, b2 = np.zeros(n, dtype), np.zeros(n, dtype)
    visits = np.zeros(n, np.int64)

    def leaf(rows, ref):
        """rows: point indices, ref: their leaf references"""
        code = -ref - 1
        start, count = code >> 3, code & 7
        for i in range(4):
            m = i < count
            r, s = rows[m], start[m] + i
            if len(r) == 0:
                continue
            d2, c1, c2 = point_triangle(p[r], v0[s], e1[s], e2[s])
            f = order[s]
            take = (d2 < best[r]) | ((d2 == best[r]) & (f < face[r]))
            r, s = r[take], s[take]
            best[r], face[r], slot[r], b1[r], b2[r] = d2[take], f[take], s, c1[take], c2[take]

    cur = np.full(n, root, np.int64)
    if root < 0:
        leaf(np.arange(n), cur)
        cur[:] = NONE
    st_node, st_bound, sp = np.zeros((n, 64), np.int64), np.zeros((n, 64), dtype), np.zeros(n, np.int64)
    while True:
        a = np.nonzero(cur != NONE)[0]
        if len(a) == 0:
            break
        visits[a] += 1
        nd = nodes[cur[a]]
        pa, ba = p[a], best[a]
        bl = box_bound(nd['lmin'].astype(dtype), nd['lmax'].astype(dtype), pa, pad)
        br = box_bound(nd['rmin'].astype(dtype), nd['rmax'].astype(dtype), pa, pad)
        swap = br < bl
        first, second = np.where(swap, nd['right'], nd['left']).astype(np.int64), np.where(swap, nd['left'], nd['right']).astype(np.int64)
        bf, bs = np.where(swap, br, bl), np.where(swap, bl, br)
        hf, hs = ~(bf > ba), ~(bs > ba)
        nxt = np.where(hf & (first >= 0), first, NONE)
        leaf_a = np.where(hf & (first < 0), first, NONE)
        leaf_b = np.where(hs & (second < 0), second, NONE)
        inner_s = hs & (second >= 0)
        direct = inner_s & (nxt == NONE)
        nxt = np.where(direct, second, nxt)
        push = inner_s & ~direct
        r = a[push]
        st_node[r, sp[r]], st_bound[r, sp[r]] = second[push], bs[push]
        sp[r] += 1
        while True:                                                  # pop until a deferred subtree still within reach, or the stack is empty
            m = (nxt == NONE) & (sp[a] > 0)
            if not m.any():
                break
            r = a[m]
            sp[r] -= 1
            keep = ~(st_bound[r, sp[r]] > best[r])
            got = np.full(len(r), NONE, np.int64)
            got[keep] = st_node[r[keep], sp[r[keep]]]
            nxt[m] = got
        cur[a] = nxt
        for lf in (leaf_a, leaf_b):
            m = lf != NONE
            if m.any():
                leaf(a[m], lf[m])
    miss = slot < 0
    best[miss], face[miss] = np.inf, -1
    return {'d2': best, 'face': face, 'b1': b1, 'b2': b2, 'slot': slot, 'visits': visits}


# ---- the query sets ------------------------------------------------------------------------------------------------------------------------
SETS = ('vertex', 'edge', 'on_face', 'off_1e-3', 'off_0.1', 'random', 'far', 'origin')


@functools.lru_cache(maxsize=None)
def query_set(name, which, n=N_POINTS):
    """float32 [n,3], read-only, a function of (mesh name, set, n) alone:
      vertex    mesh vertices (every incident face ties)          edge      edge midpoints (rounded to float32)
      on_face   points of faces, up to the rounding to float32    off_*     those moved 1e-3 / 0.1 along the face normal (zero-area faces: along z)
      random    uniform in [-1, 1]^3                              far       normal, scaled by 4
      origin    the origin, then points within 1e-3 of it (on mc_sphere and box nearly every triangle is in play)"""
    sc = TR._Scene(name)
    rg = np.random.default_rng([TR.MESHES.index(name), SETS.index(which), 77])
    if which == 'vertex':
        p = sc.vertices(rg, n)
    elif which == 'edge':
        p = sc.edge_midpoints(rg, n)
    elif which in ('on_face', 'off_1e-3', 'off_0.1'):
        p, t = sc.interior(rg, n)
        if which != 'on_face':
            x = sc.v[sc.f[t]].astype(np.float64)
            nrm = np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0])
            ln = np.linalg.norm(nrm, axis=1, keepdims=True)
            nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1), np.array([0.0, 0.0, 1.0]))
            p = p + nrm * float(which[4:])
    elif which == 'random':
        p = rg.uniform(-1, 1, (n, 3))
    elif which == 'far':
        p = rg.normal(size=(n, 3)) * 4
    else:
        assert which == 'origin', which
        p = rg.uniform(-1e-3, 1e-3, (n, 3))
        p[0] = 0
    p = np.ascontiguousarray(p, np.float32)
    assert p.shape == (n, 3) and np.isfinite(p).all() and np.abs(p).max() <= 20
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def reference(name, which, dtype='float32', n=N_POINTS):
    """exhaustive() over tracer_ref.tree(name) for query_set(name, which, n), computed once and shared; read-only arrays"""
    tree = TR.tree(name)
    res = exhaustive(query_set(name, which, n), tree['tri_array'], tree['order'], np.dtype(dtype).type)
    for a in res.values():
        a.setflags(write=False)
    return res


def scale(points, tri_array):
    """D [n]: per point, its distance to the farthest corner of the triangles' bounding box (float64) -- no corner of a triangle is farther"""
    v0, e1, e2 = _records(tri_array, np.float64)
    corners = np.concatenate([v0, v0 + e1, v0 + e2])
    lo, hi = corners.min(0), corners.max(0)
    p = np.asarray(points, np.float64)
    return np.sqrt((np.maximum(np.abs(p - lo), np.abs(p - hi)) ** 2).sum(1))


def triangle_shape(tri_array, slot):
    """(sine of the angle at v0, inradius) of the stored triangles `slot`, in float64; a zero-area triangle has sine 0 and inradius 0"""
    v0, e1, e2 = (a[slot] for a in _records(tri_array, np.float64))
    area2 = np.linalg.norm(np.cross(e1, e2), axis=1)
    l1, l2, l3 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1), np.linalg.norm(e2 - e1, axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        sine = np.where(l1 * l2 > 0, area2 / (l1 * l2), 0.0)
        inr = np.where(l1 + l2 + l3 > 0, area2 / (l1 + l2 + l3), 0.0)
    return np.minimum(sine, 1.0), inr
