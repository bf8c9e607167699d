"""numpy restatement of the tree the ray tracer's builders produce ("BVH build on the device"): the specification the
device build (nero_bvh_create_device) is compared with bit for bit.  Not a test module: tests/test_bvh_build_cpu.py checks it against
itself and against the host planning code, tests/test_bvh_build_gpu.py checks the library against it.

  * per triangle: centroid ((0 + x0) + x1 + x2) / 3 in fp32, box = exact min / max of the three coordinates (the smaller zero is -0);
  * a range of n <= 4 triangles is a leaf, reference -(lo * 8 + n) - 1; a larger one is sorted (stable, ascending, -0 == +0) on the axis of
    the largest centroid extent (0, then 1 if strictly larger, then 2 if strictly larger) and split at lo + n // 2;
  * nodes in DFS pre-order; a node holds the boxes and references of its two children."""
import functools

import numpy as np

LEAF_MAX = 4
NODE_DT = np.dtype([('lmin', '<f4', 3), ('lmax', '<f4', 3), ('rmin', '<f4', 3), ('rmax', '<f4', 3), ('left', '<i4'), ('right', '<i4'),
                    ('pad', '<i4', 2)])
TRI_DT = np.dtype([('v0', '<f4', 3), ('e1', '<f4', 3), ('e2', '<f4', 3), ('pad', '<f4', 3)])
assert NODE_DT.itemsize == 64 and TRI_DT.itemsize == 48


@functools.lru_cache(maxsize=None)
def inner_count(n):
    """I(n): inner nodes of the subtree over n triangles"""
    return 0 if n <= LEAF_MAX else 1 + inner_count(n // 2) + inner_count(n - n // 2)


def leaf_ref(lo, n):
    return -(lo * 8 + n) - 1


def _ordered(x):
    """order-preserving image of float32 in uint32 (-0 below +0)"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _unordered(k):
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def tmin(x, axis=0):
    return _unordered(_ordered(x).min(axis=axis))


def tmax(x, axis=0):
    return _unordered(_ordered(x).max(axis=axis))


def shape_levels(nT):
    """the tree's shape, a function of nT alone: per level l a dict of arrays over the ranges that exist there -- lo, n, node (pre-order
    index, meaningful where inner) and inner (n > 4) -- computed level by level"""
    lo, n, node = np.zeros(1, np.int64), np.full(1, nT, np.int64), np.zeros(1, np.int64)
    out = []
    while True:
        inner = n > LEAF_MAX
        out.append({'lo': lo, 'n': n, 'node': node, 'inner': inner})
        if not inner.any():
            return out
        lo_i, n_i, node_i = lo[inner], n[inner], node[inner]
        h = n_i // 2
        ih = np.zeros_like(h)
        for u in np.unique(h):                                        # (at most two sizes per level)
            ih[h == u] = inner_count(int(u))
        lo = np.stack([lo_i, lo_i + h], 1).reshape(-1)
        n = np.stack([h, n_i - h], 1).reshape(-1)
        node = np.stack([node_i + 1, node_i + 1 + ih], 1).reshape(-1)


def info(nT):
    """(n_nodes, n_tris, max_depth, root)"""
    levels = shape_levels(nT)
    return inner_count(nT), nT, len(levels) - 1, (leaf_ref(0, nT) if nT <= LEAF_MAX else 0)


def plan_line(nT, lds_capacity):
    """what the host planning program prints for nT (tests/test_bvh_build_cpu.py): the header, the level table a, I(a), I(a + 1) down to the
    first level with a + 1 <= 4, and per level the number of ranges, of inner ones, and the sums of their lo, n and node indices"""
    levels = shape_levels(nT)
    n_levels = len(levels) - 1
    hand_off = 0
    while hand_off < n_levels and -(-nT // (1 << hand_off)) > lds_capacity:
        hand_off += 1
    t = 0
    while (nT >> t) > LEAF_MAX - 1:
        t += 1
    table = ' '.join(f'{nT >> l}:{inner_count(nT >> l)}:{inner_count((nT >> l) + 1)}' for l in range(t + 1))
    stats = ' '.join(f"{len(L['lo'])}:{int(L['inner'].sum())}:{int(L['lo'].sum())}:{int(L['n'].sum())}:{int(L['node'][L['inner']].sum())}"
                     for L in levels)
    root = leaf_ref(0, nT) if nT <= LEAF_MAX else 0
    return f'{nT} {inner_count(nT)} {n_levels} {root} {hand_off} | {table} | {stats}'


def triangle_prep(verts, tris):
    verts = np.ascontiguousarray(verts, np.float32)
    tris = np.ascontiguousarray(tris, np.int32)
    x = verts[tris]                                                   # [nT, corner, axis]
    cen = (((np.float32(0) + x[:, 0]) + x[:, 1]) + x[:, 2]) / np.float32(3)
    assert cen.dtype == np.float32
    return x, cen, tmin(x, axis=1), tmax(x, axis=1)


def pick_axis(c):
    """c: centroids [n, 3] of a range"""
    with np.errstate(invalid='ignore', over='ignore'):
        e = c.max(axis=0) - c.min(axis=0)                             # one fp32 subtraction per axis
    axis = 0
    if e[1] > e[axis]:
        axis = 1
    if e[2] > e[axis]:
        axis = 2
    return axis


def build(verts, tris):
    """-> dict(nodes=bytes, tris=bytes, order=int64 [nT], info=(n_nodes, n_tris, max_depth, root), node_array, tri_array)"""
    x, cen, bmin, bmax = triangle_prep(verts, tris)
    nT = x.shape[0]
    order = np.arange(nT, dtype=np.int64)
    nodes = np.zeros(inner_count(nT), NODE_DT)
    depth = [0]

    def rec(lo, hi, me, level):
        n = hi - lo
        depth[0] = max(depth[0], level)
        idx = order[lo:hi]
        axis = pick_axis(cen[idx])
        order[lo:hi] = idx[np.argsort(cen[idx, axis], kind='stable')]
        h = n // 2
        mid = lo + h
        nodes['lmin'][me], nodes['lmax'][me] = tmin(bmin[order[lo:mid]]), tmax(bmax[order[lo:mid]])
        nodes['rmin'][me], nodes['rmax'][me] = tmin(bmin[order[mid:hi]]), tmax(bmax[order[mid:hi]])
        if h <= LEAF_MAX:
            nodes['left'][me] = leaf_ref(lo, h)
        else:
            nodes['left'][me] = me + 1
            rec(lo, mid, me + 1, level + 1)
        if n - h <= LEAF_MAX:
            nodes['right'][me] = leaf_ref(mid, n - h)
        else:
            nodes['right'][me] = me + 1 + inner_count(h)
            rec(mid, hi, me + 1 + inner_count(h), level + 1)

    if nT > LEAF_MAX:
        rec(0, nT, 0, 1)
        root = 0
    else:
        root = leaf_ref(0, nT)
    rec_t = np.zeros(nT, TRI_DT)
    xo = x[order]
    rec_t['v0'] = xo[:, 0]
    rec_t['e1'] = xo[:, 1] - xo[:, 0]
    rec_t['e2'] = xo[:, 2] - xo[:, 0]
    return {'nodes': nodes.tobytes(), 'tris': rec_t.tobytes(), 'order': order, 'info': (len(nodes), nT, depth[0], root),
            'node_array': nodes, 'tri_array': rec_t}


def leaves(node_array, root):
    """the leaves of a tree as a sorted list of (lo, n); walks the node array from the root"""
    out = []
    stack = [root]
    while stack:
        r = stack.pop()
        if r < 0:
            code = -r - 1
            out.append((code >> 3, code & 7))
        else:
            stack.append(int(node_array[r]['right']))
            stack.append(int(node_array[r]['left']))
    return sorted(out)
