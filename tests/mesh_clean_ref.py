"""CPU restatement of the mesh clean-up (nero_amd/csrc/mesh_clean.hip, include/nero_hip.h nero_mesh_*), built on an independent
implementation of the graph step: scipy.sparse.csgraph.connected_components.  Same conventions: components numbered in ascending order of
their smallest vertex, a face belongs to the component of its first vertex, float64 areas from the float32 vertices, exact float32 boxes,
compaction that keeps the survivors in their original relative order and always drops unreferenced vertices.  Plus the inputs the clean-up
tests share."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components as _scipy_cc

from tests import mcubes_ref as R


def components(n_verts, f):
    """-> (comp int32 [V], K): scipy's partition, renumbered by smallest vertex"""
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    V = int(n_verts)
    if V == 0:
        return np.zeros(0, np.int32), 0
    a = np.concatenate([f[:, 0], f[:, 1]])
    b = np.concatenate([f[:, 1], f[:, 2]])
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(V, V))
    K, lab = _scipy_cc(g, directed=False)
    first = np.full(K, V, np.int64)
    np.minimum.at(first, lab, np.arange(V))                          # the smallest vertex of each of scipy's components
    rank = np.empty(K, np.int64)
    rank[np.argsort(first)] = np.arange(K)
    return rank[lab].astype(np.int32), int(K)


def labels(comp):
    """comp [V] -> label [V] = the smallest vertex of the vertex's component (what nero_mesh_cc_label writes)"""
    comp = np.asarray(comp)
    K = int(comp.max()) + 1 if len(comp) else 0
    first = np.full(K, len(comp), np.int64)
    np.minimum.at(first, comp, np.arange(len(comp)))
    return first[comp].astype(np.int32)


def stats(v, f):
    """-> dict(comp, K, n_verts int32 [K], n_faces int32 [K], area float64 [K], bbox_min / bbox_max float32 [K,3])"""
    v = np.asarray(v, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    comp, K = components(len(v), f)
    fc = comp[f[:, 0]] if len(f) else np.zeros(0, np.int64)
    p = v.astype(np.float64)
    tri_area = 0.5 * np.linalg.norm(np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]), axis=1) if len(f) else np.zeros(0)
    lo = np.full((K, 3), np.inf, np.float32)
    hi = np.full((K, 3), -np.inf, np.float32)
    np.minimum.at(lo, comp, v)
    np.maximum.at(hi, comp, v)
    return {'comp': comp, 'K': K, 'n_verts': np.bincount(comp, minlength=K).astype(np.int32),
            'n_faces': np.bincount(fc, minlength=K).astype(np.int32), 'area': np.bincount(fc, weights=tri_area, minlength=K).astype(np.float64),
            'bbox_min': lo, 'bbox_max': hi}


def select(n_faces, keep=None, min_faces=0, min_face_ratio=0.0):
    """the selection rules on face counts [K] -> bool [K]: keep = 'largest' or k: the k components with the most faces, ties towards the
    smaller number; min_faces; min_face_ratio of the largest count (float64); intersected"""
    n = np.asarray(n_faces, dtype=np.int64)
    flags = np.ones(len(n), bool)
    if len(n) == 0:
        return flags
    if keep is not None:
        k = 1 if keep == 'largest' else int(keep)
        order = sorted(range(len(n)), key=lambda c: (-int(n[c]), c))
        flags[:] = False
        flags[order[:k]] = True
    if min_faces:
        flags &= n >= min_faces
    if min_face_ratio:
        flags &= n.astype(np.float64) >= np.float64(min_face_ratio) * np.float64(n.max())
    return flags


def compact(v, f, comp, flags):
    """-> (verts', tris' int32, vmap int32 [V]): the faces of the kept components and the vertices they use, original relative order"""
    v = np.asarray(v).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    fk = np.asarray(flags, bool)[comp[f[:, 0]]] if len(f) else np.zeros(0, bool)
    used = np.zeros(len(v), bool)
    used[f[fk].ravel()] = True
    vmap = np.where(used, np.cumsum(used) - 1, -1).astype(np.int32)
    return v[used], vmap[f[fk]].astype(np.int32).reshape(-1, 3), vmap


def clean(v, f, **rules):
    s = stats(v, f)
    return compact(v, f, s['comp'], select(s['n_faces'], **rules))


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------------
def random_field(shape, seed, thr=0.0):
    """as _random_field of tests/test_mcubes_gpu.py"""
    rg = np.random.default_rng(seed)
    u = rg.uniform(-1, 1, shape).astype(np.float32)
    u[rg.random(shape) < 0.05] = np.float32(thr)
    return u


RANDOM_SHAPES = {(24, 20, 18): 50, (40, 33, 27): 200, (2, 9, 11): 5}   # shape -> the least K the case must have (seed = sum(shape))

_cache = {}


def mesh_of(name):
    """the marching-cubes mesh (tests/mcubes_ref.marching_cubes) of a fixture of mcubes_ref.FIXTURES, of a random field given by its
    shape, or of 'tube'; computed once and shared read-only"""
    if name not in _cache:
        if name == 'tube':
            u = tube_field()
        elif isinstance(name, tuple):
            u = random_field(name, sum(name))
        else:
            u = R.FIXTURES[name][0]()
        v, f = R.marching_cubes(u, 0.0)
        v.setflags(write=False)
        f.setflags(write=False)
        _cache[name] = (v, f)
    return _cache[name]


def ref_stats(name):
    key = ('stats', name)
    if key not in _cache:
        _cache[key] = stats(*mesh_of(name))
    return _cache[key]


def tube_field(shape=(64, 48, 12), radius=2.2):
    """a tube around the polyline that runs along x from 6 to 57 and back on the rows y = 6, 14, 22, 30, 38 at z = 5.5: one long thin
    component (5208 vertices, 10412 triangles, vertex 0 is 265 edges from the farthest vertex)"""
    rows = [6.0, 14.0, 22.0, 30.0, 38.0]
    pts = []
    for i, y in enumerate(rows):
        xs = (6.0, 57.0) if i % 2 == 0 else (57.0, 6.0)
        pts += [(xs[0], y), (xs[1], y)]
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')
    d2 = np.full(shape, np.inf)
    for (ax, ay), (bx, by) in zip(pts[:-1], pts[1:]):
        ex, ey = bx - ax, by - ay
        t = np.clip(((x - ax) * ex + (y - ay) * ey) / (ex * ex + ey * ey), 0.0, 1.0)
        d2 = np.minimum(d2, (x - ax - t * ex) ** 2 + (y - ay - t * ey) ** 2)
    return (np.sqrt(d2 + (z - 5.5) ** 2) - radius).astype(np.float32)


def graph_eccentricity(n_verts, f, source=0):
    """the largest number of edges on a shortest path from `source` (breadth-first over the triangle edges)"""
    from scipy.sparse.csgraph import shortest_path
    f = np.asarray(f, dtype=np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    g = coo_matrix((np.ones(len(a)), (a, b)), shape=(n_verts, n_verts)).tocsr()
    d = shortest_path(g, method='D', directed=False, unweighted=True, indices=source)
    return int(d[np.isfinite(d)].max())
